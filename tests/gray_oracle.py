"""Oracle of the single-channel (8-bit gray) bilateral filters: the embedding over the
3-channel oracle. A plain helper module (not a conftest).

The gray filter is, by definition (include/vip.h vip_bilateral_run_c1), channel 0 of the
3-channel filter on the frame (g, 0, 0): the colour distance |dB| + |dG| + |dR| is then
|dg|, and channel 0's sums are the sums of g. A gray guide G embeds as (G, 0, 0) in the same
way; a 3-channel guide is used as it is. tests/test_gray_oracle.py checks the embedding
against an independent per-pixel restatement.
"""
import numpy as np

from oracle import oracle as o


def embed(g):
    """(H, W) u8 -> (H, W, 3) u8 with channel 0 = g, channels 1 and 2 = 0."""
    g = np.ascontiguousarray(g, dtype=np.uint8)
    assert g.ndim == 2
    out = np.zeros(g.shape + (3,), np.uint8)
    out[..., 0] = g
    return out


def _guide3(guide):
    guide = np.asarray(guide)
    return embed(guide) if guide.ndim == 2 else np.ascontiguousarray(guide, dtype=np.uint8)


def bilateral3(g, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA, guide=None, threads=1):
    """The embedded 3-channel output (channels 1 and 2 are 0)."""
    g3 = None if guide is None else _guide3(guide)
    return o.bilateral(embed(g), ksize, sigma_space, sigma_color, profile, guide=g3, threads=threads)


def bilateral(g, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA, threads=1):
    return np.ascontiguousarray(bilateral3(g, ksize, sigma_space, sigma_color, profile, None, threads)[..., 0])


def joint_bilateral(g, guide, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA, threads=1):
    """guide: (H, W) gray or (H, W, 3)."""
    return np.ascontiguousarray(bilateral3(g, ksize, sigma_space, sigma_color, profile, guide, threads)[..., 0])
