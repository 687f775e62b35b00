"""Oracle of the single-channel (8-bit gray) adaptive bilateral filter: the embedding over the
3-channel oracle. A plain helper module (not a conftest).

The gray filter is, by definition (include/vip.h vip_adaptive_run_c1), channel 0 of the
3-channel adaptive filter on the frame (g, 0, 0): channels 1 and 2 have n = c = mean = 0, so
they add exact zeros to the colour distance, which is then |(n - c) - o| of channel 0 alone,
and channel 0's sums are the sums of g. tests/test_gray_adaptive_oracle.py checks the
embedding against an independent per-pixel restatement. frame() and lut_indices() are the
inputs the CPU and GPU tests share and the LUT index they reach.
"""
import numpy as np

from gray_oracle import embed
from oracle import oracle as o


STATS = ("uniform", "narrow", "step", "const255", "impulse", "impulse_inv")


def frame(w, h, stat="uniform"):
    """The test inputs, by statistics. impulse: a 255 background with isolated 0 pixels (one per
    16 x 16 cell, so a window of ksize <= 15 holds one at most); impulse_inv: its inverse. With
    c = 0 among 255s the index |n - 2c + mean| comes close to 510: the top of the table."""
    rng = np.random.default_rng(1000 * w + h)
    if stat == "uniform":
        g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif stat == "narrow":
        g = rng.integers(100, 120, (h, w), dtype=np.uint8)
    elif stat == "step":  # two levels (40 | 210) with +-3 noise
        g = (np.where(np.arange(w)[None, :] < w // 2, 40, 210) + rng.integers(-3, 4, (h, w))).astype(np.uint8)
    elif stat == "const255":
        g = np.full((h, w), 255, np.uint8)
    elif stat in ("impulse", "impulse_inv"):
        g = np.full((h, w), 255, np.uint8)
        g[5::16, 7::16] = 0
        if stat == "impulse_inv":
            g = 255 - g
    else:
        raise ValueError(stat)
    g.setflags(write=False)
    return g


def lut_indices(g, ksize):
    """int(dist) of every tap of every pixel, dist = |((float)n - (float)c) - o| in float32:
    an (H, W, k, k) int array."""
    g = np.asarray(g, np.uint8)
    r = ksize // 2
    h, w = g.shape
    pad = np.pad(g, r, mode="edge").astype(np.int32)
    win = np.stack([np.stack([pad[ky:ky + h, kx:kx + w] for kx in range(ksize)], -1) for ky in range(ksize)], -2)
    c = g.astype(np.float32)
    mean = (win.sum((-1, -2)).astype(np.float32) / np.float32(ksize * ksize)).astype(np.float32)
    off = (c - mean).astype(np.float32)
    d0 = (win.astype(np.float32) - c[..., None, None]).astype(np.float32)
    return np.abs((d0 - off[..., None, None]).astype(np.float32)).astype(np.int32)


def adaptive3(g, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA, threads=1):
    """The embedded 3-channel output (channels 1 and 2 are 0)."""
    return o.adaptive(embed(g), ksize, sigma_space, sigma_color, profile, threads=threads)


def adaptive(g, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA, threads=1):
    return np.ascontiguousarray(adaptive3(g, ksize, sigma_space, sigma_color, profile, threads)[..., 0])


def adaptive_rows(g, row0, rows, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA):
    """Rows [row0, row0 + rows) of adaptive(g)."""
    out = o.adaptive_rows(embed(g), row0, rows, ksize, sigma_space, sigma_color, profile)
    return np.ascontiguousarray(out[..., 0])
