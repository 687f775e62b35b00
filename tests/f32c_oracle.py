"""Oracle and shapes of the joint bilateral filter on an interleaved f32 source of 2..4 channels under
an 8-bit guide (include/vip.h vip_joint_bilateral_run_f32c). A plain helper module (not a conftest).

The definition ties channel c of the result to vip_joint_bilateral_run_f32 on plane c, so the oracle
is tests/f32_oracle.py's joint_bilateral applied per channel; it takes and returns (H, W, C).
source() builds the fields the tests use, whose channels differ from each other; waves(), copies()
and tile_rows() restate csrc/vip_joint_f32c.hip's F32cForm (tests/test_f32c_capi.py holds them
against the committed resource table). The tile width is 128 for every C, so round_shapes' tall(),
wide() and rounds() serve as they are.
"""
import functools

import numpy as np

import f32_oracle
import round_shapes as rs
from oracle import oracle as o

STATS = ("depth", "signed", "tiny", "depth")  # channel c of source(): the statistic, seeded per c
MAX_KSIZE = {1: 47, 2: 31, 3: 15, 4: 15}      # vip_joint_f32c_max_ksize


def plane(w, h, stat, c):
    """tests/test_gpu_joint_f32.py's _source(w, h, stat), seeded per channel c as well."""
    rng = np.random.default_rng(977 * w + 31 * h + len(stat) + 7919 * c)
    if stat == "depth":
        f = rng.uniform(0.5, 10.0, (h, w))
    elif stat == "signed":
        f = rng.standard_normal((h, w)) * 1000
    else:  # tiny: +-[1e-36, 1e-30], products with the weights go subnormal
        assert stat == "tiny"
        f = rng.choice([-1.0, 1.0], (h, w)) * 10.0 ** rng.uniform(-36, -30, (h, w))
    return np.ascontiguousarray(f, dtype=np.float32)


def source(w, h, channels, stat=None):
    """(H, W, C) float32: channel c is plane(w, h, STATS[c], c), or plane(w, h, stat, c) for every c."""
    return np.ascontiguousarray(np.stack([plane(w, h, stat or STATS[c], c) for c in range(channels)], axis=2))


def joint_bilateral(f, guide, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA):
    """f: (H, W, C) float32, finite; guide: (H, W) gray or (H, W, 3) uint8. Returns (H, W, C) float32."""
    f = np.asarray(f, dtype=np.float32)
    assert f.ndim == 3
    return np.ascontiguousarray(np.stack(
        [f32_oracle.joint_bilateral(f[..., c], guide, ksize, sigma_space, sigma_color, profile)
         for c in range(f.shape[2])], axis=2))


# ---- csrc/vip_joint_f32c.hip F32cForm, restated ----
def max_waves(channels, radius, guide_channels):
    """f32c_max_waves: what the registers hold without scratch."""
    if channels == 2:
        m16, m12 = (2, 8) if guide_channels == 3 else (3, 9)
        return 16 if radius <= m16 else (12 if radius <= m12 else 8)
    if channels == 3:
        return 12 if radius <= 4 else 8
    return 8


@functools.lru_cache(maxsize=None)
def form(channels, radius, guide_channels):
    """(waves, LUT copies): the full LUT while 8 waves fit beside the channels + 1 planes, else
    the copies halved until they do."""
    assert channels in (2, 3, 4) and guide_channels in (1, 3) and 1 <= radius <= MAX_KSIZE[channels] // 2
    entries, full = (768, 16) if guide_channels == 3 else (256, 32)
    cap = max_waves(channels, radius, guide_channels)

    def waves_with(copies):
        return rs.pick_waves(radius, channels + 1, cap, entries * copies)

    if waves_with(full) >= 8:
        copies = full
    elif waves_with(full // 2) >= 8 or full // 2 == 8:
        copies = full // 2
    else:
        copies = full // 4
    return waves_with(copies), copies


def waves(channels, radius, guide_channels):
    return form(channels, radius, guide_channels)[0]


def copies(channels, radius, guide_channels):
    return form(channels, radius, guide_channels)[1]


def tile_rows(channels, radius, guide_channels):
    return rs.RPW * waves(channels, radius, guide_channels)


def switch_ksizes(channels, guide_channels):
    """The ksizes either side of every change of the wave count or the LUT copies."""
    ks = set()
    for r in range(1, MAX_KSIZE[channels] // 2):
        if form(channels, r, guide_channels) != form(channels, r + 1, guide_channels):
            ks |= {2 * r + 1, 2 * r + 3}
    return sorted(ks)
