"""Oracle and shapes of joint bilateral upsampling of an interleaved f32 field of 2..4 channels under
an 8-bit guide (include/vip.h vip_upsample_run_f32c). A plain helper module (not a conftest).

The definition ties channel c of the result to vip_upsample_run_f32 on plane c, so the oracle is
tests/upsample_oracle.py's upsample applied per channel; it takes (h, w, C) and returns (H, W, C).
source() builds the low-resolution fields the tests use, whose channels differ from each other in
statistic and seed (f32c_oracle's planes at the low-resolution size). waves(), tile_rows() and
lds_bytes() restate csrc/vip_upsample_f32c.hpp's up_c_waves and csrc/vip_upsample.hpp's UpGeom
(tests/test_upsample_f32c_capi.py holds them against the committed resource table); the tile is
TW = 128 outputs wide for every kernel, so round_shapes' tall(), wide() and rounds() serve as they
are, given tile_rows().
"""
import numpy as np

import f32c_oracle as fo
import upsample_oracle as uo
from oracle import oracle as o

SCALES = uo.SCALES
CHANNELS = (2, 3, 4)
MAX_RADIUS = 4           # csrc/vip_launch.hpp kUpMaxRadius: ksize <= 9 at every channel count
TW = 128                 # csrc/vip_upsample.hpp kUpTW
LDS_BUDGET = 160 * 1024  # csrc/vip_launch.hpp kLdsBudget
LUT_COPIES = 32          # csrc/vip_upsample.hpp kUpCopies


def source(w, h, s, channels, stat=None):
    """(lh, lw, C) float32, the low-resolution field of a w x h output at scale s: channel c is
    f32c_oracle.plane(lw, lh, STATS[c], c) (depth, signed, tiny, depth), or of `stat` for every c."""
    lw, lh = uo.low_size(w, h, s)
    return fo.source(lw, lh, channels, stat)


def upsample(f, g_lo, g_hi, s, ksize=5, sigma_space=1.0, sigma_color=30.0, profile=o.CUDA, with_fallback=False):
    """f: (h, w, C) float32, finite; the guides as upsample_oracle.upsample takes them. Returns
    (H, W, C) float32, and with with_fallback also the (H, W) bool map of the sumk == 0 pixels (the
    weights come from the guides alone: one map for every channel)."""
    f = np.asarray(f, dtype=np.float32)
    assert f.ndim == 3
    outs = [uo.upsample(f[..., c], g_lo, g_hi, s, ksize, sigma_space, sigma_color, profile, with_fallback=True)
            for c in range(f.shape[2])]
    out = np.ascontiguousarray(np.stack([p for p, _ in outs], axis=2))
    assert all(np.array_equal(z, outs[0][1]) for _, z in outs)
    return (out, outs[0][1]) if with_fallback else out


# ---- csrc/vip_upsample.hpp UpGeom and csrc/vip_upsample_f32c.hpp up_c_waves, restated ----
def _round_up(v, m):
    return (v + m - 1) // m * m


def plane_words(radius, s, waves):
    """UpGeom<R, S, WAVES>::ROWS * LS: one LDS plane of a tile of 4 * waves output rows."""
    cw, ch, apron = TW // s, 4 * waves // s, _round_up(radius, 4)
    row = cw + 2 * apron
    stride = {2: _round_up(row, 64), 4: row + 1, 8: _round_up(row - 16, 32) + 16}[s]
    return (ch + 2 * radius) * stride


def lds_bytes_at(channels, s, radius, guide_channels, waves):
    entries = 768 if guide_channels == 3 else 256
    return 4 * (entries * LUT_COPIES + (channels + 1) * plane_words(radius, s, waves))


def waves(channels, s, radius, guide_channels):
    """up_c_waves: 16 where the registers hold the kernel (all but C = 4 from R = 1 at S = 2 and from
    R = 3 at S = 4 and 8) and the guide plane and the C float planes fit LDS beside the LUT, else 8."""
    assert channels in CHANNELS and s in SCALES and 0 <= radius <= MAX_RADIUS and guide_channels in (1, 3)
    if channels == 4 and radius >= (1 if s == 2 else 3):
        return 8
    return 16 if lds_bytes_at(channels, s, radius, guide_channels, 16) <= LDS_BUDGET else 8


def lds_bytes(channels, s, radius, guide_channels):
    return lds_bytes_at(channels, s, radius, guide_channels, waves(channels, s, radius, guide_channels))


def tile_rows(channels, s, radius, guide_channels):
    """Tile height in output rows: 4 per wave (64 or 32)."""
    return 4 * waves(channels, s, radius, guide_channels)


def kernel_name(channels, s, radius, guide_channels, fma):
    return f"vip::upsample_f32c_kernel<{radius}, {s}, {channels}, {guide_channels}, {'true' if fma else 'false'}>"
