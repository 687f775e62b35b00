"""Frames that take the persistent one-channel kernels past one tile per workgroup. A plain helper
module (not a conftest), shared by tests/test_round_shapes.py (CPU: the shapes reach the rounds
they exist for) and tests/test_gpu_c1_rounds.py (GPU: bit-exact parity on those shapes).

vip::gray_kernel, gray_adaptive_kernel, joint_f32_kernel, joint_conf_f32_kernel and
upsample_f32_kernel share one tile loop (csrc/vip_gray.hip:64-111 and its four copies): workgroup b
of min(tiles, CUs) (csrc/vip_launch.hpp:242 persistent_blocks) filters the tiles of the slots
b, b + grid, b + 2 grid, ... and loads the next slot's tile into registers under the current one's
taps. Everything past the loop's `if (next >= a.tiles_total) break;` runs only on a frame of more
tiles than the device has CUs. tile_rows() restates each kernel's tile height from the sources,
tall() and wide() are the two frames that reach the later rounds with few pixels, rounds() counts
what a frame reaches. gray_band() / adaptive_band() are the C oracles' row-band entry points as the
GPU file's row-band cases use them, in_bands() the band form of the NumPy oracles that have none.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import gray_adaptive_oracle as gao
from gray_oracle import embed
from oracle import oracle as o

TW = 128  # tile width of all five kernels: P = 8 outputs per thread, 16 threads per tile row
RPW = 4   # tile rows per wave (csrc/vip_stencil.hpp:101 Geom::RPW = 64 / 16)
KERNELS = ("gray_kernel", "gray_adaptive_kernel", "joint_f32_kernel", "joint_conf_f32_kernel", "upsample_f32_kernel")
MAX_RADIUS = 15  # csrc/vip_launch.hpp:17 kMaxRadius


# ---- pick_waves, restated (csrc/vip_stencil.hpp:98-121, csrc/vip_launch.hpp:21) ----
LDS_BUDGET = 160 * 1024


def _round_up(v, m):
    return (v + m - 1) // m * m


def _stride(radius):
    """Geom<R, 8, 16>::S, the plane's row stride in words."""
    return _round_up(TW + 2 * _round_up(radius, 4), 8) + 4


def lds_bytes(radius, waves, planes, lut_words):
    return 4 * lut_words + 4 * planes * (waves * RPW + 2 * radius) * _stride(radius)


def pick_waves(radius, planes, max_waves, lut_words):
    """Largest wave count (<= max_waves: 16, 12, 8 or 4) whose planes and LUT fit LDS, else 0."""
    for waves in (16, 12, 8, 4):
        if max_waves >= waves and lds_bytes(radius, waves, planes, lut_words) <= LDS_BUDGET:
            return waves
    return 0


def waves(kernel, radius, guide_channels):
    """Waves per workgroup of the radius-specialised kernel."""
    if kernel in ("gray_kernel", "gray_adaptive_kernel", "upsample_f32_kernel"):
        # csrc/vip_gray.hip:38 kGrayWaves, csrc/vip_gray_adaptive.hip:43 kGrayAdaWaves,
        # csrc/vip_upsample.hip:43 kUpWaves: 16 at every radius
        return 16
    if guide_channels not in (1, 3) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError((kernel, radius, guide_channels))
    rgb = guide_channels == 3
    if kernel == "joint_f32_kernel":
        # csrc/vip_joint_f32.hip:59-62 (LUT copies), :69-74 (f32_waves: kF32Max16Gray 12, kF32Max16Rgb 9)
        lut = 768 * 16 if rgb else 256 * 32
        return pick_waves(radius, 2, 16 if radius <= (9 if rgb else 12) else 12, lut)
    if kernel == "joint_conf_f32_kernel":
        # csrc/vip_joint_conf.hip:56-59 (conf_rgb_copies: 8 from R 14), :96-103 (conf_waves:
        # kConfMax16Gray 3, kConfMax16Rgb 2, kConfMax12Gray 9, kConfMax12Rgb 8)
        lut = 768 * (8 if radius >= 14 else 16) if rgb else 256 * 32
        m16, m12 = (2, 8) if rgb else (3, 9)
        return pick_waves(radius, 3, 16 if radius <= m16 else (12 if radius <= m12 else 8), lut)
    raise ValueError(kernel)


def tile_rows(kernel, radius, guide_channels):
    """Tile height in rows: RPW rows per wave.
      gray_kernel             64                csrc/vip_gray.hip:49       TH = WAVES * G::RPW
      gray_adaptive_kernel    4 * kGrayAdaWaves csrc/vip_gray_adaptive.hip:69
      upsample_f32_kernel     64                csrc/vip_upsample.hip:44   kUpTH
      joint_f32_kernel        64 / 48           csrc/vip_joint_f32.hip:94  (f32_waves, :71)
      joint_conf_f32_kernel   64 / 48 / 32      csrc/vip_joint_conf.hip:166 (conf_waves, :99)"""
    return RPW * waves(kernel, radius, guide_channels)


# ---- the frames ----
def tall(cus, th):
    """(width, height) of the narrow frame: one tile column, 2 cus + 10 tiles (two full rounds and a
    third of 10 tiles whose last has 5 rows). Dense pitches 9, 27 and 36 bytes: no dword guide
    load, no float4 load or store, no word store."""
    return 9, th * (2 * cus + 9) + 5


def columns(cus):
    """Tile columns of wide(): the smallest count from 3 up that is coprime to cus (3 unless 3
    divides cus, then 4 unless cus is even), so a workgroup changes column between rounds."""
    c = 3
    while np.gcd(c, cus) != 1:
        c += 1
    return c


def wide(cus, th):
    """(width, height) of the frame of columns(cus) tile columns, the last 4 pixels wide (260 x ...
    at 256 CUs: tiles of 128, 128 and 4 pixels): one full round and a partial second, the last tile
    row 5 rows tall. Dense pitches (260, 780, 1040) are multiples of 4 and 16: dword guide loads,
    float4 source loads and stores, word stores."""
    c = columns(cus)
    return TW * (c - 1) + 4, th * -(-(cus + 26) // c) + 5


def rounds(w, h, th, cus):
    """(tiles, full_rounds, last_round_tiles) of a w x h frame in TW x th tiles on cus CUs."""
    tiles = -(-w // TW) * -(-h // th)
    blocks = min(tiles, cus)
    return tiles, tiles // blocks, tiles % blocks


def band(cus, th):
    """(height, row_lo, row_hi, src_row0, out_rows) of the row-band case on tall(cus, th): the
    neighbour range is narrower than the frame at both ends, the band lies one row inside it at
    both ends (so that the first tile's loads clamp to row_lo and the last, prefetched tile's to
    row_hi - 1 from radius 2 on) and is 2 cus + 9 tiles tall."""
    h = tall(cus, th)[1]
    row_lo, row_hi = 5, h - 7
    src_row0 = row_lo + 1
    return h, row_lo, row_hi, src_row0, row_hi - 1 - src_row0


# ---- the oracles' row-band entry points ----
def gray_band(g, guide, row0, rows, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA):
    """Rows [row0, row0 + rows) of gray_oracle.bilateral(g) (guide None) or joint_bilateral(g, guide)."""
    if guide is None:
        out = o.bilateral_rows(embed(g), row0, rows, ksize, sigma_space, sigma_color, profile)
    else:
        guide = np.asarray(guide)
        g3 = embed(guide) if guide.ndim == 2 else np.ascontiguousarray(guide, dtype=np.uint8)
        out = o.joint_bilateral_rows(embed(g), g3, row0, rows, ksize, sigma_space, sigma_color, profile)
    return np.ascontiguousarray(out[..., 0])


def adaptive_band(g, row0, rows, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA):
    """Rows [row0, row0 + rows) of gray_adaptive_oracle.adaptive(g)."""
    return gao.adaptive_rows(g, row0, rows, ksize, sigma_space, sigma_color, profile)


def in_bands(fn, radius, *planes, threads=8):
    """fn(*planes) of a whole-frame NumPy oracle without a band form (f32_oracle, conf_oracle),
    evaluated band by band in parallel threads (NumPy releases the GIL inside its loops): `threads`
    equal row bands, each run on its rows plus `radius` halo rows either side, clipped at the
    frame's edges -- where the crop's replicate border is the frame's own -- and cut back to the
    band. fn returns one (H, W) array or a tuple of them; so does this."""
    h = planes[0].shape[0]
    cuts = [h * i // threads for i in range(threads + 1)]

    def run(i):
        a, b = cuts[i], cuts[i + 1]
        lo, hi = max(0, a - radius), min(h, b + radius)
        out = fn(*(np.ascontiguousarray(p[lo:hi]) for p in planes))
        return tuple(x[a - lo:b - lo] for x in (out if isinstance(out, tuple) else (out,)))

    with ThreadPoolExecutor(threads) as ex:
        parts = [p for p in ex.map(run, range(threads)) if len(p[0])]
    whole = tuple(np.concatenate(c) for c in zip(*parts))
    return whole if len(whole) > 1 else whole[0]
