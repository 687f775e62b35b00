"""CPU tests of the single-channel (8-bit gray) adaptive bilateral filter.

1. tests/gray_adaptive_oracle.py -- the embedding of a gray frame g as (g, 0, 0) over the
   3-channel adaptive oracle -- equals an independent per-pixel float32 restatement of the
   definition in include/vip.h (vip_adaptive_run_c1), bit for bit, in both numerics profiles.
   The restatement takes the two LUTs as given (the oracle's LUT builders, 512 colour entries)
   and restates everything per pixel: box mean, offset, distance, weights, sums, rounding.
2. The LUT index int(dist) never exceeds 510, and the impulse frames the GPU test runs reach
   the top of the table.
3. The built library exports the entry points and the Python layer has the methods (fails
   without the feature).
"""
import ctypes
import struct

import numpy as np
import pytest

import gray_adaptive_oracle as gao

F = np.float32


def _fma32(a, b, c):
    """fmaf(a, b, c) for a float32 a in [0, 255] with an integer value, and float32 b, c: the
    product is exact in float64 (8 x 24 bits); the sum is rounded to odd in float64 (TwoSum's
    error term says whether it was inexact), after which the rounding to float32 is correct."""
    p = float(a) * float(b)
    c = float(c)
    hi = p + c
    bb = hi - p
    lo = (p - (hi - bb)) + (c - bb)
    if lo != 0.0 and not struct.unpack("<Q", struct.pack("<d", hi))[0] & 1:
        hi = float(np.nextafter(hi, np.inf if lo > 0 else -np.inf))
    return F(hi)


def _restate(oracle, g, ksize, ss, sc, profile):
    h, w = g.shape
    r = ksize // 2
    space = oracle.space_lut(ksize, ss, profile)
    color = oracle.color_lut(512, sc, profile)
    kk = F(ksize * ksize)
    out = np.zeros((h, w), np.uint8)
    top = 0
    for y in range(h):
        for x in range(w):
            taps = [(ky, kx, int(g[min(max(y + ky, 0), h - 1), min(max(x + kx, 0), w - 1)]))
                    for ky in range(-r, r + 1) for kx in range(-r, r + 1)]
            c = F(g[y, x])
            mean = F(F(sum(n for _, _, n in taps)) / kk)
            off = F(c - mean)
            s = sk = F(0)
            for ky, kx, n in taps:
                dist = abs(F(F(F(n) - c) - off))
                top = max(top, int(dist))
                wt = F(space[ky + r, kx + r] * color[int(dist)])
                s = _fma32(F(n), wt, s) if profile == oracle.CUDA else F(s + F(F(n) * wt))
                sk = F(sk + wt)
            with np.errstate(invalid="ignore", divide="ignore"):
                v = F(F(s / sk) + F(0.5))
            out[y, x] = int(v) if v >= 0 else 0  # NaN (every weight 0) -> 0, as the kernels' conversion
    return out, top


@pytest.mark.parametrize("w,h,k", [(23, 11, 5), (17, 9, 9), (3, 7, 9)])  # the last: width below the radius
@pytest.mark.parametrize("ss,sc", [(10.0, 30.0), (3.0, 200.0)])
@pytest.mark.parametrize("profile", [0, 1])
def test_embedding_equals_per_pixel_restatement(oracle, w, h, k, ss, sc, profile):
    g = oracle.random_u8(w * h).reshape(h, w)
    want, top = _restate(oracle, g, k, ss, sc, profile)
    full = gao.adaptive3(g, k, ss, sc, profile)
    assert not full[..., 1:].any()  # channels 1 and 2 of the embedded output are 0
    assert np.array_equal(full[..., 0], want), np.argwhere(full[..., 0] != want)[:5].tolist()
    assert np.array_equal(gao.adaptive(g, k, ss, sc, profile), want)
    assert np.array_equal(gao.adaptive_rows(g, 2, 4, k, ss, sc, profile), want[2:6])
    assert top <= 510
    assert top == gao.lut_indices(g, k).max()  # the vectorised index count agrees with the loop


@pytest.mark.parametrize("k", [1, 3, 9, 15, 31, 63])
@pytest.mark.parametrize("stat", gao.STATS)
def test_lut_index_stays_inside_512_entries(stat, k):
    assert gao.lut_indices(gao.frame(67, 33, stat), k).max() <= 510


@pytest.mark.parametrize("k", [9, 15])
@pytest.mark.parametrize("stat", ["impulse", "impulse_inv"])
def test_impulse_frames_reach_the_top_of_the_table(stat, k):
    """The GPU test's impulse inputs (67 x 33) exercise the last entries of the 512-entry table."""
    assert gao.lut_indices(gao.frame(67, 33, stat), k).max() >= 500


def test_library_and_python_have_the_gray_adaptive_entry_points():
    import various_image_processings_amd as vip
    from various_image_processings_amd import _lib
    from various_image_processings_amd.filters import _AdaptiveImpl
    handle = ctypes.CDLL(vip.LIB_PATH)
    for name in ("vip_adaptive_run_c1", "vip_adaptive_run_rows_c1"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name
    for m in ("execute_c1", "run_rows_c1"):
        assert callable(getattr(_AdaptiveImpl, m, None)), m
    assert callable(getattr(vip.CudaAdaptiveBilateralFilter, "execute_c1", None))
