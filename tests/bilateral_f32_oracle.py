"""Oracle of the self-guided bilateral filter on an f32 one-channel image (include/vip.h
vip_bilateral_f32_run). A plain helper module (not a conftest).

A NumPy restatement of the definition in the style of tests/f32_oracle.py, vectorised over the
pixels with a Python loop over the taps in row-major order. Per tap
  d = |f_n - f_c|, t = min(d * scale, N), i = int(t), a = t - float(i),
  wc = fmaf(a, D[i], L[i]) (CUDA profile) or float32(L[i] + float32(a * D[i])) (CPP profile),
  w = ws[ky,kx] * wc, s = fmaf(f_n, w, s) or float32(s + float32(f_n * w)), sumk += w;
dst = s / sumk in binary32. fmaf is f32_oracle.fmaf. The range table is built here as the
definition states it, with libm's expf and exp (NumPy's own exp loops are not libm's); the spatial
table is oracle.space_lut of the profile.

Taps outside the disc (ws == 0) are skipped: for finite input such a tap adds f_n * 0 = +-0 to s,
which is never -0 itself (it starts at +0 and an exact cancellation gives +0), and 0 to sumk, so
skipping changes no bit. tests/test_bilateral_f32_oracle.py checks this module against a per-pixel,
per-tap transcription that skips nothing.

bilateral_rows() is the row-band form (vip_bilateral_f32_run_rows): output row i is centred on
source row i + src_row0 and every row read clamps into [row_lo, row_hi).
"""
import ctypes
import ctypes.util

import numpy as np

from f32_oracle import fmaf
from oracle import oracle as o

BINS = 1024  # VIP_BILATERAL_F32_BINS

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
_libm.exp.restype, _libm.exp.argtypes = ctypes.c_double, [ctypes.c_double]


def scale_of(value_range):
    """(float)N / value_range, a float division."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        return np.float32(BINS) / np.float32(value_range)


def tables(sigma_color, value_range, profile=o.CUDA):
    """(scale, L, D): L has BINS + 2 entries, D = L[i + 1] - L[i] has BINS + 1 (D[BINS] = 0)."""
    scale = scale_of(value_range)
    two_s2 = np.float32(2) * np.float32(sigma_color) * np.float32(sigma_color)
    cf = np.float32(-1.0) / two_s2
    cd = -1.0 / float(two_s2)
    L = np.empty(BINS + 2, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(BINS + 1):
            v = np.float32(i) / scale
            if profile == o.CPP:
                L[i] = np.float32(_libm.exp(float(v) * float(v) * cd))
            else:
                L[i] = _libm.expf(float(np.float32(np.float32(v * v) * cf)))
    L[BINS + 1] = L[BINS]
    D = (L[1:] - L[:-1]).astype(np.float32)
    return scale, L, D


def bilateral_rows(f, out_rows, src_row0, row_lo, row_hi, ksize=9, sigma_space=10.0, sigma_color=30.0,
                   value_range=255.0, profile=o.CUDA):
    """f: (H, W) float32, finite. Returns (out_rows, W) float32."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    h, w = f.shape
    assert 0 <= row_lo < row_hi <= h and out_rows >= 0
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    scale, L, D = tables(sigma_color, value_range, profile)
    fp = np.pad(f, ((0, 0), (r, r)), mode="edge")
    rows = np.arange(out_rows) + src_row0
    c = f[np.clip(rows, row_lo, row_hi - 1)]
    s = np.zeros((out_rows, w), np.float32)
    sumk = np.zeros((out_rows, w), np.float32)
    top = np.float32(BINS)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for ky in range(ksize):
            block = fp[np.clip(rows + ky - r, row_lo, row_hi - 1)]
            for kx in range(ksize):
                if ws[ky, kx] == 0:
                    continue
                n = block[:, kx:kx + w]
                d = np.abs(n - c)
                t = np.minimum(d * scale, top)
                i = t.astype(np.int32)
                a = t - i.astype(np.float32)
                if profile == o.CUDA:
                    wc = fmaf(a, D[i], L[i])
                else:
                    wc = (L[i] + (a * D[i]).astype(np.float32)).astype(np.float32)
                wgt = (ws[ky, kx] * wc).astype(np.float32)
                if profile == o.CUDA:
                    s = fmaf(n, wgt, s)
                else:
                    s = (s + (n * wgt).astype(np.float32)).astype(np.float32)
                sumk = (sumk + wgt).astype(np.float32)
        return (s / sumk).astype(np.float32)


def bilateral(f, ksize=9, sigma_space=10.0, sigma_color=30.0, value_range=255.0, profile=o.CUDA):
    """The whole frame: f (H, W) float32, finite. Returns (H, W) float32."""
    h = np.asarray(f).shape[0]
    return bilateral_rows(f, h, 0, 0, h, ksize, sigma_space, sigma_color, value_range, profile)
