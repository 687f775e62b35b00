"""Oracle of the self-guided bilateral filter on an f32 image of 2 or 3 interleaved channels
(include/vip.h vip_bilateral_f32_run_c). A plain helper module (not a conftest).

tests/bilateral_f32_oracle.py with the colour kernels' range weight: a NumPy restatement of the
definition, vectorised over the pixels with a Python loop over the taps in row-major order. Per tap
  d = |f_0(n) - f_0(c)| + |f_1(n) - f_1(c)| (C = 3: that sum + |f_2(n) - f_2(c)|), every subtract
      and add a binary32 one, the adds left to right,
  t = min(d * scale, N), i = int(t), a = t - float(i),
  wc = fmaf(a, D[i], L[i]) (CUDA profile) or float32(L[i] + float32(a * D[i])) (CPP profile),
  w = ws[ky,kx] * wc, formed once, then for each channel s_c = fmaf(f_c(n), w, s_c) or
  float32(s_c + float32(f_c(n) * w)), and sumk += w once;
dst_c = s_c / sumk in binary32. The tables are bilateral_f32_oracle.tables, the spatial table is
oracle.space_lut of the profile, fmaf is f32_oracle.fmaf.

Taps outside the disc (ws == 0) are skipped, for the reason bilateral_f32_oracle gives: for finite
input such a tap adds +-0 to a sum that is never -0, and 0 to sumk.
tests/test_bilateral_f32c_oracle.py checks this module against a per-pixel, per-tap transcription
that skips nothing.

bilateral_rows() is the row-band form (vip_bilateral_f32_run_rows_c): output row i is centred on
source row i + src_row0 and every row read clamps into [row_lo, row_hi).
"""
import numpy as np

from bilateral_f32_oracle import BINS, tables
from f32_oracle import fmaf
from oracle import oracle as o


def bilateral_rows(f, out_rows, src_row0, row_lo, row_hi, ksize=9, sigma_space=10.0, sigma_color=30.0,
                   value_range=255.0, profile=o.CUDA):
    """f: (H, W, C) float32, finite, C = 2 or 3. Returns (out_rows, W, C) float32."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    h, w, ch = f.shape
    assert ch in (2, 3) and 0 <= row_lo < row_hi <= h and out_rows >= 0
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    scale, L, D = tables(sigma_color, value_range, profile)
    fp = np.pad(f, ((0, 0), (r, r), (0, 0)), mode="edge")
    rows = np.arange(out_rows) + src_row0
    c = f[np.clip(rows, row_lo, row_hi - 1)]
    s = np.zeros((out_rows, w, ch), np.float32)
    sumk = np.zeros((out_rows, w), np.float32)
    top = np.float32(BINS)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for ky in range(ksize):
            block = fp[np.clip(rows + ky - r, row_lo, row_hi - 1)]
            for kx in range(ksize):
                if ws[ky, kx] == 0:
                    continue
                n = block[:, kx:kx + w]
                d = (np.abs(n[..., 0] - c[..., 0]) + np.abs(n[..., 1] - c[..., 1])).astype(np.float32)
                if ch == 3:
                    d = (d + np.abs(n[..., 2] - c[..., 2])).astype(np.float32)
                t = np.minimum(d * scale, top)
                i = t.astype(np.int32)
                a = t - i.astype(np.float32)
                if profile == o.CUDA:
                    wc = fmaf(a, D[i], L[i])
                else:
                    wc = (L[i] + (a * D[i]).astype(np.float32)).astype(np.float32)
                wgt = (ws[ky, kx] * wc).astype(np.float32)
                if profile == o.CUDA:  # every channel under the one weight
                    s = fmaf(n, wgt[..., None], s)
                else:
                    s = (s + (n * wgt[..., None]).astype(np.float32)).astype(np.float32)
                sumk = (sumk + wgt).astype(np.float32)
        return (s / sumk[..., None]).astype(np.float32)


def bilateral(f, ksize=9, sigma_space=10.0, sigma_color=30.0, value_range=255.0, profile=o.CUDA):
    """The whole frame: f (H, W, C) float32, finite. Returns (H, W, C) float32."""
    h = np.asarray(f).shape[0]
    return bilateral_rows(f, h, 0, 0, h, ksize, sigma_space, sigma_color, value_range, profile)
