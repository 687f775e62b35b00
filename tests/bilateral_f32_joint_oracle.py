"""Oracle of the joint bilateral filter of an f32 one-channel source under an f32 one-channel guide
(include/vip.h vip_bilateral_f32_run_joint). A plain helper module (not a conftest).

tests/bilateral_f32_oracle.py with the distance taken from the guide g and the accumulated value from
the source f: a NumPy restatement of the definition, vectorised over the pixels with a Python loop
over the taps in row-major order. Per tap
  d = |g_n - g_c|, t = min(d * scale, N), i = int(t), a = t - float(i),
  wc = fmaf(a, D[i], L[i]) (CUDA profile) or float32(L[i] + float32(a * D[i])) (CPP profile),
  w = ws[ky,kx] * wc, s = fmaf(f_n, w, s) or float32(s + float32(f_n * w)), sumk += w;
dst = s / sumk in binary32. The tables are bilateral_f32_oracle.tables (value_range spans the guide's
differences), fmaf is f32_oracle.fmaf, the spatial table oracle.space_lut of the profile.

Taps outside the disc (ws == 0) are skipped, for bilateral_f32_oracle's reason: for finite input
such a tap adds f_n * 0 = +-0 to s, which is never -0 itself, and 0 to sumk.
tests/test_bilateral_f32_joint_oracle.py checks this module against a per-pixel, per-tap
transcription that skips nothing.

joint_rows() is the row-band form (vip_bilateral_f32_run_rows_joint): output row i is centred on
row i + src_row0 of both images and every row read of either clamps into [row_lo, row_hi).
"""
import numpy as np

from bilateral_f32_oracle import BINS, tables
from f32_oracle import fmaf
from oracle import oracle as o


def joint_rows(f, g, out_rows, src_row0, row_lo, row_hi, ksize=9, sigma_space=10.0, sigma_color=30.0,
               value_range=255.0, profile=o.CUDA):
    """f, g: (H, W) float32, finite. Returns (out_rows, W) float32."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    assert f.shape == g.shape and f.ndim == 2
    h, w = f.shape
    assert 0 <= row_lo < row_hi <= h and out_rows >= 0
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    scale, L, D = tables(sigma_color, value_range, profile)
    fp = np.pad(f, ((0, 0), (r, r)), mode="edge")
    gp = np.pad(g, ((0, 0), (r, r)), mode="edge")
    rows = np.arange(out_rows) + src_row0
    c = g[np.clip(rows, row_lo, row_hi - 1)]
    s = np.zeros((out_rows, w), np.float32)
    sumk = np.zeros((out_rows, w), np.float32)
    top = np.float32(BINS)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for ky in range(ksize):
            sel = np.clip(rows + ky - r, row_lo, row_hi - 1)
            fblock, gblock = fp[sel], gp[sel]
            for kx in range(ksize):
                if ws[ky, kx] == 0:
                    continue
                n = fblock[:, kx:kx + w]
                d = np.abs(gblock[:, kx:kx + w] - c)
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


def joint(f, g, ksize=9, sigma_space=10.0, sigma_color=30.0, value_range=255.0, profile=o.CUDA):
    """The whole frame: f, g (H, W) float32, finite. Returns (H, W) float32."""
    h = np.asarray(f).shape[0]
    return joint_rows(f, g, h, 0, 0, h, ksize, sigma_space, sigma_color, value_range, profile)
