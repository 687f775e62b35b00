"""Oracle of joint bilateral upsampling of a low-resolution f32 field under an 8-bit guide
(include/vip.h vip_upsample_run_f32). A plain helper module (not a conftest).

A NumPy restatement of the definition, vectorised over the output pixels with a Python loop over
the taps in row-major order. Per output (x, y): cx = x // s, px = x % s (cy, py likewise); tap
(ky, kx) reads low-resolution cell (clamp(cx + kx), clamp(cy + ky)), weighs it by
wsp * wc[d] with d = the L1 distance of the cell's low-resolution guide pixel to the output's
full-resolution one and wsp = space_weight(ox^2 + oy^2, 2 s sigma_space) for the offset
ox = 2 s kx + (s - 1) - 2 px (oy likewise) in half full-resolution pixels; s = fmaf(f_n, w, s)
(CUDA profile) or float32(s + float32(f_n * w)) (CPP profile), sumk += w; dst = s / sumk, or the
nearest sample f[cy, cx] where sumk == 0.

The LUTs are the handle's: oracle.color_lut(768, ...) and, for the spatial weight, the table
oracle.space_lut(2M + 1, 2 s sigma_space, profile)[M + oy, M + ox] with M >= sqrt(2) *
(2 s R + s - 1), so that every offset used lies inside the table's disc (space_lut zeroes what is
outside); 2 s sigma_space is formed in float32 (exact: a power of two times a float32). fmaf is
f32_oracle's.
"""
import math

import numpy as np

from f32_oracle import fmaf
from oracle import oracle as o

SCALES = (2, 4, 8)


def low_size(width, height, s):
    return -(-width // s), -(-height // s)


def space_table(s, r, sigma_space, profile):
    """(table, M): table[M + oy, M + ox] = space_weight(ox^2 + oy^2, 2 s sigma_space)."""
    m = math.ceil(math.sqrt(2.0) * (2 * s * r + s - 1))
    sig = np.float32(2 * s) * np.float32(sigma_space)
    return o.space_lut(2 * m + 1, float(sig), profile), m


def _prepare(f, g_lo, g_hi, s):
    f = np.ascontiguousarray(f, dtype=np.float32)
    g_lo = np.ascontiguousarray(g_lo, dtype=np.uint8)
    g_hi = np.ascontiguousarray(g_hi, dtype=np.uint8)
    hh, ww = g_hi.shape[:2]
    lw, lh = low_size(ww, hh, s)
    assert s in SCALES and f.shape == (lh, lw) and g_lo.shape[:2] == (lh, lw), (f.shape, g_lo.shape, (lh, lw))
    assert g_lo.ndim == g_hi.ndim and (g_hi.ndim == 2 or (g_hi.shape[2] == 3 and g_lo.shape[2] == 3))
    return f, g_lo.reshape(lh, lw, -1).astype(np.int32), g_hi.reshape(hh, ww, -1).astype(np.int32)


def upsample_sums(f, g_lo, g_hi, s, ksize=5, sigma_space=1.0, sigma_color=30.0, profile=o.CUDA):
    """(s, sumk) of every output pixel, float32 (H, W) each."""
    f, gl, gh = _prepare(f, g_lo, g_hi, s)
    hh, ww = gh.shape[:2]
    lh, lw = f.shape
    r = ksize // 2
    assert ksize % 2 == 1 and 1 <= ksize <= 9
    ws, m = space_table(s, r, sigma_space, profile)
    wc = o.color_lut(768, sigma_color, profile)
    x, y = np.arange(ww), np.arange(hh)
    cx, px, cy, py = x // s, x % s, y // s, y % s
    acc = np.zeros((hh, ww), np.float32)
    sumk = np.zeros((hh, ww), np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for ky in range(-r, r + 1):
            iy = np.clip(cy + ky, 0, lh - 1)
            oy = 2 * s * ky + (s - 1) - 2 * py
            for kx in range(-r, r + 1):
                ix = np.clip(cx + kx, 0, lw - 1)
                ox = 2 * s * kx + (s - 1) - 2 * px
                wsp = ws[(m + oy)[:, None], (m + ox)[None, :]]
                n = f[iy[:, None], ix[None, :]]
                d = np.abs(gl[iy[:, None], ix[None, :]] - gh).sum(axis=2)
                wgt = (wsp * wc[d]).astype(np.float32)
                if profile == o.CUDA:
                    acc = fmaf(n, wgt, acc)
                else:
                    acc = (acc + (n * wgt).astype(np.float32)).astype(np.float32)
                sumk = (sumk + wgt).astype(np.float32)
    return acc, sumk


def upsample(f, g_lo, g_hi, s, ksize=5, sigma_space=1.0, sigma_color=30.0, profile=o.CUDA, with_fallback=False):
    """f: (h, w) float32, finite; g_lo: (h, w[, 3]) uint8; g_hi: (H, W[, 3]) uint8, h = ceil(H / s),
    w = ceil(W / s). Returns (H, W) float32, and with with_fallback also the bool map of the pixels
    that took the sumk == 0 branch."""
    acc, sumk = upsample_sums(f, g_lo, g_hi, s, ksize, sigma_space, sigma_color, profile)
    f = np.ascontiguousarray(f, dtype=np.float32)
    hh, ww = acc.shape
    near = f[(np.arange(hh) // s)[:, None], (np.arange(ww) // s)[None, :]]
    zero = sumk == 0
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        out = np.where(zero, near, (acc / sumk).astype(np.float32)).astype(np.float32)
    return (out, zero) if with_fallback else out


def upsample_scalar(f, g_lo, g_hi, s, ksize=5, sigma_space=1.0, sigma_color=30.0, profile=o.CUDA):
    """The definition transcribed pixel by pixel (slow: small frames only)."""
    f, gl, gh = _prepare(f, g_lo, g_hi, s)
    hh, ww = gh.shape[:2]
    lh, lw = f.shape
    r = ksize // 2
    ws, m = space_table(s, r, sigma_space, profile)
    wc = o.color_lut(768, sigma_color, profile)
    out = np.empty((hh, ww), np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for y in range(hh):
            cy, py = y // s, y % s
            for x in range(ww):
                cx, px = x // s, x % s
                acc, sumk = np.float32(0), np.float32(0)
                for ky in range(-r, r + 1):
                    iy = min(max(cy + ky, 0), lh - 1)
                    oy = 2 * s * ky + (s - 1) - 2 * py
                    for kx in range(-r, r + 1):
                        ix = min(max(cx + kx, 0), lw - 1)
                        ox = 2 * s * kx + (s - 1) - 2 * px
                        d = int(np.abs(gl[iy, ix] - gh[y, x]).sum())
                        wgt = np.float32(ws[m + oy, m + ox] * wc[d])
                        if profile == o.CUDA:
                            acc = fmaf(f[iy, ix], wgt, acc)[()]
                        else:
                            acc = np.float32(acc + np.float32(f[iy, ix] * wgt))
                        sumk = np.float32(sumk + wgt)
                out[y, x] = f[cy, cx] if sumk == 0 else np.float32(acc / sumk)
    return out
