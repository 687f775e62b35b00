"""Oracle of the joint bilateral filter on an f32 one-channel source under an 8-bit guide
(include/vip.h vip_joint_bilateral_run_f32). A plain helper module (not a conftest).

A NumPy restatement of the definition, vectorised over the pixels with a Python loop over the
taps in row-major order: per tap w = ws[ky,kx] * wc[d], s = fmaf(f_n, w, s) (CUDA profile) or
float32(s + float32(f_n * w)) (CPP profile), sumk += w; dst = s / sumk in binary32. The LUTs are
the handle's: oracle.space_lut / oracle.color_lut(768, ...) of the profile.

fmaf: NumPy has none, and float32(float64(n) * w + s) rounds twice (at n = w = 1 + 2^-12,
s = 2^-54 it gives 0x1.002p+0 where fmaf gives 0x1.002002p+0). The emulation forms the product
in float64 (exact: 24 + 24 bits), adds s in float64, recovers the sum's error with TwoSum and,
when the sum is inexact and its last mantissa bit is even, steps it to the neighbour towards the
error (round to odd); the cast to float32 then rounds once. tests/test_f32_oracle.py checks it
against libm's fmaf.
"""
import numpy as np

from oracle import oracle as o


def fmaf(n, w, s):
    """float32(n * w + s) with one rounding, elementwise on float32 arrays."""
    n64, w64, s64 = (np.asarray(x, np.float32).astype(np.float64) for x in (n, w, s))
    with np.errstate(over="ignore", invalid="ignore"):
        p = n64 * w64                      # exact
        t = p + s64
        bb = t - p                         # TwoSum: t + e == p + s exactly
        e = (p - (t - bb)) + (s64 - bb)
        inexact = np.isfinite(t) & (e != 0)
        even = (t.view(np.int64) & 1) == 0
        odd = np.nextafter(t, np.where(e > 0, np.inf, -np.inf))
        t = np.where(inexact & even, odd, t)
        return t.astype(np.float32)


def f2u8(v):
    """The project's f2u8: (uint32)(int)v & 0xff."""
    return (np.asarray(v, np.float32).astype(np.int32) & 0xFF).astype(np.uint8)


def joint_bilateral(f, guide, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA):
    """f: (H, W) float32, finite; guide: (H, W) gray or (H, W, 3) uint8. Returns (H, W) float32."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    guide = np.ascontiguousarray(guide, dtype=np.uint8)
    h, w = f.shape
    assert guide.shape[:2] == (h, w) and (guide.ndim == 2 or guide.shape[2] == 3)
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    wc = o.color_lut(768, sigma_color, profile)
    g = guide.reshape(h, w, -1).astype(np.int32)
    fp = np.pad(f, r, mode="edge")
    gp = np.pad(g, ((r, r), (r, r), (0, 0)), mode="edge")
    s = np.zeros((h, w), np.float32)
    sumk = np.zeros((h, w), np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for ky in range(ksize):
            for kx in range(ksize):
                n = fp[ky:ky + h, kx:kx + w]
                d = np.abs(gp[ky:ky + h, kx:kx + w] - g).sum(axis=2)
                wgt = (ws[ky, kx] * wc[d]).astype(np.float32)  # float32 * float32
                if profile == o.CUDA:
                    s = fmaf(n, wgt, s)
                else:
                    s = (s + (n * wgt).astype(np.float32)).astype(np.float32)
                sumk = (sumk + wgt).astype(np.float32)
        return (s / sumk).astype(np.float32)
