"""Oracle of the confidence-weighted joint bilateral filter on an f32 one-channel source under an
8-bit guide (include/vip.h vip_joint_bilateral_run_conf_f32). A plain helper module (not a conftest).

A NumPy restatement of the definition, vectorised over the pixels with a Python loop over the taps
in row-major order, built on tests/f32_oracle.py's fmaf and the handle's LUTs
(oracle.space_lut / oracle.color_lut(768, ...) of the profile):

    p = (c == 0) ? +0 : float32(f * c)                       per pixel, once
    w = ws[ky,kx] * wc[d]                                    per tap
    s = fmaf(p_n, w, s);  sumk = fmaf(c_n, w, sumk)          CUDA profile
    s = s + float32(p_n * w);  sumk = sumk + float32(c_n * w)   CPP profile
    dst = (sumk == 0) ? hole_value : s / sumk;  weight = sumk

Also here: the inputs the CPU and the GPU tests share (`confidence`, `holes_mask`).
"""
import numpy as np

from f32_oracle import fmaf
from oracle import oracle as o


def product(f, c):
    """p of the definition: one binary32 product, +0 where c == 0 (whatever f holds there)."""
    f = np.asarray(f, np.float32)
    c = np.asarray(c, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.where(c == 0, np.float32(0), (f * c).astype(np.float32)).astype(np.float32)


def joint_bilateral_conf(f, c, guide, ksize=9, sigma_space=10.0, sigma_color=30.0, profile=o.CUDA, hole_value=0.0):
    """f, c: (H, W) float32 (c finite, >= 0; f finite where c > 0); guide: (H, W) gray or (H, W, 3)
    uint8. Returns (dst, sumk), both (H, W) float32."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    c = np.ascontiguousarray(c, dtype=np.float32)
    guide = np.ascontiguousarray(guide, dtype=np.uint8)
    h, w = f.shape
    assert c.shape == (h, w) and guide.shape[:2] == (h, w) and (guide.ndim == 2 or guide.shape[2] == 3)
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    wc = o.color_lut(768, sigma_color, profile)
    g = guide.reshape(h, w, -1).astype(np.int32)
    pp = np.pad(product(f, c), r, mode="edge")
    cp = np.pad(c, r, mode="edge")
    gp = np.pad(g, ((r, r), (r, r), (0, 0)), mode="edge")
    s = np.zeros((h, w), np.float32)
    sumk = np.zeros((h, w), np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for ky in range(ksize):
            for kx in range(ksize):
                pn = pp[ky:ky + h, kx:kx + w]
                cn = cp[ky:ky + h, kx:kx + w]
                d = np.abs(gp[ky:ky + h, kx:kx + w] - g).sum(axis=2)
                wgt = (ws[ky, kx] * wc[d]).astype(np.float32)  # float32 * float32
                if profile == o.CUDA:
                    s = fmaf(pn, wgt, s)
                    sumk = fmaf(cn, wgt, sumk)
                else:
                    s = (s + (pn * wgt).astype(np.float32)).astype(np.float32)
                    sumk = (sumk + (cn * wgt).astype(np.float32)).astype(np.float32)
        hole = sumk == 0
        dst = np.where(hole, np.float32(hole_value), (s / np.where(hole, np.float32(1), sumk)).astype(np.float32))
    return dst.astype(np.float32), sumk


# ---- shared inputs ----
def holes_mask(w, h, seed=0):
    """A 0/1 mask with about 40 % random holes plus two all-zero blocks larger than a ksize-9 window
    (14 x 16 and 8 x 12 on 67 x 33; scaled with the frame)."""
    rng = np.random.default_rng(4001 + 13 * w + h + seed)
    m = (rng.random((h, w)) >= 0.4).astype(np.float32)
    bh, bw = max(1, (14 * h) // 33), max(1, (16 * w) // 67)
    m[h // 10: h // 10 + bh, w // 12: w // 12 + bw] = 0
    bh, bw = max(1, (8 * h) // 33), max(1, (12 * w) // 67)
    m[h - bh - h // 10: h - h // 10, w - bw - w // 8: w - w // 8] = 0
    return m


def confidence(kind, w, h):
    """The confidence kinds of the GPU tests, (H, W) float32."""
    rng = np.random.default_rng(733 * w + 17 * h + len(kind))
    if kind == "ones":
        c = np.ones((h, w))
    elif kind == "quarter":
        c = np.full((h, w), 0.25)
    elif kind == "holes":
        c = holes_mask(w, h)
    elif kind == "real":  # [0, 1] with 20 % exact zeros
        c = np.where(rng.random((h, w)) < 0.2, 0.0, rng.uniform(0.0, 1.0, (h, w)))
    elif kind == "tiny":  # p and sumk go subnormal
        c = 10.0 ** rng.uniform(-36, -30, (h, w))
    else:  # the holes mask with -0.0f for its zeros
        assert kind == "negzero"
        c = holes_mask(w, h)
        c = np.where(c == 0, np.float32(-0.0), c)
    return np.ascontiguousarray(c, dtype=np.float32)
