"""Oracle of the single-channel (8-bit gray) bilateral texture filter: the restriction of the
3-channel oracle to frames with three equal channels. A plain helper module (not a conftest).

The gray filter is, by definition (include/vip.h vip_texture_run_c1), any channel of the
3-channel texture filter on the frame (g, g, g): every stage maps three equal channels to three
equal channels. This is NOT the (g, 0, 0) embedding of the gray bilateral and adaptive filters:
the texture filter couples the channels in the intensity, the gradient magnitude and the guide's
L1 distance. tests/test_gray_texture_oracle.py pins the definition; frame() is the input the CPU
and GPU tests share.
"""
import numpy as np

import gray_adaptive_oracle as gao
from oracle import oracle as o

# gray_adaptive_oracle's statistics that the filter changes at k = 5 (uniform, narrow, step), and:
#   const   : a constant frame (rtv is 0 everywhere: the argmin's all-ties case; the filter is the
#             identity on it). It stands for gray_adaptive_oracle's const255 too.
#   checker : a checkerboard of 4-pixel cells with +-2 noise (texture that the filter removes)
#   speck   : a 128 background with isolated 131 pixels, one per 16 x 16 cell. It replaces
#             gray_adaptive_oracle's impulse / impulse_inv (0 among 255s), which the filter leaves
#             unchanged: under sigma_color sqrt(3) a distance of 3 * 255 weighs exactly 0, so an
#             identity kernel would pass on them (tests/test_gray_texture_oracle.py checks that
#             every statistic kept here except const is changed).
STATS = ("uniform", "narrow", "step", "speck", "const", "checker")
CONSTANT = ("const",)


def frame(w, h, stat="uniform"):
    if stat == "const":
        g = np.full((h, w), 97, np.uint8)
    elif stat == "speck":
        g = np.full((h, w), 128, np.uint8)
        g[5::16, 7::16] = 131
    elif stat == "checker":
        rng = np.random.default_rng(1000 * w + h)
        cells = (np.arange(h)[:, None] // 4 + np.arange(w)[None, :] // 4) & 1
        g = (np.where(cells == 1, 180, 70) + rng.integers(-2, 3, (h, w))).astype(np.uint8)
    elif stat in ("uniform", "narrow", "step"):
        return gao.frame(w, h, stat)
    else:
        raise ValueError(stat)
    g.setflags(write=False)
    return g


def replicate(g):
    """(g, g, g) as an H x W x 3 frame."""
    g = np.asarray(g, np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


def texture3(g, ksize=9, nitr=3, profile=o.CUDA):
    """The 3-channel output on the replicated frame (its channels are equal)."""
    return o.texture(replicate(g), ksize, nitr, profile)


def texture(g, ksize=9, nitr=3, profile=o.CUDA):
    return np.ascontiguousarray(texture3(g, ksize, nitr, profile)[..., 0])
