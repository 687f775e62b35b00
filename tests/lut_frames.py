"""Frames and sigmas that put the colour LUT's form switches and top entries under test.
A plain helper module (not a conftest), shared by tests/test_lut_frames.py (CPU: the frames
reach the distances they exist for) and tests/test_gpu_lut_forms.py (GPU: bit-exact parity).

The 3-channel joint and adaptive launchers pick the LUT's form from the handle's lut_nonzero,
the index from which the colour LUT is exactly zero (csrc/vip_bilateral.hip launch_bilateral_r,
csrc/vip_adaptive.hip launch_adaptive_r). zero_point() is that index taken from the oracle's
LUT, sigma_with_zero_point() a sigma_color that gives a chosen one; the frame generators make
guides whose tap distances straddle a zero point, and saturated frames whose distances reach
the last LUT entries (765, 1529, 255, 509). joint_distances() / adaptive_distances() restate
the tap distances so that the CPU test can count what each frame reaches.
"""
import functools

import numpy as np

from oracle import oracle as o

W, H = 129, 65  # one 128 x 64 tile plus a column and a row; crosses the 64-pixel adaptive seams
PROFILES = (o.CUDA, o.CPP)


# ---- the LUT's zero point and a sigma_color that has a given one ----
def zero_point(n, sigma, profile):
    """One past the last nonzero entry of oracle.color_lut(n, sigma, profile)."""
    nz = np.flatnonzero(o.color_lut(n, float(np.float32(sigma)), profile))
    return int(nz[-1]) + 1 if len(nz) else 0


def _first_sigma_reaching(n, target, profile):
    """Bit pattern of the smallest float32 sigma in [2^-6, 2^20) whose zero point is >= target
    (positive floats order like their bit patterns; the zero point does not fall as sigma grows)."""
    lo, hi = int(np.float32(2.0 ** -6).view(np.uint32)), int(np.float32(2.0 ** 20).view(np.uint32))
    if zero_point(n, np.uint32(hi).view(np.float32), profile) < target:
        raise ValueError(f"no sigma gives a {n}-entry LUT a zero point of {target}")
    while lo < hi:
        mid = (lo + hi) // 2
        if zero_point(n, np.uint32(mid).view(np.float32), profile) >= target:
            hi = mid
        else:
            lo = mid + 1
    return lo


@functools.lru_cache(maxsize=None)
def sigma_interval(n, target, profile):
    """(first, last) float32 sigma_color, as Python floats, with zero_point(n, ., profile) == target."""
    if not 1 <= target < n:
        raise ValueError("a zero point inside the table: 1 <= target < n")
    a = _first_sigma_reaching(n, target, profile)
    b = _first_sigma_reaching(n, target + 1, profile) - 1
    if b < a:
        raise ValueError(f"no float32 sigma gives a zero point of {target}")
    return float(np.uint32(a).view(np.float32)), float(np.uint32(b).view(np.float32))


@functools.lru_cache(maxsize=None)
def sigma_with_zero_point(n, target, profile):
    """A float32 sigma_color (as a Python float) with zero_point(n, sigma, profile) == target: the
    middle of the interval of such sigmas, found by bisection over oracle.color_lut."""
    a, b = sigma_interval(n, target, profile)
    s = float(np.float32((a + b) / 2))
    if zero_point(n, s, profile) != target:
        raise AssertionError((n, target, profile, a, b, s))
    return s


# ---- the frames (seeded, deterministic, read-only) ----
def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


def _checker(w, h, cell):
    y, x = np.mgrid[0:h, 0:w]
    return ((y // cell + x // cell) & 1).astype(bool)


@functools.lru_cache(maxsize=None)
def noise_guide(amp=20, w=W, h=H, seed=1):
    """Each channel 100 + uniform{0..amp-1}: L1 distances 0..3(amp-1), dense either side of the
    joint filter's switches (26 | 27, 31 | 32) and at the small distances whose weights show."""
    return _ro(100 + np.random.default_rng(seed).integers(0, amp, (h, w, 3)))


@functools.lru_cache(maxsize=None)
def blocks(lo=50, hi=170, cell=8, noise=6, w=W, h=H, seed=2):
    """A cell x cell checker of two levels plus uniform{0..noise-1} per channel. With (50, 170)
    the adaptive distances of the taps across an edge lie around 511."""
    base = np.repeat(np.where(_checker(w, h, cell), hi, lo)[..., None], 3, axis=2)
    if noise:
        base = base + np.random.default_rng(seed).integers(0, noise, (h, w, 3))
    return _ro(base)


def two_level(w=W, h=H):
    """The checker with pure 0 and 255: the L1 distance across an edge is 765 (gray: 255)."""
    return blocks(0, 255, 8, 0, w, h)


def two_level_noisy(w=W, h=H):
    """Levels 0..5 and 250..255: the distances 735..765 (gray 245..255), the LUT's last entries."""
    return blocks(0, 250, 8, 6, w, h, seed=3)


@functools.lru_cache(maxsize=None)
def lone_pixel(negative=False, w=W, h=H):
    """One black pixel at (row 32, column 64) on white, or its negative. In the adaptive filter
    the centre's own offset adds to the tap's difference: at ksize 31 the distance reaches 1529."""
    a = np.full((h, w, 3), 255, np.uint8)
    a[32, 64] = 0
    return _ro(255 - a if negative else a)


@functools.lru_cache(maxsize=None)
def flat(v, w=W, h=H):
    return _ro(np.full((h, w, 3), v, np.uint8))


@functools.lru_cache(maxsize=None)
def random_source(w=W, h=H, seed=4):
    """A full-range random frame that holds both 0 and 255 in every channel."""
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[0, 0], a[h - 1, w - 1] = 0, 255
    return _ro(a)


def gray(frame):
    """A 3-channel frame reduced to its channel 0."""
    return _ro(frame[..., 0])


@functools.lru_cache(maxsize=None)
def blocks_batch():
    """The three frames of a multi-frame launch at the adaptive switch: blocks(), blocks() flipped
    both ways, and its transpose laid back into the frame's shape."""
    f = blocks()
    return f, _ro(f[::-1, ::-1]), _ro(np.ascontiguousarray(f.transpose(1, 0, 2)).reshape(f.shape))


# ---- the tap distances, restated: replicate border, vectorised over the frame, a Python loop
# over the k x k taps. The oracle indexes the LUT at every tap of the square; the kernels run
# over the disc (the spatial weight is zero outside it), so disc=True counts what a kernel reads ----
def _taps(r, disc):
    return [(ky, kx) for ky in range(-r, r + 1) for kx in range(-r, r + 1)
            if not disc or ky * ky + kx * kx <= r * r]


def _disc_taps(r):
    return _taps(r, True)


def _windows(a, r):
    """a (H, W, C) int32 -> the function (ky, kx) -> the frame shifted by that tap, edges replicated."""
    h, w = a.shape[:2]
    pad = np.pad(a, ((r, r), (r, r), (0, 0)), mode="edge")
    return lambda ky, kx: pad[r + ky:r + ky + h, r + kx:r + kx + w]


def joint_distances(guide, r, disc=False):
    """Histogram (766 bins) of the L1 guide distance over all (pixel, tap) pairs of the square of
    radius r, or of its disc; guide (H, W, 3) or gray (H, W)."""
    g = np.asarray(guide)
    g = g.reshape(g.shape[0], g.shape[1], -1).astype(np.int32)
    win = _windows(g, r)
    hist = np.zeros(766, np.int64)
    for ky, kx in _taps(r, disc):
        hist += np.bincount(np.abs(win(ky, kx) - g).sum(axis=2).ravel(), minlength=766)
    return hist


def _adaptive_indices(a, r, disc):
    """(ky, kx, index (H, W)) of every tap: the LUT index as vipo_adaptive_rows forms it, in float32."""
    k = 2 * r + 1
    win = _windows(a, r)
    box = np.zeros_like(a)
    for ky, kx in _taps(r, False):  # the box sum runs over the full square (exact in int32)
        box = box + win(ky, kx)
    off = (a.astype(np.float32) - box.astype(np.float32) / np.float32(k * k)).astype(np.float32)
    for ky, kx in _taps(r, disc):
        d = np.abs((win(ky, kx) - a).astype(np.float32) - off)  # float32 throughout
        dist = d[..., 0]
        for c in range(1, d.shape[2]):
            dist = (dist + d[..., c]).astype(np.float32)
        yield ky, kx, dist.astype(np.int64)


def adaptive_distances(img, r, disc=False):
    """(histogram, dmin): the adaptive filter's LUT index int(sum_c |(n_c - c_c) - (c_c - boxsum_c / k^2)|)
    in float32, the form of vipo_adaptive_rows (oracle/vip_oracle.c), over all (pixel, tap) pairs
    of the square of radius r or of its disc (1536 bins), and per pixel the smallest index among
    its taps of the disc (the taps whose spatial weight is not zero). img (H, W, 3) or gray
    (H, W): a gray frame is the frame (g, 0, 0), whose other channels add exact zeros."""
    a = np.asarray(img)
    a = a.reshape(a.shape[0], a.shape[1], -1).astype(np.int32)
    hist = np.zeros(1536, np.int64)
    dmin = np.full(a.shape[:2], 1 << 30, np.int64)
    for ky, kx, idx in _adaptive_indices(a, r, disc):
        hist += np.bincount(idx.ravel(), minlength=1536)
        if ky * ky + kx * kx <= r * r:
            dmin = np.minimum(dmin, idx)
    return hist, dmin


# ---- float64 filters of the same definitions: exact exp weights, no float32 LUT, so no weight
# is rounded to float32 or flushed to zero; the output rounds as the oracle rounds ----
def _space64(r, sigma_space):
    ws = {}
    for ky, kx in _disc_taps(r):
        ws[ky, kx] = np.exp(-(ky * ky + kx * kx) / (2.0 * float(sigma_space) ** 2))
    return ws


def _round_u8(acc, sumk):
    return np.clip(np.floor(acc / sumk[..., None] + 0.5), 0, 255).astype(np.uint8)


def bilateral_f64(src, ksize, sigma_space, sigma_color, guide=None):
    src = np.asarray(src)
    s = src.astype(np.int32)
    g = s if guide is None else np.asarray(guide).astype(np.int32)
    r = ksize // 2
    ws, ws_, wg = _space64(r, sigma_space), _windows(s, r), _windows(g, r)
    acc, sumk = np.zeros(s.shape, np.float64), np.zeros(s.shape[:2], np.float64)
    for ky, kx in _disc_taps(r):
        d = np.abs(wg(ky, kx) - g).sum(axis=2).astype(np.float64)
        wgt = ws[ky, kx] * np.exp(-d * d / (2.0 * float(sigma_color) ** 2))
        acc += ws_(ky, kx) * wgt[..., None]
        sumk += wgt
    return _round_u8(acc, sumk)


def adaptive_f64(src, ksize, sigma_space, sigma_color):
    """The weight is exp(-i^2 / 2 sigma^2) of the LUT index i, formed as the definition forms it
    (float32, truncated); the table's float32 entries and the float32 sums are what is left out."""
    s = np.asarray(src).astype(np.int32)
    r = ksize // 2
    ws, win = _space64(r, sigma_space), _windows(s, r)
    acc, sumk = np.zeros(s.shape, np.float64), np.zeros(s.shape[:2], np.float64)
    for ky, kx, idx in _adaptive_indices(s, r, True):
        i = idx.astype(np.float64)
        wgt = ws[ky, kx] * np.exp(-i * i / (2.0 * float(sigma_color) ** 2))
        acc += win(ky, kx) * wgt[..., None]
        sumk += wgt
    return _round_u8(acc, sumk)


# ---- the adaptive cases the GPU file runs; the CPU file checks sumk > 0 on each ----
ADAPTIVE_SWITCH_KSIZES = (3, 9, 15, 17, 19)  # the box-sum paths and the square sums
ADAPTIVE_BATCH_KSIZES = (9, 15)              # adaptive_frames_kernel (radius <= 8)
ADAPTIVE_SWITCH = (511, 512)                 # zero points either side of launch_adaptive_r's test


def adaptive_cases(profile):
    """[(label, frame (3-channel or gray), ksize, sigma_color)]: every adaptive run of
    tests/test_gpu_lut_forms.py in this profile."""
    out = []
    for zp in ADAPTIVE_SWITCH:
        sc = sigma_with_zero_point(1536, zp, profile)
        for k in ADAPTIVE_SWITCH_KSIZES:
            out.append((f"blocks zp{zp}", blocks(), k, sc))
        for k in ADAPTIVE_BATCH_KSIZES:
            for f, frame in enumerate(blocks_batch()[1:], 1):
                out.append((f"blocks zp{zp} batch frame {f}", frame, k, sc))
    for neg in (False, True):
        for k in (15, 31):
            out.append((f"lone_pixel neg={neg}", lone_pixel(neg), k, 1e4))
            out.append((f"gray lone_pixel neg={neg}", gray(lone_pixel(neg)), k, 1e4))
    out.append(("two_level_noisy", two_level_noisy(), 9, 1000.0))
    out.append(("gray two_level_noisy", gray(two_level_noisy()), 9, 1000.0))
    for v in (0, 1, 254, 255):
        for k in (3, 31, 63):
            out.append((f"flat {v}", flat(v), k, 30.0))
    return out
