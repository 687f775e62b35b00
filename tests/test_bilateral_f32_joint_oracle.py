"""CPU tests of tests/bilateral_f32_joint_oracle.py, the oracle of the f32 joint bilateral filter under
an f32 guide (include/vip.h vip_bilateral_f32_run_joint): a transcription of the definition, the
three identities that pin it to oracles already pinned to the reference, the row-band form and its
distance from a float64 filter with exact exp weights."""
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest

import bilateral_f32_joint_oracle as jo
import bilateral_f32_oracle as bo
import f32_oracle
from oracle import oracle as o

PROFILES = [o.CUDA, o.CPP]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _libm():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    libm.exp.restype, libm.exp.argtypes = ctypes.c_double, [ctypes.c_double]
    return libm


# ---- 1. the oracle against a per-pixel, per-tap transcription of the definition ----
def _transcription(f, g, ksize, sigma_space, sigma_color, value_range, profile):
    """include/vip.h, line by line, on Python scalars: every binary32 operation is one np.float32
    operation, fmaf and expf are libm's. No tap is skipped."""
    F = np.float32
    m = _libm()
    N = bo.BINS
    h, w = f.shape
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    scale = F(N) / F(value_range)
    two_s2 = F(2) * F(sigma_color) * F(sigma_color)
    cf, cd = F(-1.0) / two_s2, -1.0 / float(two_s2)
    L = []
    for i in range(N + 1):
        v = F(i) / scale
        L.append(F(m.exp(float(v) * float(v) * cd)) if profile == o.CPP else F(m.expf(float(F(v * v) * cf))))
    L.append(L[N])
    D = [F(L[i + 1] - L[i]) for i in range(N + 1)]
    out = np.empty((h, w), np.float32)
    for y in range(h):
        for x in range(w):
            c, s, sumk = g[y, x], F(0), F(0)
            for ky in range(-r, r + 1):
                for kx in range(-r, r + 1):
                    yy, xx = min(max(y + ky, 0), h - 1), min(max(x + kx, 0), w - 1)
                    n, gn = f[yy, xx], g[yy, xx]
                    d = F(abs(F(gn - c)))
                    t = min(F(d * scale), F(N))
                    i = int(t)
                    a = F(t - F(i))
                    if profile == o.CUDA:
                        wc = F(m.fmaf(float(a), float(D[i]), float(L[i])))
                    else:
                        wc = F(L[i] + F(a * D[i]))
                    wgt = F(ws[ky + r, kx + r] * wc)
                    if profile == o.CUDA:
                        s = F(m.fmaf(float(n), float(wgt), float(s)))
                    else:
                        s = F(s + F(n * wgt))
                    sumk = F(sumk + wgt)
            out[y, x] = F(s / sumk)
    return out


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("profile", PROFILES)
def test_oracle_matches_the_transcription(profile, k):
    """9 x 7: a guide whose scaled differences land inside the bins, on their edges (the quarter
    steps: value_range 8 has bins of 1/128) and past the table's end (the outlier), under a signed
    source with a -0."""
    rng = np.random.default_rng(12)
    g = (rng.standard_normal((7, 9)) * 1.5).astype(np.float32)
    g[2, 2:7] = np.float32(0.25) * rng.integers(-8, 9, 5).astype(np.float32)
    g[5, 6] = np.float32(40.0)
    f = (rng.standard_normal((7, 9)) * 30).astype(np.float32)
    f[3, 1] = np.float32(-0.0)
    with np.errstate(all="ignore"):
        want = _transcription(f, g, k, 1.5, 0.75, 8.0, profile)
    got = jo.joint(f, g, k, 1.5, 0.75, 8.0, profile)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5].tolist()


# ---- 2. the identities, on a 141 x 37 frame ----
W, H = 141, 37


@functools.lru_cache(maxsize=None)
def _frames():
    rng = np.random.default_rng(20261022)
    f = rng.uniform(0.0, 3.6, (H, W)).astype(np.float32)
    noise = (rng.standard_normal((H, W)) * 20).astype(np.float32)
    g8 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for a in (f, noise, g8):
        a.setflags(write=False)
    return f, noise, g8


@pytest.mark.parametrize("k", [1, 5, 9, 15])
@pytest.mark.parametrize("profile", PROFILES)
def test_i1_guide_equal_to_source_is_the_self_guided_filter(profile, k):
    f = _frames()[0]
    got = jo.joint(f, f, k, 10.0, 0.25, 4.0, profile)
    want = bo.bilateral(f, k, 10.0, 0.25, 4.0, profile)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("k", [1, 5, 9, 15])
@pytest.mark.parametrize("profile", PROFILES)
def test_i2_integer_guide_is_the_u8_guided_filter(profile, k):
    """value_range 1024: scale is 1, t = |g_n - g_c| is an integer, a = 0 and wc = L[i], the colour
    LUT's entry i: f32_oracle.joint_bilateral under the u8 guide, bit for bit, at the same sigmas."""
    _, noise, g8 = _frames()
    for sc in (0.25, 30.0):
        got = jo.joint(noise, g8.astype(np.float32), k, 10.0, sc, 1024.0, profile)
        want = f32_oracle.joint_bilateral(noise, g8, k, 10.0, sc, profile)
        assert np.array_equal(_bits(got), _bits(want)), (k, sc)


def _spatial_only(f, ksize, sigma_space, profile):
    """The definition with every wc = 1 (L[0]): w = ws * 1 = ws."""
    h, w = f.shape
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    fp = np.pad(f, r, mode="edge")
    s, sumk = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for ky in range(ksize):
        for kx in range(ksize):
            n = fp[ky:ky + h, kx:kx + w]
            wgt = np.full((h, w), ws[ky, kx], np.float32)
            s = f32_oracle.fmaf(n, wgt, s) if profile == o.CUDA else (s + (n * wgt).astype(np.float32)).astype(np.float32)
            sumk = (sumk + wgt).astype(np.float32)
    return (s / sumk).astype(np.float32)


@pytest.mark.parametrize("k", [1, 5, 9])
@pytest.mark.parametrize("profile", PROFILES)
def test_i3_constant_guide_and_ksize_1(profile, k):
    _, noise, g8 = _frames()
    const = np.full((H, W), np.float32(2.5))
    got = jo.joint(noise, const, k, 3.0, 0.25, 4.0, profile)
    assert np.array_equal(_bits(got), _bits(_spatial_only(noise, k, 3.0, profile)))
    if k == 1:  # ksize 1 returns f with -0 as +0, whatever the guide
        f = noise.copy()
        f[3, 4], f[5, 6] = np.float32(-0.0), np.float32(0.0)
        for guide in (const, g8.astype(np.float32), _frames()[0]):
            got = jo.joint(f, guide, 1, 3.0, 0.25, 4.0, profile)
            assert np.array_equal(_bits(got), _bits(np.where(f == 0, np.float32(0.0), f)))


# ---- 3. the row-band form ----
@pytest.mark.parametrize("profile", PROFILES)
def test_row_bands(profile):
    rng = np.random.default_rng(5)
    f = (rng.standard_normal((40, 21)) * 20).astype(np.float32)
    g = rng.uniform(0.5, 10.0, (40, 21)).astype(np.float32)
    args = (7, 2.0, 1.0, 10.0, profile)
    whole = jo.joint(f, g, *args)
    parts = [jo.joint_rows(f, g, b - a, a, 0, 40, *args) for a, b in ((0, 13), (13, 14), (14, 40))]
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole))
    # neighbour rows of both images clamped to [8, 30): the filter of those rows alone
    band = jo.joint_rows(f, g, 18, 10, 8, 30, *args)
    alone = jo.joint(f[8:30], g[8:30], *args)
    assert np.array_equal(_bits(band), _bits(alone[2:20]))
    assert not np.array_equal(_bits(band), _bits(whole[10:28]))


# ---- 4. the definition against a float64 filter with exact exp weights ----
def _f64_filter(f, g, ksize, sigma_space, sigma_color):
    h, w = f.shape
    r = ksize // 2
    f64, g64 = f.astype(np.float64), g.astype(np.float64)
    fp, gp = np.pad(f64, r, mode="edge"), np.pad(g64, r, mode="edge")
    s, sumk = np.zeros((h, w)), np.zeros((h, w))
    for ky in range(ksize):
        for kx in range(ksize):
            r2 = (ky - r) ** 2 + (kx - r) ** 2
            if r2 > r * r:
                continue
            n, gn = fp[ky:ky + h, kx:kx + w], gp[ky:ky + h, kx:kx + w]
            wgt = np.exp(-r2 / (2.0 * sigma_space ** 2)) * np.exp(-((gn - g64) ** 2) / (2.0 * sigma_color ** 2))
            s += n * wgt
            sumk += wgt
    return s / sumk


# measured on the frame below: the largest |oracle - float64 filter| over both profiles (DESIGN.md
# section 4 records it): 3.054e-5 in the CUDA profile, 3.060e-5 in the CPP profile
F64_MEASURED = 3.1e-5


@pytest.mark.parametrize("profile", PROFILES)
def test_definition_is_close_to_the_float64_filter(profile):
    """Checks the definition (1024 bins, linear interpolation, binary32 sums), not the kernel: the
    guide is test_bilateral_f32_oracle.f64_frame() (141 x 37, spread 3.6), the source independent
    unit-variance noise, sigma_color 0.25, value_range 4, ksize 9. The bound is 4 x the measured
    value, the one-channel sibling's margin, which leaves room for another draw of the frames."""
    g = np.random.default_rng(20261021).uniform(0.0, 3.6, (37, 141)).astype(np.float32)  # f64_frame() there
    assert 3.5 < float(g.max() - g.min()) < 3.6
    f = np.random.default_rng(20261023).standard_normal(g.shape).astype(np.float32)
    got = jo.joint(f, g, 9, 10.0, 0.25, 4.0, profile)
    err = float(np.abs(got.astype(np.float64) - _f64_filter(f, g, 9, 10.0, 0.25)).max())
    print(f"profile {profile}: max |oracle - float64 filter| = {err:.3e}")
    assert err <= 4 * F64_MEASURED, err


def test_profiles_differ():
    """An oracle that dropped the FMA would make the CUDA profile the CPP one: not one bit would differ."""
    f, noise, _ = _frames()
    a, b = (jo.joint(noise, f, 5, 10.0, 0.25, 4.0, p) for p in PROFILES)
    assert (_bits(a) != _bits(b)).any()
