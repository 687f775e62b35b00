"""CPU tests of tests/bilateral_f32_oracle.py, the oracle of the self-guided f32 bilateral filter
(include/vip.h vip_bilateral_f32_run)."""
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest

import bilateral_f32_oracle as bo
import gray_oracle
from f32_oracle import f2u8
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
def _transcription(f, ksize, sigma_space, sigma_color, value_range, profile):
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
            c, s, sumk = f[y, x], F(0), F(0)
            for ky in range(-r, r + 1):
                for kx in range(-r, r + 1):
                    n = f[min(max(y + ky, 0), h - 1), min(max(x + kx, 0), w - 1)]
                    d = F(abs(F(n - c)))
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
    """13 x 9, signed values whose scaled differences land inside the bins, on their edges (the
    quarter steps: value_range 8 has bins of 1/128) and past the table's end (the two outliers)."""
    rng = np.random.default_rng(11)
    f = (rng.standard_normal((9, 13)) * 1.5).astype(np.float32)
    f[2, 3:8] = np.float32(0.25) * rng.integers(-8, 9, 5).astype(np.float32)
    f[5, 6], f[7, 1] = np.float32(40.0), np.float32(-0.0)
    with np.errstate(all="ignore"):
        want = _transcription(f, k, 1.5, 0.75, 8.0, profile)
    got = bo.bilateral(f, k, 1.5, 0.75, 8.0, profile)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5].tolist()
    if k == 1:  # ksize 1 returns f, with -0 -> +0
        assert np.array_equal(_bits(got), _bits(np.where(f == 0, np.float32(0.0), f)))


def test_tables():
    for profile in PROFILES:
        scale, L, D = bo.tables(30.0, 1024.0, profile)
        assert scale == 1 and L.shape == (bo.BINS + 2,) and D.shape == (bo.BINS + 1,)
        assert L[0] == 1 and L[bo.BINS + 1] == L[bo.BINS] and D[bo.BINS] == 0
        # bin width exactly 1: the table is the colour LUT, bit for bit
        assert np.array_equal(_bits(L[:768]), _bits(o.color_lut(768, 30.0, profile)))


# ---- 2. the tie to the u8 form ----
@pytest.mark.parametrize("k", [5, 15, 31])
@pytest.mark.parametrize("profile", PROFILES)
def test_integer_sources_round_to_the_u8_filter(profile, k):
    rng = np.random.default_rng(100 * 67 + 33)
    g = rng.integers(0, 256, (33, 67), dtype=np.uint8)
    out = bo.bilateral(g.astype(np.float32), k, 10.0, 30.0, 1024.0, profile)
    got = f2u8(out + np.float32(0.5))
    want = gray_oracle.bilateral(g, k, 10.0, 30.0, profile)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


# ---- 3. the row-band form ----
@pytest.mark.parametrize("profile", PROFILES)
def test_row_bands(profile):
    rng = np.random.default_rng(5)
    f = rng.uniform(0.5, 10.0, (40, 21)).astype(np.float32)
    args = (7, 2.0, 1.0, 10.0, profile)
    whole = bo.bilateral(f, *args)
    parts = [bo.bilateral_rows(f, b - a, a, 0, 40, *args) for a, b in ((0, 13), (13, 14), (14, 40))]
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole))
    # neighbour rows clamped to [8, 30): the filter of those rows alone
    band = bo.bilateral_rows(f, 18, 10, 8, 30, *args)
    alone = bo.bilateral(f[8:30], *args)
    assert np.array_equal(_bits(band), _bits(alone[2:20]))
    assert not np.array_equal(_bits(band), _bits(whole[10:28]))


# ---- 4. the definition against a float64 filter with exact exp weights ----
def f64_frame():
    """141 x 37, uniform in [0, 3.6): every difference lies inside value_range 4."""
    return np.random.default_rng(20261021).uniform(0.0, 3.6, (37, 141)).astype(np.float32)


def _f64_filter(f, ksize, sigma_space, sigma_color):
    h, w = f.shape
    r = ksize // 2
    f64 = f.astype(np.float64)
    fp = np.pad(f64, r, mode="edge")
    s, sumk = np.zeros((h, w)), np.zeros((h, w))
    for ky in range(ksize):
        for kx in range(ksize):
            r2 = (ky - r) ** 2 + (kx - r) ** 2
            if r2 > r * r:
                continue
            n = fp[ky:ky + h, kx:kx + w]
            wgt = np.exp(-r2 / (2.0 * sigma_space ** 2)) * np.exp(-((n - f64) ** 2) / (2.0 * sigma_color ** 2))
            s += n * wgt
            sumk += wgt
    return s / sumk


# measured on f64_frame(): the largest |oracle - float64 filter| (DESIGN.md section 4 records it)
F64_MEASURED = 8.3e-6


@pytest.mark.parametrize("profile", PROFILES)
def test_definition_is_close_to_the_float64_filter(profile):
    """Checks the definition (1024 bins, linear interpolation, binary32 sums), not the kernel:
    sigma_color 0.25, value_range 4, ksize 9. The bound is 4 x the measured value, which leaves
    room for another draw of the frame."""
    f = f64_frame()
    assert 3.5 < float(f.max() - f.min()) < 3.6
    got = bo.bilateral(f, 9, 10.0, 0.25, 4.0, profile)
    err = float(np.abs(got.astype(np.float64) - _f64_filter(f, 9, 10.0, 0.25)).max())
    print(f"profile {profile}: max |oracle - float64 filter| = {err:.3e}")
    assert err <= 4 * F64_MEASURED, err


def test_profiles_differ():
    """An oracle that dropped the FMA would make the CUDA profile the CPP one: not one bit would differ."""
    f = f64_frame()
    a, b = (bo.bilateral(f, 5, 10.0, 0.25, 4.0, p) for p in PROFILES)
    assert (_bits(a) != _bits(b)).any()
