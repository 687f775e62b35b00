"""CPU tests of tests/bilateral_f32c_oracle.py, the oracle of the self-guided f32 bilateral filter on
2 and 3 interleaved channels (include/vip.h vip_bilateral_f32_run_c): the helper against a
transcription of the definition, and the definition's three identities."""
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest

import bilateral_f32_oracle as bo
import bilateral_f32c_oracle as bc
from f32_oracle import f2u8
from oracle import oracle as o

PROFILES = [o.CUDA, o.CPP]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _libm():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return libm


# ---- the oracle against a per-pixel, per-tap transcription of the definition ----
def _transcription(f, ksize, sigma_space, sigma_color, value_range, profile):
    """include/vip.h, line by line, on Python scalars: every binary32 operation is one np.float32
    operation, fmaf is libm's. No tap is skipped. The tables are the handle's, as the definition
    takes them (bilateral_f32_oracle.tables; tests/test_bilateral_f32_oracle.py transcribes those)."""
    F = np.float32
    m = _libm()
    N = bo.BINS
    h, w, ch = f.shape
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    scale, L, D = bo.tables(sigma_color, value_range, profile)
    out = np.empty((h, w, ch), np.float32)
    for y in range(h):
        for x in range(w):
            c, s, sumk = f[y, x], [F(0)] * ch, F(0)
            for ky in range(-r, r + 1):
                for kx in range(-r, r + 1):
                    n = f[min(max(y + ky, 0), h - 1), min(max(x + kx, 0), w - 1)]
                    d = F(F(abs(F(n[0] - c[0]))) + F(abs(F(n[1] - c[1]))))
                    if ch == 3:
                        d = F(d + F(abs(F(n[2] - c[2]))))
                    t = min(F(d * scale), F(N))
                    i = int(t)
                    a = F(t - F(i))
                    if profile == o.CUDA:
                        wc = F(m.fmaf(float(a), float(D[i]), float(L[i])))
                    else:
                        wc = F(L[i] + F(a * D[i]))
                    wgt = F(ws[ky + r, kx + r] * wc)
                    for k in range(ch):
                        if profile == o.CUDA:
                            s[k] = F(m.fmaf(float(n[k]), float(wgt), float(s[k])))
                        else:
                            s[k] = F(s[k] + F(n[k] * wgt))
                    sumk = F(sumk + wgt)
            for k in range(ch):
                out[y, x, k] = F(s[k] / sumk)
    return out


def _small_frame(ch):
    """9 x 7: signed values whose scaled distances land inside the bins, on their edges (the quarter
    steps: value_range 8 has bins of 1/128) and past the table's end (the outlier), and a -0."""
    rng = np.random.default_rng(11 + ch)
    f = (rng.standard_normal((7, 9, ch)) * 1.5).astype(np.float32)
    f[2, 3:8] = np.float32(0.25) * rng.integers(-8, 9, (5, ch)).astype(np.float32)
    f[5, 6, ch - 1], f[4, 1, 0], f[4, 1, 1] = np.float32(40.0), np.float32(-0.0), np.float32(-0.0)
    return f


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("profile", PROFILES)
def test_oracle_matches_the_transcription(profile, ch, k):
    f = _small_frame(ch)
    with np.errstate(all="ignore"):
        want = _transcription(f, k, 1.5, 0.75, 8.0, profile)
    got = bc.bilateral(f, k, 1.5, 0.75, 8.0, profile)
    assert got.shape == f.shape and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5].tolist()


# ---- identity 1: the tie to the 8-bit colour filter ----
@pytest.mark.parametrize("k", [9, 15])
@pytest.mark.parametrize("profile", PROFILES)
def test_integer_sources_round_to_the_u8_colour_filter(profile, k):
    """value_range 1024, f = float32(g) for a u8 3-channel frame: d <= 765 is an integer, a = 0 at
    every tap, and u8(dst_c + 0.5f) is the 8-bit colour filter on g."""
    g = np.random.default_rng(100 * 41 + 29).integers(0, 256, (29, 41, 3), dtype=np.uint8)
    out = bc.bilateral(g.astype(np.float32), k, 10.0, 30.0, 1024.0, profile)
    got = f2u8(out + np.float32(0.5))
    want = o.bilateral(g, k, 10.0, 30.0, profile)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


# ---- identity 2: the tie to the one-channel filter ----
@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("profile", PROFILES)
def test_constant_other_channels_give_the_one_channel_filter(profile, ch):
    """Every channel but channel 0 constant over the frame: their terms of d are exactly +0 and
    channel 0 of the result is the one-channel filter on plane 0, bit for bit."""
    rng = np.random.default_rng(7)
    f = np.empty((21, 33, ch), np.float32)
    f[..., 0] = rng.uniform(0.5, 10.0, (21, 33))
    f[..., 1] = np.float32(-3.25)
    if ch == 3:
        f[..., 2] = np.float32(1e30)
    got = bc.bilateral(f, 7, 2.0, 1.0, 9.5, profile)
    want = bo.bilateral(np.ascontiguousarray(f[..., 0]), 7, 2.0, 1.0, 9.5, profile)
    assert np.array_equal(_bits(got[..., 0]), _bits(want))


# ---- identity 3: ksize 1 ----
@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("profile", PROFILES)
def test_ksize_1_returns_the_source(profile, ch):
    f = _small_frame(ch)
    assert np.signbit(f[f == 0]).any()
    got = bc.bilateral(f, 1, 1.5, 0.75, 8.0, profile)
    assert np.array_equal(_bits(got), _bits(np.where(f == 0, np.float32(0.0), f)))


# ---- the row-band form ----
@pytest.mark.parametrize("profile", PROFILES)
def test_row_bands(profile):
    f = np.random.default_rng(5).uniform(0.5, 10.0, (40, 21, 3)).astype(np.float32)
    args = (7, 2.0, 1.0, 20.0, profile)
    whole = bc.bilateral(f, *args)
    parts = [bc.bilateral_rows(f, b - a, a, 0, 40, *args) for a, b in ((0, 13), (13, 14), (14, 40))]
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole))
    band = bc.bilateral_rows(f, 18, 10, 8, 30, *args)  # neighbour rows clamped to [8, 30): those rows alone
    alone = bc.bilateral(f[8:30], *args)
    assert np.array_equal(_bits(band), _bits(alone[2:20]))
    assert not np.array_equal(_bits(band), _bits(whole[10:28]))


def test_the_weight_couples_the_channels():
    """An oracle that filtered plane by plane would pass identity 2: on a frame whose channels all
    vary, channel 0 is not the one-channel filter on plane 0."""
    f = np.random.default_rng(9).uniform(0.5, 10.0, (15, 17, 3)).astype(np.float32)
    got = bc.bilateral(f, 5, 2.0, 1.0, 9.5, o.CUDA)
    alone = bo.bilateral(np.ascontiguousarray(f[..., 0]), 5, 2.0, 1.0, 9.5, o.CUDA)
    assert (_bits(got[..., 0]) != _bits(alone)).any()
