"""CPU tests of tests/conf_oracle.py, the oracle of the confidence-weighted f32 joint bilateral
filter (include/vip.h vip_joint_bilateral_run_conf_f32), of the inputs the GPU tests reuse, and of
the new entry point's presence in the built library and the Python binding."""
import ctypes
import functools
import math

import numpy as np
import pytest

import conf_oracle as co
import f32_oracle
from oracle import oracle as o

PROFILES = [o.CUDA, o.CPP]
FORMS = ["gray", "rgb"]
W, H, K = 67, 33, 9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _guide(form, w, h):
    rng = np.random.default_rng(1000 * w + h + (7 if form == "rgb" else 0))
    return rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _field(w, h, signed=False):
    rng = np.random.default_rng(977 * w + 31 * h + signed)
    f = rng.standard_normal((h, w)) * 1000 if signed else rng.uniform(0.5, 10.0, (h, w))
    return np.ascontiguousarray(f, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _holes_run(form, profile):
    return co.joint_bilateral_conf(_field(W, H), co.confidence("holes", W, H), _guide(form, W, H), K, profile=profile,
                                   hole_value=-1.0)


# ---- the vectorised oracle against a per-pixel scalar transcription of the definition ----
def _fma_scalar(a, b, c):
    """fmaf through float64: exact product, TwoSum, round to odd (as f32_oracle.fmaf, one element)."""
    return float(f32_oracle.fmaf(np.float32(a), np.float32(b), np.float32(c)))


def _scalar(f, c, guide, ksize, ss, sc, profile, hole_value):
    h, w = f.shape
    r = ksize // 2
    ws = o.space_lut(ksize, ss, profile)
    wc = o.color_lut(768, sc, profile)
    g = guide.reshape(h, w, -1).astype(np.int64)
    F = np.float32
    dst = np.empty((h, w), np.float32)
    wgt = np.empty((h, w), np.float32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                s, sumk = F(0), F(0)
                for ky in range(-r, r + 1):
                    for kx in range(-r, r + 1):
                        ny, nx = min(max(y + ky, 0), h - 1), min(max(x + kx, 0), w - 1)
                        d = int(np.abs(g[ny, nx] - g[y, x]).sum())
                        wt = F(F(ws[ky + r, kx + r]) * F(wc[d]))
                        cn = F(c[ny, nx])
                        pn = F(0) if cn == 0 else F(F(f[ny, nx]) * cn)
                        if profile == o.CUDA:
                            s, sumk = F(_fma_scalar(pn, wt, s)), F(_fma_scalar(cn, wt, sumk))
                        else:
                            s, sumk = F(s + F(pn * wt)), F(sumk + F(cn * wt))
                dst[y, x] = F(hole_value) if sumk == 0 else F(s / sumk)
                wgt[y, x] = sumk
    return dst, wgt


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("profile", PROFILES)
def test_vectorised_oracle_is_the_scalar_definition(profile, form):
    w, h, k = 11, 7, 5
    rng = np.random.default_rng(5)
    f = (rng.standard_normal((h, w)) * 100).astype(np.float32)
    c = np.where(rng.random((h, w)) < 0.3, 0.0, rng.uniform(0, 1, (h, w))).astype(np.float32)
    c[0:4, 0:5] = 0   # a block larger than the window's reach from its corner: sumk == 0 there
    f[c == 0] = np.nan
    guide = _guide(form, w, h)
    got = co.joint_bilateral_conf(f, c, guide, k, 2.0, 30.0, profile, -7.0)
    want = _scalar(f, c, guide, k, 2.0, 30.0, profile, -7.0)
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    assert np.array_equal(_bits(got[1]), _bits(want[1]))
    assert (got[1] == 0).any() and (got[0][got[1] == 0] == -7.0).all()


# ---- the ties of the definition ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("kind", ["ones", "quarter"])
def test_constant_confidence_is_the_f32_filter(profile, form, kind):
    """c == 1: p = f and fmaf(1, w, sumk) = sumk + w. c == 2^-2: every product and sum scales by an
    exact power of two (no underflow on this input), and the quotient is unchanged."""
    f, guide = _field(W, H, True), _guide(form, W, H)
    dst, sumk = co.joint_bilateral_conf(f, co.confidence(kind, W, H), guide, K, profile=profile)
    want = f32_oracle.joint_bilateral(f, guide, K, profile=profile)
    assert np.array_equal(_bits(dst), _bits(want))
    assert (sumk >= (1.0 if kind == "ones" else 0.25)).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("profile", PROFILES)
def test_source_under_a_hole_is_not_read(profile, form):
    c = co.confidence("holes", W, H)
    guide = _guide(form, W, H)
    base = _holes_run(form, profile)
    for junk in (np.nan, np.inf, -np.inf, 1e38):
        f = np.where(c == 0, np.float32(junk), _field(W, H)).astype(np.float32)
        got = co.joint_bilateral_conf(f, c, guide, K, profile=profile, hole_value=-1.0)
        assert np.array_equal(_bits(got[0]), _bits(base[0])), junk
        assert np.array_equal(_bits(got[1]), _bits(base[1])), junk


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("profile", PROFILES)
def test_hole_value_marks_exactly_the_empty_windows(profile, form):
    dst, sumk = _holes_run(form, profile)   # hole_value -1; the field is >= 0.5, so -1 is no filter output
    assert np.array_equal(dst == -1.0, sumk == 0)
    nan_dst, _ = co.joint_bilateral_conf(_field(W, H), co.confidence("holes", W, H), _guide(form, W, H), K,
                                         profile=profile, hole_value=math.nan)
    assert np.array_equal(np.isnan(nan_dst), sumk == 0)
    # c > 0 everywhere: the centre tap alone gives sumk >= c > 0, and no hole_value appears
    c = np.maximum(co.confidence("real", W, H), np.float32(1e-3))
    dst, sumk = co.joint_bilateral_conf(_field(W, H), c, _guide(form, W, H), K, profile=profile, hole_value=-1.0)
    assert (sumk > 0).all() and not (dst == -1.0).any()


# ---- the condition on the inputs the GPU tests reuse: both hole paths are exercised ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("profile", PROFILES)
def test_holes_input_exercises_both_hole_paths(profile, form):
    c = co.confidence("holes", W, H)
    assert set(np.unique(c)) == {0.0, 1.0}
    _, sumk = _holes_run(form, profile)
    empty = (sumk == 0).mean()
    filled = ((c == 0) & (sumk > 0)).mean()
    print(f"{form} profile {profile}: sumk == 0 at {100 * empty:.1f} %, filled holes at {100 * filled:.1f} %")
    assert 0.01 <= empty <= 0.25, empty
    assert filled >= 0.20, filled
    assert (sumk[c > 0] > 0).all()
    # the negative-zero form of the same mask is the same input
    neg = co.confidence("negzero", W, H)
    assert np.array_equal(neg == 0, c == 0) and np.signbit(neg[neg == 0]).all()
    got = co.joint_bilateral_conf(_field(W, H), neg, _guide(form, W, H), K, profile=profile, hole_value=-1.0)
    assert np.array_equal(_bits(got[0]), _bits(_holes_run(form, profile)[0]))
    assert np.array_equal(_bits(got[1]), _bits(sumk))


@pytest.mark.parametrize("form", FORMS)
def test_profiles_differ_on_a_real_confidence(form):
    """Both profiles are genuinely tested: on a signed source under a real-valued confidence the
    fused and the twice-rounded sums differ at a large share of the pixels."""
    f, c, guide = _field(W, H, True), co.confidence("real", W, H), _guide(form, W, H)
    a, _ = co.joint_bilateral_conf(f, c, guide, K, profile=o.CUDA)
    b, _ = co.joint_bilateral_conf(f, c, guide, K, profile=o.CPP)
    share = (_bits(a) != _bits(b)).mean()
    print(f"{form}: the profiles differ at {100 * share:.1f} % of the pixels")
    assert share >= 0.2, share


def test_ksize_1_is_the_normalised_product():
    f, c = _field(W, H, True), co.confidence("real", W, H)
    dst, sumk = co.joint_bilateral_conf(f, c, _guide("gray", W, H), 1, hole_value=-5.0)
    with np.errstate(all="ignore"):
        want = np.where(c == 0, np.float32(-5.0), (co.product(f, c) / np.where(c == 0, np.float32(1), c)))
    assert np.array_equal(_bits(dst), _bits(want.astype(np.float32)))
    assert np.array_equal(_bits(sumk), _bits(c))


# ---- the entry point exists: this fails without the feature, and needs no GPU ----
def test_entry_point_is_exported_and_bound():
    import inspect

    import various_image_processings_amd as vip
    from various_image_processings_amd import _lib, filters
    name = "vip_joint_bilateral_run_conf_f32"
    assert hasattr(ctypes.CDLL(vip.LIB_PATH), name)
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 14
    assert _lib.SIGNATURES[name][1][8] is ctypes.c_float   # hole_value
    assert vip.VIP_FILTER_JOINT_CONF == 5
    assert vip.lib().vip_max_ksize(vip.VIP_FILTER_JOINT_CONF) == 31
    assert vip.max_ksize(vip.VIP_FILTER_JOINT_CONF) == 31
    for cls in (filters._BilateralImpl, vip.CudaBilateralFilter):
        params = list(inspect.signature(cls.joint_bilateral_filter_conf_f32).parameters)
        assert params[1:8] == ["d_src", "d_conf", "d_guide", "guide_channels", "d_dst", "hole_value", "d_weight"]
