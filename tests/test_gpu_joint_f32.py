"""GPU parity of the joint bilateral filter on an f32 one-channel source under an 8-bit guide
(csrc/vip_joint_f32.hip; include/vip.h vip_joint_bilateral_run_f32).

Bar: every output equals tests/f32_oracle.py bit for bit (compared as uint32), in both numerics
profiles, with a gray and with a 3-channel guide, and under both kernel selections: the
radius-specialised vip::joint_f32_kernel (radius 1..15) and the runtime-radius
vip::joint_f32_rt_kernel (radius 0 and 16..23, or every radius under VIP_PATH_RUNTIME).
Frames of more tiles than the device has CUs (joint_f32_kernel's later rounds): tests/test_gpu_c1_rounds.py.
"""
import functools

import numpy as np
import pytest

import f32_oracle
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _BilateralImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
PATHS = [vip.VIP_PATH_AUTO, vip.VIP_PATH_RUNTIME]
FORMS = ["gray", "rgb"]
SENTINEL = 0xA5A5A5A5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mismatch(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    first = [(tuple(i), float(a[tuple(i)]), float(b[tuple(i)])) for i in d[:4]]
    return f"{len(d)} mismatches, first (index, got, want) {first}"


@pytest.fixture
def path(request):
    vip.set_stencil_path(request.param)
    yield request.param
    vip.set_stencil_path(vip.VIP_PATH_AUTO)


# ---- inputs and their oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _source(w, h, stat):
    rng = np.random.default_rng(977 * w + 31 * h + len(stat))
    if stat == "depth":
        f = rng.uniform(0.5, 10.0, (h, w))
    elif stat == "signed":
        f = rng.standard_normal((h, w)) * 1000
    elif stat == "integer":
        f = rng.integers(0, 256, (h, w))
    elif stat == "sparse":  # 70 % exact zeros
        f = np.where(rng.random((h, w)) < 0.7, 0.0, rng.uniform(1.0, 2.0, (h, w)))
    else:  # tiny: +-[1e-36, 1e-30], products with the weights go subnormal
        assert stat == "tiny"
        f = rng.choice([-1.0, 1.0], (h, w)) * 10.0 ** rng.uniform(-36, -30, (h, w))
    return np.ascontiguousarray(f, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _guide(form, w, h):
    rng = np.random.default_rng(1000 * w + h + (7 if form == "rgb" else 0))
    return rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _want(form, w, h, k, profile, ss=10.0, sc=30.0, stat="depth"):
    out = f32_oracle.joint_bilateral(_source(w, h, stat), _guide(form, w, h), k, ss, sc, profile)
    out.setflags(write=False)
    return out


def _gch(guide):
    return 1 if guide.ndim == 2 else 3


def _run(dev, f, guide, k, numerics, ss=10.0, sc=30.0):
    h, w = f.shape
    impl = _BilateralImpl(w, h, k, ss, sc, numerics)
    d_dst = dev.empty((h, w), np.float32)
    impl.joint_bilateral_filter_f32(dev.put(f), dev.put(guide), _gch(guide), d_dst)
    return dev.get(d_dst)


def _check(dev, form, w, h, k, numerics, profile, ss=10.0, sc=30.0, stat="depth"):
    got = _run(dev, _source(w, h, stat), _guide(form, w, h), k, numerics, ss, sc)
    want = _want(form, w, h, k, profile, ss, sc, stat)
    assert np.array_equal(_bits(got), _bits(want)), (form, w, h, k, stat, _mismatch(got, want))


# ---- ksize sweep on 131 x 70: crosses the seams of 64- and 128-pixel tiles both ways; 15 | 17
# and 31 | 33 are the two sides of the specialised kernels' wave-count and radius limits ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 5, 15, 17, 31, 33, 47])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_sweep(dev, path, form, k, numerics, profile):
    _check(dev, form, 131, 70, k, numerics, profile)


# radii either side of the 16 | 12-wave switch of the specialised kernel (gray guide: 12 | 13,
# 3-channel guide: 9 | 10); 131 x 70 crosses the 48- and 64-row tile seams
@pytest.mark.parametrize("form,k", [("gray", 25), ("gray", 27), ("rgb", 19), ("rgb", 21)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_wave_count_switch(dev, form, k, numerics, profile):
    _check(dev, form, 131, 70, k, numerics, profile)


@pytest.mark.parametrize("stat", ["depth", "signed", "integer", "sparse", "tiny"])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_source_statistics(dev, path, stat, numerics, profile):
    """tiny: gradual underflow (denormal mode 3) is part of the definition.
    sparse: gray guide only, where every weight is >= 1e-16 at the default sigmas."""
    for form in (["gray"] if stat == "sparse" else FORMS):
        _check(dev, form, 67, 33, 9, numerics, profile, stat=stat)


# ---- sigmas: the default; a LUT that is zero from d = 25; one never small; only d = 0 ----
@pytest.mark.parametrize("ss,sc", [(10.0, 30.0), (4.0, 3.0 ** 0.5), (1.5, 200.0), (0.3, 0.1)])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_sigmas(dev, path, ss, sc, numerics, profile):
    for form in FORMS:
        _check(dev, form, 67, 33, 9, numerics, profile, ss, sc)


# ---- shapes (tests/test_gpu_gray.py SHAPES): tiny frames, and one pixel either side of both
# kernels' tile widths (128, 64) and one row either side of their tile height (64) ----
SHAPES = [(1, 1), (2, 3), (3, 1), (64, 64), (67, 5), (127, 3), (129, 3), (63, 3), (65, 3), (9, 63), (9, 65)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_shapes(dev, path, w, h, k, numerics, profile):
    for form in FORMS:
        _check(dev, form, w, h, k, numerics, profile)


@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_1_returns_the_source(dev, path, numerics, profile):
    f = _source(67, 33, "signed")
    for form in FORMS:
        got = _run(dev, f, _guide(form, 67, 33), 1, numerics)
        assert np.array_equal(_bits(got), _bits(f)), (form, _mismatch(got, f))


@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_integer_source_rounds_to_the_u8_filter(dev, path, numerics, profile):
    """The tie to the u8 form, on the device: u8(dst + 0.5f) is vip_joint_bilateral_run_c1."""
    w, h, k = 67, 33, 9
    f = _source(w, h, "integer")
    for form in FORMS:
        guide = _guide(form, w, h)
        impl = _BilateralImpl(w, h, k, numerics=numerics)
        d_u8 = dev.empty((h, w))
        impl.joint_bilateral_filter_c1(dev.put(f.astype(np.uint8)), dev.put(guide), _gch(guide), d_u8)
        got = f32_oracle.f2u8(_run(dev, f, guide, k, numerics) + np.float32(0.5))
        assert np.array_equal(got, dev.get(d_u8)), form


# ---- pitch and alignment, through the C ABI ----
def _rows_f32(h, src, sp, guide, gp, gch, dst, dp, out_rows, src_row0, row_lo, row_hi):
    return _lib.lib().vip_joint_bilateral_run_rows_f32(h, src, sp, guide, gp, gch, dst, dp, out_rows, src_row0,
                                                       row_lo, row_hi, None)


def _pitched(dev, a, pitch, offset):
    """Device buffer holding the rows of `a` (2-D bytes) at `offset` + r * pitch; (tensor, address)."""
    rows, rowbytes = a.shape
    host = np.full(offset + rows * pitch + 16, 0x5A, np.uint8)
    for r in range(rows):
        host[offset + r * pitch: offset + r * pitch + rowbytes] = a[r]
    t = dev.put(host)
    return t, t.data_ptr() + offset


# (source offset, source pitch in floats, dst offset, dst pitch in floats): a float-aligned source
# that is not 16-byte aligned, dst pitch (w + 3) * 4 with a 16-byte-aligned base and without;
# then every base and pitch a multiple of 16 (float4 loads and stores, a dword tail in the last
# tile column)
@pytest.mark.parametrize("src_off,src_pf,dst_off,dst_pf", [(4, 132, 0, 134), (4, 132, 4, 134), (0, 132, 0, 136)])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment(dev, path, k, src_off, src_pf, dst_off, dst_pf, numerics, profile):
    w, h = 131, 70
    f = _source(w, h, "depth")
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    t_src, p_src = _pitched(dev, f.view(np.uint8).reshape(h, 4 * w), 4 * src_pf, src_off)
    t_gg, p_gg = _pitched(dev, _guide("gray", w, h), w + 1, 1)                        # base + 1, pitch w + 1
    t_g3, p_g3 = _pitched(dev, _guide("rgb", w, h).reshape(h, 3 * w), 3 * w + 1, 1)  # base + 1, pitch 3w + 1
    assert t_src.data_ptr() % 16 == 0
    for form, pg, gp, gch in (("gray", p_gg, w + 1, 1), ("rgb", p_g3, 3 * w + 1, 3)):
        words = dst_off // 4 + h * dst_pf + 4
        d_dst = dev.put(np.full(words, SENTINEL, np.uint32).view(np.int32))
        assert d_dst.data_ptr() % 16 == 0
        rc = _rows_f32(impl._h, p_src, 4 * src_pf, pg, gp, gch, d_dst.data_ptr() + dst_off, 4 * dst_pf, h, 0, 0, h)
        assert rc == 0, (form, rc)
        raw = dev.get(d_dst).view(np.uint32)
        body = raw[dst_off // 4: dst_off // 4 + h * dst_pf].reshape(h, dst_pf)
        want = _want(form, w, h, k, profile)
        assert np.array_equal(body[:, :w], _bits(want)), (form, _mismatch(body[:, :w].view(np.float32), want))
        assert (body[:, w:] == SENTINEL).all(), form  # the row padding is the caller's
        assert (raw[:dst_off // 4] == SENTINEL).all() and (raw[dst_off // 4 + h * dst_pf:] == SENTINEL).all(), form
    del t_src, t_gg, t_g3


# ---- row bands (131 x 70, ksize 15) ----
def _sentinel_rows(dev, rows, w):
    return dev.put(np.full((rows, w), SENTINEL, np.uint32).view(np.float32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_bands_concatenate_to_the_frame(dev, path, form, numerics, profile):
    w, h, k = 131, 70, 15
    guide = _guide(form, w, h)
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    d_src, d_guide = dev.put(_source(w, h, "depth")), dev.put(guide)
    parts = []
    for r0, r1 in ((0, 23), (23, 24), (24, 70)):
        d_dst = _sentinel_rows(dev, r1 - r0 + 2, w)
        impl.run_rows_f32(d_src, d_guide, _gch(guide), d_dst, r1 - r0, r0, 0, h)
        out = dev.get(d_dst)
        assert (_bits(out[r1 - r0:]) == SENTINEL).all()  # rows past out_rows are untouched
        parts.append(out[:r1 - r0])
    got = np.concatenate(parts)
    want = _want(form, w, h, k, profile)
    assert np.array_equal(_bits(got), _bits(want)), _mismatch(got, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_band_clamps_to_its_row_range(dev, path, form, numerics, profile):
    """row_lo = 10, row_hi = 50: the band is the filter of rows 10..49 alone."""
    w, h, k = 131, 70, 15
    f, guide = _source(w, h, "depth"), _guide(form, w, h)
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    d_dst = _sentinel_rows(dev, 42, w)
    impl.run_rows_f32(dev.put(f), dev.put(guide), _gch(guide), d_dst, 40, 10, 10, 50)
    out = dev.get(d_dst)
    want = f32_oracle.joint_bilateral(f[10:50], guide[10:50], k, profile=profile)
    assert np.array_equal(_bits(out[:40]), _bits(want)), _mismatch(out[:40], want)
    assert (_bits(out[40:]) == SENTINEL).all()


# ---- argument errors: the C ABI's codes, and VipError / ValueError in Python ----
def test_argument_errors(dev):
    w, h = 16, 8
    impl = _BilateralImpl(w, h, 5)
    big = _BilateralImpl(w, h, 49)  # above the joint filter's largest ksize (47)
    d_src, d_dst = dev.put(np.zeros((h + 1, w), np.float32)), dev.empty((h + 1, w), np.float32)
    d_g1, d_g3 = dev.put(np.zeros((h, w), np.uint8)), dev.put(np.zeros((h, w, 3), np.uint8))
    s, d, g1, g3 = d_src.data_ptr(), d_dst.data_ptr(), d_g1.data_ptr(), d_g3.data_ptr()
    p = 4 * w
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING
    run = L.vip_joint_bilateral_run_f32
    assert run(impl._h, s, p, g1, w, 1, d, p, None) == 0
    assert run(impl._h, s, p, g3, 3 * w, 3, d, p, None) == 0
    assert run(None, s, p, g1, w, 1, d, p, None) == INV
    assert run(impl._h, None, p, g1, w, 1, d, p, None) == INV
    assert run(impl._h, s, p, g1, w, 1, None, p, None) == INV
    assert run(impl._h, s, p, None, w, 1, d, p, None) == INV       # a null guide: there is no plain f32 form
    for off in (1, 2, 3):                                            # bases and pitches must be multiples of 4
        assert run(impl._h, s + off, p, g1, w, 1, d, p, None) == INV
        assert run(impl._h, s, p, g1, w, 1, d + off, p, None) == INV
        assert run(impl._h, s, p + off, g1, w, 1, d, p, None) == INV
        assert run(impl._h, s, p, g1, w, 1, d, p + off, None) == INV
    assert run(impl._h, s + 4, p, g1, w, 1, d + 4, p, None) == 0   # any multiple of 4 works
    for gch in (0, 2, 4, -1):
        assert run(impl._h, s, p, g1, w, gch, d, p, None) == INV
    assert _rows_f32(None, s, p, g1, w, 1, d, p, h, 0, 0, h) == INV
    for band in ((h, 0, 4, 4), (h, 0, -1, h), (h, 0, 0, h + 1), (-1, 0, 0, h)):  # out_rows, src_row0, lo, hi
        assert _rows_f32(impl._h, s, p, g1, w, 1, d, p, *band) == INV, band
    assert run(big._h, s, p, g1, w, 1, d, p, None) == KS
    assert run(big._h, s, p, g3, 3 * w, 3, d, p, None) == KS
    assert run(impl._h, s, p, g1, w, 1, s, p, None) == AL
    assert run(impl._h, s, p, g1, w, 1, g1, p, None) == AL
    dev.torch_.cuda.synchronize()

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    f = vip.CudaBilateralFilter(w, h, 5)
    assert code(f.joint_bilateral_filter_f32, d_src, d_g1, 1, d_src) == AL
    assert code(f.joint_bilateral_filter_f32, d_src, d_g1, 2, d_dst) == INV
    assert code(impl.run_rows_f32, d_src, d_g1, 1, d_dst, h, 0, 4, 4) == INV
    assert code(big.joint_bilateral_filter_f32, d_src, d_g3, 3, d_dst) == KS
    with pytest.raises(ValueError):  # a 3-channel guide needs width * height * 3 bytes
        f.joint_bilateral_filter_f32(d_src, d_g1, 3, d_dst)
    with pytest.raises(ValueError):  # the source is float32, width * height * 4 bytes
        f.joint_bilateral_filter_f32(d_g3, d_g1, 1, d_dst)
    with pytest.raises(ValueError):
        f.joint_bilateral_filter_f32(d_src, d_g1, 1, dev.empty((h, w // 2), np.float32))


# ---- launch log and kernel timing see the f32 kernels ----
@pytest.mark.parametrize("k", [9, 33])
def test_launch_log_and_timing(dev, k):
    impl = _BilateralImpl(67, 33, k)
    d_src, d_guide = dev.put(_source(67, 33, "depth")), dev.put(_guide("rgb", 67, 33))
    d_dst = dev.empty((33, 67), np.float32)
    launched_kernels()
    impl.joint_bilateral_filter_f32(d_src, d_guide, 3, d_dst)
    names = launched_kernels()
    assert len(names) == 1 and "joint_f32" in names[0], names
    with kernel_timing(1) as kt:
        impl.joint_bilateral_filter_f32(d_src, d_guide, 3, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "joint_f32" in rec[0][0] and rec[0][1] > 0, rec
