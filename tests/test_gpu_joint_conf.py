"""GPU parity of the confidence-weighted joint bilateral filter on an f32 one-channel source under
an 8-bit guide (csrc/vip_joint_conf.hip; include/vip.h vip_joint_bilateral_run_conf_f32).

Bar: dst and the weight output equal tests/conf_oracle.py bit for bit (compared as uint32), in both
numerics profiles, with a gray and with a 3-channel guide, and dst is the same bits with and
without the weight output.
Frames of more tiles than the device has CUs (joint_conf_f32_kernel's later rounds): tests/test_gpu_c1_rounds.py.
"""
import functools
import math

import numpy as np
import pytest

import conf_oracle as co
import f32_oracle
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _BilateralImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
FORMS = ["gray", "rgb"]
SENTINEL = 0xA5A5A5A5
HOLE = -1.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mismatch(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    first = [(tuple(i), float(a[tuple(i)]), float(b[tuple(i)])) for i in d[:4]]
    return f"{len(d)} mismatches, first (index, got, want) {first}"


# ---- inputs and their oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _source(w, h, stat):
    """tests/test_gpu_joint_f32.py's sources of the same names."""
    rng = np.random.default_rng(977 * w + 31 * h + len(stat))
    if stat == "depth":
        f = rng.uniform(0.5, 10.0, (h, w))
    elif stat == "signed":
        f = rng.standard_normal((h, w)) * 1000
    else:  # tiny: +-[1e-36, 1e-30], products with the weights go subnormal
        assert stat == "tiny"
        f = rng.choice([-1.0, 1.0], (h, w)) * 10.0 ** rng.uniform(-36, -30, (h, w))
    return np.ascontiguousarray(f, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _guide(form, w, h):
    rng = np.random.default_rng(1000 * w + h + (7 if form == "rgb" else 0))
    return rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _conf(kind, w, h):
    return co.confidence(kind, w, h)


@functools.lru_cache(maxsize=None)
def _want(form, w, h, k, profile, kind="holes", stat="depth", ss=10.0, sc=30.0):
    dst, sumk = co.joint_bilateral_conf(_source(w, h, stat), _conf(kind, w, h), _guide(form, w, h), k, ss, sc,
                                        profile, HOLE)
    dst.setflags(write=False)
    sumk.setflags(write=False)
    return dst, sumk


def _gch(guide):
    return 1 if guide.ndim == 2 else 3


def _run(dev, f, c, guide, k, numerics, hole=HOLE, weight=True, ss=10.0, sc=30.0):
    """(dst, weight or None) of one call on dense buffers."""
    h, w = f.shape
    impl = _BilateralImpl(w, h, k, ss, sc, numerics)
    d_dst = dev.empty((h, w), np.float32)
    d_wgt = dev.empty((h, w), np.float32) if weight else None
    impl.joint_bilateral_filter_conf_f32(dev.put(f), dev.put(c), dev.put(guide), _gch(guide), d_dst, hole, d_wgt)
    return dev.get(d_dst), (dev.get(d_wgt) if weight else None)


def _check(dev, form, w, h, k, numerics, profile, kind="holes", stat="depth", ss=10.0, sc=30.0):
    """dst and weight against the oracle, and dst again without the weight output."""
    f, c, guide = _source(w, h, stat), _conf(kind, w, h), _guide(form, w, h)
    want, want_k = _want(form, w, h, k, profile, kind, stat, ss, sc)
    got, got_k = _run(dev, f, c, guide, k, numerics, ss=ss, sc=sc)
    tag = (form, w, h, k, kind, stat)
    assert np.array_equal(_bits(got), _bits(want)), (tag, _mismatch(got, want))
    assert np.array_equal(_bits(got_k), _bits(want_k)), (tag, "weight", _mismatch(got_k, want_k))
    alone, _ = _run(dev, f, c, guide, k, numerics, weight=False, ss=ss, sc=sc)
    assert np.array_equal(_bits(alone), _bits(got)), (tag, "dst without d_weight", _mismatch(alone, got))


def _kernel_name(k, gch, numerics):
    fma = "true" if numerics == vip.VIP_NUMERICS_CUDA else "false"
    return f"joint_conf_f32_k1_kernel<{fma}>" if k == 1 else f"joint_conf_f32_kernel<{k // 2}, {gch}, {fma}>"


# ---- ksize sweep on 131 x 70: crosses the 128-pixel tile seam and the seams of the 64-, 48- and
# 32-row tiles of the 16-, 12- and 8-wave kernels ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 3, 5, 15, 31])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_sweep(dev, form, k, numerics, profile):
    launched_kernels()
    _check(dev, form, 131, 70, k, numerics, profile)
    names = launched_kernels()
    want = _kernel_name(k, 1 if form == "gray" else 3, numerics)
    assert names and all(want in n for n in names), (want, names)  # both launches: the one instantiation


# ksizes either side of every switch of the specialised kernel (csrc/vip_joint_conf.hip conf_waves,
# conf_rgb_copies). Gray guide: 16 | 12 waves at radius 3 | 4, 12 | 8 waves at 9 | 10. 3-channel guide:
# 16 | 12 waves at 2 | 3, 12 | 8 waves at 8 | 9, 16 | 8 LUT copies at 13 | 14.
SWITCHES = [("gray", 7), ("gray", 9), ("gray", 19), ("gray", 21),
            ("rgb", 5), ("rgb", 7), ("rgb", 17), ("rgb", 19), ("rgb", 27), ("rgb", 29)]


@pytest.mark.parametrize("form,k", SWITCHES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_wave_count_switch(dev, form, k, numerics, profile):
    launched_kernels()
    _check(dev, form, 131, 70, k, numerics, profile, kind="real", stat="signed")
    names = launched_kernels()
    want = _kernel_name(k, 1 if form == "gray" else 3, numerics)
    assert names and all(want in n for n in names), (want, names)


# ---- confidence kinds on 67 x 33, ksize 9 ----
@pytest.mark.parametrize("kind", ["ones", "holes", "real", "tiny", "negzero"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_confidence_kinds(dev, kind, numerics, profile):
    """tiny: p and sumk go subnormal; gradual underflow (denormal mode 3) is part of the definition."""
    for form in FORMS:
        _check(dev, form, 67, 33, 9, numerics, profile, kind=kind, stat="signed" if kind == "real" else "depth")


@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_all_ones_is_the_f32_filter_on_the_device(dev, numerics, profile):
    """The tie of the definition, kernel against kernel: c == 1 gives vip_joint_bilateral_run_f32."""
    w, h, k = 67, 33, 9
    f = _source(w, h, "signed")
    for form in FORMS:
        guide = _guide(form, w, h)
        got, got_k = _run(dev, f, _conf("ones", w, h), guide, k, numerics)
        d_ref = dev.empty((h, w), np.float32)
        _BilateralImpl(w, h, k, numerics=numerics).joint_bilateral_filter_f32(dev.put(f), dev.put(guide),
                                                                              _gch(guide), d_ref)
        ref = dev.get(d_ref)
        assert np.array_equal(_bits(got), _bits(ref)), (form, _mismatch(got, ref))
        want = f32_oracle.joint_bilateral(f, guide, k, profile=profile)
        assert np.array_equal(_bits(got), _bits(want)), (form, _mismatch(got, want))
        assert (got_k >= 1).all()


@pytest.mark.parametrize("stat", ["depth", "signed", "tiny"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_source_statistics(dev, stat, numerics, profile):
    for form in FORMS:
        _check(dev, form, 67, 33, 9, numerics, profile, kind="real", stat=stat)


# ---- where c == 0 the source is not read as a number ----
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_source_under_a_hole_is_a_dont_care(dev, numerics, profile):
    w, h, k = 67, 33, 9
    c = _conf("holes", w, h)
    for form in FORMS:
        want, want_k = _want(form, w, h, k, profile)
        for junk in (math.nan, math.inf, 1e38, 0.0):
            f = np.where(c == 0, np.float32(junk), _source(w, h, "depth")).astype(np.float32)
            got, got_k = _run(dev, f, c, _guide(form, w, h), k, numerics)
            assert np.array_equal(_bits(got), _bits(want)), (form, junk, _mismatch(got, want))
            assert np.array_equal(_bits(got_k), _bits(want_k)), (form, junk)


# ---- hole_value: exactly where sumk == 0 ----
@pytest.mark.parametrize("ss,sc", [(10.0, 30.0), (4.0, 3.0 ** 0.5)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_hole_value(dev, ss, sc, numerics, profile):
    """Under sigmas (4, sqrt 3) the colour LUT underflows to 0, so sumk == 0 also arises from the
    weights, but never at a pixel with c > 0 of its own: the centre tap has w = 1."""
    w, h, k = 67, 33, 9
    f, c = _source(w, h, "depth"), _conf("holes", w, h)
    for form in FORMS:
        guide = _guide(form, w, h)
        want, want_k = _want(form, w, h, k, profile, ss=ss, sc=sc)
        empty = want_k == 0
        assert empty.any() and not empty[c > 0].any()
        for hole in (-1.0, 0.0, math.nan):
            got, got_k = _run(dev, f, c, guide, k, numerics, hole=hole, ss=ss, sc=sc)
            assert np.array_equal(_bits(got_k), _bits(want_k)), (form, hole)
            assert np.array_equal(_bits(got[~empty]), _bits(want[~empty])), (form, hole)
            if math.isnan(hole):
                assert np.isnan(got[empty]).all() and not np.isnan(got[~empty]).any(), form
            else:
                assert np.array_equal(_bits(got[empty]), _bits(np.full(int(empty.sum()), hole, np.float32))), form


# ---- shapes (tests/test_gpu_joint_f32.py SHAPES): tiny frames, one pixel either side of the tile
# width and one row either side of the 64-row tile ----
SHAPES = [(1, 1), (2, 3), (3, 1), (64, 64), (67, 5), (127, 3), (129, 3), (63, 3), (65, 3), (9, 63), (9, 65)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_shapes(dev, w, h, k, numerics, profile):
    for form in FORMS:
        _check(dev, form, w, h, k, numerics, profile, kind="real", stat="signed")


@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_1_on_a_frame_taller_than_the_grid(dev, numerics, profile):
    """The elementwise ksize-1 kernel strides its rows over grid.y, which stops at 65535."""
    _check(dev, "gray", 3, 65541, 1, numerics, profile, kind="real", stat="signed")


# ---- pitch and alignment, through the C ABI ----
def _pitched(dev, a, pitch, offset):
    """Device buffer holding the rows of `a` (2-D bytes) at `offset` + r * pitch; (tensor, address)."""
    rows, rowbytes = a.shape
    host = np.full(offset + rows * pitch + 16, 0x5A, np.uint8)
    for r in range(rows):
        host[offset + r * pitch: offset + r * pitch + rowbytes] = a[r]
    t = dev.put(host)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + offset


def _sentinel(dev, h, pitch_f, off):
    t = dev.put(np.full(off // 4 + h * pitch_f + 4, SENTINEL, np.uint32).view(np.int32))
    assert t.data_ptr() % 16 == 0
    return t


def _body(dev, t, h, w, pitch_f, off, tag):
    """The w columns of the h rows written into a sentinel buffer; everything else must be untouched."""
    raw = dev.get(t).view(np.uint32)
    body = raw[off // 4: off // 4 + h * pitch_f].reshape(h, pitch_f)
    assert (body[:, w:] == SENTINEL).all(), (tag, "row padding written")
    assert (raw[:off // 4] == SENTINEL).all() and (raw[off // 4 + h * pitch_f:] == SENTINEL).all(), tag
    return body[:, :w]


# which float array is only 4-byte aligned (base + 4, pitch = 4 mod 16) while the others are
# 16-byte aligned with a pitch of (w + 5) floats = 0 mod 16 bytes; "none": all four are 16-byte aligned
@pytest.mark.parametrize("odd", ["none", "src", "conf", "dst", "weight"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment(dev, k, odd, numerics, profile):
    w, h = 131, 70
    f, c = _source(w, h, "depth"), _conf("holes", w, h)
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    geo = {n: ((4, w + 2) if n == odd else (0, w + 5)) for n in ("src", "conf", "dst", "weight")}  # offset, floats
    t_src, p_src = _pitched(dev, f.view(np.uint8).reshape(h, 4 * w), 4 * geo["src"][1], geo["src"][0])
    t_cnf, p_cnf = _pitched(dev, c.view(np.uint8).reshape(h, 4 * w), 4 * geo["conf"][1], geo["conf"][0])
    t_gg, p_gg = _pitched(dev, _guide("gray", w, h), w + 1, 1)                        # base + 1, pitch w + 1
    t_g3, p_g3 = _pitched(dev, _guide("rgb", w, h).reshape(h, 3 * w), 3 * w + 1, 1)  # base + 1, pitch 3w + 1
    run = _lib.lib().vip_joint_bilateral_run_conf_f32
    for form, pg, gp, gch in (("gray", p_gg, w + 1, 1), ("rgb", p_g3, 3 * w + 1, 3)):
        (doff, dpf), (woff, wpf) = geo["dst"], geo["weight"]
        d_dst, d_wgt = _sentinel(dev, h, dpf, doff), _sentinel(dev, h, wpf, woff)
        rc = run(impl._h, p_src, 4 * geo["src"][1], p_cnf, 4 * geo["conf"][1], pg, gp, gch, HOLE,
                 d_dst.data_ptr() + doff, 4 * dpf, d_wgt.data_ptr() + woff, 4 * wpf, None)
        assert rc == 0, (form, rc)
        want, want_k = _want(form, w, h, k, profile)
        got = _body(dev, d_dst, h, w, dpf, doff, (form, "dst"))
        got_k = _body(dev, d_wgt, h, w, wpf, woff, (form, "weight"))
        assert np.array_equal(got, _bits(want)), (form, odd, _mismatch(got.view(np.float32), want))
        assert np.array_equal(got_k, _bits(want_k)), (form, odd, "weight")
    del t_src, t_cnf, t_gg, t_g3


# ---- argument errors: the C ABI's codes, and VipError / ValueError in Python ----
def test_argument_errors(dev):
    w, h = 16, 8
    impl = _BilateralImpl(w, h, 5)
    big = _BilateralImpl(w, h, 33)  # above the largest ksize (31)
    d_src, d_cnf = dev.put(np.zeros((h + 1, w), np.float32)), dev.put(np.ones((h + 1, w), np.float32))
    d_dst, d_wgt = dev.empty((h + 1, w), np.float32), dev.empty((h + 1, w), np.float32)
    d_g1, d_g3 = dev.put(np.zeros((h, w), np.uint8)), dev.put(np.zeros((h, w, 3), np.uint8))
    s, c, d, k = d_src.data_ptr(), d_cnf.data_ptr(), d_dst.data_ptr(), d_wgt.data_ptr()
    g1, g3 = d_g1.data_ptr(), d_g3.data_ptr()
    p = 4 * w
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING

    def run(hd=impl._h, s=s, sp=p, c=c, cp=p, g=g1, gp=w, gch=1, d=d, dp=p, k=k, kp=p):
        return L.vip_joint_bilateral_run_conf_f32(hd, s, sp, c, cp, g, gp, gch, 0.0, d, dp, k, kp, None)

    assert run() == 0
    assert run(g=g3, gp=3 * w, gch=3) == 0
    assert run(k=None, kp=0) == 0                                     # no weight output: its pitch is not looked at
    assert run(hd=None) == INV
    for null in ("s", "c", "g", "d"):
        assert run(**{null: None}) == INV, null
    for gch in (0, 2, 4, -1):
        assert run(gch=gch) == INV
    for off in (1, 2, 3):                                             # float bases and pitches: multiples of 4
        for name in ("s", "c", "d", "k"):
            assert run(**{name: locals()[name] + off}) == INV, (name, off)
            assert run(**{name + "p": p + off}) == INV, (name, off)
    assert run(s=s + 4, c=c + 4, d=d + 4, k=k + 4) == 0              # any multiple of 4 works
    for name in ("sp", "cp", "dp", "kp"):                             # a pitch smaller than a row
        assert run(**{name: p - 4}) == INV, name
    assert run(gp=w - 1) == INV
    assert run(g=g3, gp=3 * w - 1, gch=3) == INV
    for out in ("d", "k"):                                            # an output equals an input
        for src in (s, c, g1):
            assert run(**{out: src}) == AL, (out, src)
    assert run(k=d) == AL                                             # the two outputs equal each other
    assert run(hd=big._h) == KS
    assert run(hd=big._h, g=g3, gp=3 * w, gch=3) == KS
    assert L.vip_max_ksize(vip.VIP_FILTER_JOINT_CONF) == 31
    dev.torch_.cuda.synchronize()

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    f = vip.CudaBilateralFilter(w, h, 5)
    assert code(f.joint_bilateral_filter_conf_f32, d_src, d_cnf, d_g1, 1, d_src) == AL
    assert code(f.joint_bilateral_filter_conf_f32, d_src, d_cnf, d_g1, 1, d_dst, 0.0, d_cnf) == AL
    assert code(f.joint_bilateral_filter_conf_f32, d_src, d_cnf, d_g1, 2, d_dst) == INV
    assert code(big.joint_bilateral_filter_conf_f32, d_src, d_cnf, d_g3, 3, d_dst) == KS
    with pytest.raises(ValueError):  # a 3-channel guide needs width * height * 3 bytes
        f.joint_bilateral_filter_conf_f32(d_src, d_cnf, d_g1, 3, d_dst)
    with pytest.raises(ValueError):  # the confidence is float32
        f.joint_bilateral_filter_conf_f32(d_src, d_g3, d_g1, 1, d_dst)
    with pytest.raises(ValueError):
        f.joint_bilateral_filter_conf_f32(d_src, d_cnf, d_g1, 1, d_dst, 0.0, dev.empty((h, w // 2), np.float32))


# ---- launch log and kernel timing see the kernels ----
@pytest.mark.parametrize("k", [1, 9])
def test_launch_log_and_timing(dev, k):
    impl = _BilateralImpl(67, 33, k)
    d_src, d_cnf = dev.put(_source(67, 33, "depth")), dev.put(_conf("holes", 67, 33))
    d_guide, d_dst = dev.put(_guide("rgb", 67, 33)), dev.empty((33, 67), np.float32)
    launched_kernels()
    impl.joint_bilateral_filter_conf_f32(d_src, d_cnf, d_guide, 3, d_dst)
    names = launched_kernels()
    assert len(names) == 1 and _kernel_name(k, 3, vip.VIP_NUMERICS_CUDA) in names[0], names
    with kernel_timing(1) as kt:
        impl.joint_bilateral_filter_conf_f32(d_src, d_cnf, d_guide, 3, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "joint_conf_f32" in rec[0][0] and rec[0][1] > 0, rec
