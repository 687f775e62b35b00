"""GPU parity of the joint bilateral filter of an f32 one-channel source under an f32 one-channel
guide (csrc/vip_bilateral_f32j.hpp; include/vip.h vip_bilateral_f32_run_joint).

Bar: every output equals tests/bilateral_f32_joint_oracle.py bit for bit (compared as uint32), in
both numerics profiles. vip::bilateral_f32_joint_kernel<R, FMA> has its own copy of the persistent
tile loop, which commits two planes, so the frames of more tiles than the device has CUs
(tests/round_shapes.py) are here too.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import bilateral_f32_joint_oracle as jo
import bilateral_f32_oracle as bo
import round_shapes as rs
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _BilateralF32Impl, _BilateralImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
SENTINEL = 0xA5A5A5A5
CAP = 31  # vip_bilateral_f32_max_ksize_joint(), asserted in test_cap


def waves(k):
    """Waves per workgroup of bilateral_f32_joint_kernel<k // 2> (csrc/vip_bilateral_f32j.hpp bf32j_waves):
    the most that the registers hold without scratch (LDS would allow 16 up to radius 8 and 12 up to 13)."""
    r = k // 2
    return 16 if r <= 2 else (12 if r <= 8 else 8)


def tile_rows(k):
    return 4 * waves(k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mismatch(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    first = [(tuple(i), float(a[tuple(i)]), float(b[tuple(i)])) for i in d[:4]]
    return f"{len(d)} mismatches of {a.size}, first (index, got, want) {first}"


def _fma(numerics):
    return "true" if numerics == vip.VIP_NUMERICS_CUDA else "false"


# ---- inputs and their oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _guide(w, h, stat="depth"):
    rng = np.random.default_rng(977 * w + 31 * h + len(stat))
    if stat == "depth":
        g = rng.uniform(0.5, 10.0, (h, w))
    elif stat == "ends":  # multiples of 2^-7 in [0, 8]: with value_range 8 (scale 128) t is an integer up to N exactly
        g = rng.integers(0, 1025, (h, w)) / 128.0
        g[::5, ::7], g[::5, 1::7] = 0.0, 8.0
    elif stat == "levels":  # two levels more than value_range apart: t clamps to N
        g = np.where(rng.random((h, w)) < 0.5, 1.0, 100.0) + rng.uniform(0.0, 0.5, (h, w))
    else:
        assert stat == "integer"
        g = rng.integers(0, 256, (h, w))
    g = np.ascontiguousarray(g, dtype=np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _source(w, h):
    """Signed noise independent of every guide, with a few -0 and exact zeros."""
    rng = np.random.default_rng(613 * w + 17 * h + 5)
    f = (rng.standard_normal((h, w)) * 50).astype(np.float32)
    f[rng.random((h, w)) < 0.02] = np.float32(-0.0)
    f.setflags(write=False)
    return f


# (sigma_space, sigma_color, value_range) per guide statistic
PARAMS = {"depth": (10.0, 3.0, 9.5), "ends": (10.0, 3.0, 8.0), "levels": (10.0, 5.0, 20.0),
          "integer": (10.0, 30.0, 1024.0)}


@functools.lru_cache(maxsize=None)
def _want(w, h, k, profile, stat="depth", vr=None):
    ss, sc, vr = PARAMS[stat][0], PARAMS[stat][1], (PARAMS[stat][2] if vr is None else vr)
    out = jo.joint(_source(w, h), _guide(w, h, stat), k, ss, sc, vr, profile)
    out.setflags(write=False)
    return out


def _impl(w, h, k, numerics, stat="depth", vr=None):
    ss, sc, vr = PARAMS[stat][0], PARAMS[stat][1], (PARAMS[stat][2] if vr is None else vr)
    return _BilateralF32Impl(w, h, k, ss, sc, vr, numerics)


def _run(dev, f, g, impl):
    h, w = f.shape
    d_dst = dev.put(np.full((h, w), SENTINEL, np.uint32).view(np.float32))
    impl.joint_bilateral_filter(dev.put(f.copy()), dev.put(g.copy()), d_dst)  # read-only arrays: torch wants writable ones
    return dev.get(d_dst)


def _check(dev, w, h, k, numerics, profile, stat="depth", vr=None):
    launched_kernels()
    got = _run(dev, _source(w, h), _guide(w, h, stat), _impl(w, h, k, numerics, stat, vr=vr))
    names = launched_kernels()
    assert len(names) == 1 and names[0].endswith(f"vip::bilateral_f32_joint_kernel<{k // 2}, {_fma(numerics)}>"), names
    want = _want(w, h, k, profile, stat, vr=vr)
    assert np.array_equal(_bits(got), _bits(want)), (w, h, k, stat, _mismatch(got, want))


def test_cap():
    cap = _lib.lib().vip_bilateral_f32_max_ksize_joint()
    assert cap == CAP and cap >= 15 and cap % 2 == 1 and cap <= 31
    assert [waves(k) for k in (5, 7, 17, 19, CAP)] == [16, 12, 12, 8, 8]


# ---- every ksize on 150 x 70: past the 128-column seam and the 64-, 48- and 32-row seams ----
@pytest.mark.parametrize("k", range(1, CAP + 1, 2))
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_every_ksize(dev, k, numerics, profile):
    assert 150 > rs.TW and 70 > tile_rows(k)
    _check(dev, 150, 70, k, numerics, profile)


# ---- ragged frames: one pixel, a few, one pixel over a tile each way, three tile columns; ksize 5, 17
# and the cap are the largest of each wave count, 17 and 27 what LDS alone would make the largest ----
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (129, 65), (259, 70)])
@pytest.mark.parametrize("k", [5, 15, 17, 27, CAP])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ragged_frames(dev, w, h, k, numerics, profile):
    _check(dev, w, h, k, numerics, profile)


# ---- I1: g == f is the self-guided filter, with the guide in a buffer of its own and with d_guide == d_src ----
@pytest.mark.parametrize("k", [1, 9, 19, CAP])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_guide_equal_to_source_is_the_self_guided_filter(dev, k, numerics, profile):
    w, h = 259, 70
    f = _guide(w, h, "depth")
    impl = _impl(w, h, k, numerics)
    d_src, d_copy = dev.put(f.copy()), dev.put(f.copy())
    d_self, d_sep, d_same = (dev.put(np.full((h, w), SENTINEL, np.uint32).view(np.float32)) for _ in range(3))
    impl.bilateral_filter(d_src, d_self)
    launched_kernels()
    for d_guide, d_out in ((d_copy, d_sep), (d_src, d_same)):  # the log names a kernel once: read it per call
        impl.joint_bilateral_filter(d_src, d_guide, d_out)
        names = launched_kernels()  # d_guide == d_src launches this kernel too: no forwarding
        assert len(names) == 1 and f"bilateral_f32_joint_kernel<{k // 2}, {_fma(numerics)}>" in names[0], names
    want = dev.get(d_self)
    assert np.array_equal(_bits(want), _bits(bo.bilateral(f, k, *PARAMS["depth"], profile)))
    for got in (dev.get(d_sep), dev.get(d_same)):
        assert np.array_equal(_bits(got), _bits(want)), _mismatch(got, want)


# ---- I2: value_range 1024 under g = float(g8) is the f32 joint filter under the 8-bit guide g8 ----
@pytest.mark.parametrize("k", [5, 15, CAP])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_integer_guide_is_the_u8_guided_filter(dev, k, numerics, profile):
    w, h = 259, 70
    f, g = _source(w, h), _guide(w, h, "integer")
    ss, sc, vr = PARAMS["integer"]
    u8 = _BilateralImpl(w, h, k, ss, sc, numerics)
    d_src = dev.put(f.copy())
    d_u8 = dev.put(np.full((h, w), SENTINEL, np.uint32).view(np.float32))
    u8.joint_bilateral_filter_f32(d_src, dev.put(g.astype(np.uint8)), 1, d_u8)
    got = _run(dev, f, g, _impl(w, h, k, numerics, "integer"))
    want = dev.get(d_u8)
    assert np.array_equal(_bits(got), _bits(want)), _mismatch(got, want)


# ---- table ends: value_range 8 on multiples of 2^-7 puts guide differences exactly on t = N (and on
# every other integer); value_range 8 (1 + 2^-20) puts the same differences just below it; a
# value_range below the guide's spread clamps taps to N ----
@pytest.mark.parametrize("vr", [8.0, 8.0 * (1 + 2.0 ** -20)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_table_ends(dev, vr, numerics, profile):
    w, h = 67, 33
    g = _guide(w, h, "ends")
    t = np.abs(g[:, 1:] - g[:, :-1]) * bo.scale_of(vr)
    if vr == 8.0:
        assert (t == bo.BINS).any() and (t == np.floor(t)).all()
    else:
        assert (t < bo.BINS).all() and (t > bo.BINS - 1).any()
    _check(dev, w, h, 9, numerics, profile, "ends", vr=vr)


@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_value_range_below_the_guides_spread_clamps(dev, numerics, profile):
    w, h = 67, 33
    g = _guide(w, h, "levels")
    t = np.abs(g[:, 1:] - g[:, :-1]) * bo.scale_of(PARAMS["levels"][2])
    assert (t > bo.BINS).mean() > 0.3 and (t < bo.BINS).mean() > 0.3
    _check(dev, w, h, 9, numerics, profile, "levels")


# ---- pitch and alignment, through the C ABI ----
def _pitched(dev, a, pitch, offset):
    """Device buffer holding the rows of `a` (2-D bytes) at `offset` + r * pitch; (tensor, address)."""
    rows, rowbytes = a.shape
    host = np.full(offset + rows * pitch + 16, 0x5A, np.uint8)
    for r in range(rows):
        host[offset + r * pitch: offset + r * pitch + rowbytes] = a[r]
    t = dev.put(host)
    return t, t.data_ptr() + offset


# (base offset in bytes, pitch in floats) of a buffer: dense (pitch no multiple of 16 bytes); base and pitch
# multiples of 16; pitch a multiple of 16 but the base offset 4
LAYOUTS = [(0, 131), (0, 132), (4, 132)]


def _layout_check(dev, k, src_l, guide_l, dst_l, numerics, profile):
    w, h = 131, 70
    f, g = _source(w, h), _guide(w, h)
    impl = _impl(w, h, k, numerics)
    (so, sp), (go, gp), (do, dp) = LAYOUTS[src_l], LAYOUTS[guide_l], LAYOUTS[dst_l]
    t_src, p_src = _pitched(dev, f.view(np.uint8).reshape(h, 4 * w), 4 * sp, so)
    t_guide, p_guide = _pitched(dev, g.view(np.uint8).reshape(h, 4 * w), 4 * gp, go)
    words = do // 4 + h * dp + 4
    d_dst = dev.put(np.full(words, SENTINEL, np.uint32).view(np.int32))
    assert t_src.data_ptr() % 16 == 0 and t_guide.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    rc = _lib.lib().vip_bilateral_f32_run_joint(impl._h, p_src, 4 * sp, p_guide, 4 * gp, d_dst.data_ptr() + do,
                                                4 * dp, None)
    assert rc == 0, rc
    raw = dev.get(d_dst).view(np.uint32)
    body = raw[do // 4: do // 4 + h * dp].reshape(h, dp)
    want = _want(w, h, k, profile)
    assert np.array_equal(body[:, :w], _bits(want)), _mismatch(body[:, :w].view(np.float32), want)
    assert (body[:, w:] == SENTINEL).all()  # the row padding is the caller's
    assert (raw[:do // 4] == SENTINEL).all() and (raw[do // 4 + h * dp:] == SENTINEL).all()
    del t_src, t_guide


# source, guide and destination vary independently: all 27 combinations of the three layouts at ksize 5
@pytest.mark.parametrize("src_l,guide_l,dst_l", list(itertools.product(range(3), repeat=3)))
def test_pitch_and_alignment(dev, src_l, guide_l, dst_l):
    _layout_check(dev, 5, src_l, guide_l, dst_l, *PROFILES[0])


# the three layouts rotated over the three buffers, in a 12-wave kernel and in both profiles
@pytest.mark.parametrize("src_l,guide_l,dst_l", [(0, 1, 2), (1, 2, 0), (2, 0, 1)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment_12_waves(dev, src_l, guide_l, dst_l, numerics, profile):
    _layout_check(dev, 19, src_l, guide_l, dst_l, numerics, profile)


# ---- a row band on 129 x 200: rows 6..190 with neighbours of both images clamped to [5, 195) ----
@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_row_band(dev, k, numerics, profile):
    w, h = 129, 200
    out_rows, src_row0, row_lo, row_hi = 185, 6, 5, 195
    f, g = _source(w, h), _guide(w, h)
    impl = _impl(w, h, k, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w), SENTINEL, np.uint32).view(np.float32))
    impl.run_rows_joint(dev.put(f.copy()), dev.put(g.copy()), d_dst, out_rows, src_row0, row_lo, row_hi)
    out = dev.get(d_dst)
    want = jo.joint_rows(f, g, out_rows, src_row0, row_lo, row_hi, k, *PARAMS["depth"], profile)
    assert np.array_equal(_bits(out[:out_rows]), _bits(want)), _mismatch(out[:out_rows], want)
    assert (_bits(out[out_rows:]) == SENTINEL).all()  # rows past out_rows are untouched


# ---- later rounds of the persistent loop (this kernel's own copy of it, which commits both planes) ----
@pytest.fixture(scope="module")
def cus(dev):
    """The number csrc/vip_launch.hpp device_cus() reads."""
    return int(dev.torch_.cuda.get_device_properties(0).multi_processor_count)


def _frame(kind, cus, th):
    """(w, h) of the tall or wide frame, with its rounds asserted before any launch."""
    w, h = {"tall": rs.tall, "wide": rs.wide}[kind](cus, th)
    tiles, full, last = rs.rounds(w, h, th, cus)
    assert tiles > cus and full >= (2 if kind == "tall" else 1) and 0 < last < cus, (kind, w, h, tiles, full, last)
    assert 0 < h % th < th
    return w, h


def _rounds_check(dev, cus, kind, k, numerics, profile):
    w, h = _frame(kind, cus, tile_rows(k))
    f, g = _source(w, h), _guide(w, h)
    ss, sc, vr = PARAMS["depth"]
    launched_kernels()
    got = _run(dev, f, g, _impl(w, h, k, numerics))
    names = launched_kernels()
    assert len(names) == 1 and f"vip::bilateral_f32_joint_kernel<{k // 2}, {_fma(numerics)}>" in names[0], names
    want = rs.in_bands(lambda p, q: jo.joint(p, q, k, ss, sc, vr, profile), k // 2, f, g, threads=16)
    assert np.array_equal(_bits(got), _bits(want)), (kind, w, h, k, _mismatch(got, want))


@pytest.mark.parametrize("k", [5, CAP])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_rounds_tall(dev, cus, k, numerics, profile):
    _rounds_check(dev, cus, "tall", k, numerics, profile)


def test_rounds_wide(dev, cus):
    _rounds_check(dev, cus, "wide", 5, *PROFILES[0])


# ---- non-finite input: values only; the kernel's index clamp keeps every table read inside the table ----
@pytest.mark.parametrize("where", ["guide", "source"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_non_finite_input_stays_local(dev, where, numerics, profile):
    """A NaN, a +Inf and a -Inf in the guide or in the source of a 129 x 65 frame at ksize 9: every
    output farther than the radius from all three equals the oracle of the clean frame; nothing is
    asserted about the others."""
    w, h, k = 129, 65, 9
    f, g = _source(w, h).copy(), _guide(w, h).copy()
    spots = [(10, 20), (40, 100), (63, 127)]
    for (y, x), v in zip(spots, (np.nan, np.inf, -np.inf)):
        (g if where == "guide" else f)[y, x] = v
    got = _run(dev, f, g, _impl(w, h, k, numerics))
    yy, xx = np.mgrid[0:h, 0:w]
    far = np.ones((h, w), bool)
    for y, x in spots:
        far &= (np.abs(yy - y) > k // 2) | (np.abs(xx - x) > k // 2)
    want = _want(w, h, k, profile)
    assert far.sum() > h * w - 3 * k * k
    assert np.array_equal(_bits(got)[far], _bits(want)[far]), _mismatch(np.where(far, got, 0), np.where(far, want, 0))


# ---- argument errors: the C ABI's codes, without a launch ----
def test_argument_errors(dev):
    w, h = 16, 8
    impl = _BilateralF32Impl(w, h, 5, 10.0, 3.0, 10.0)
    d_src, d_guide = dev.put(np.zeros((h + 1, w), np.float32)), dev.put(np.ones((h + 1, w), np.float32))
    d_dst = dev.empty((h + 1, w), np.float32)
    s, g, d, p = d_src.data_ptr(), d_guide.data_ptr(), d_dst.data_ptr(), 4 * w
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING
    run, rows = L.vip_bilateral_f32_run_joint, L.vip_bilateral_f32_run_rows_joint
    launched_kernels()
    assert run(None, s, p, g, p, d, p, None) == INV
    assert run(impl._h, None, p, g, p, d, p, None) == INV
    assert run(impl._h, s, p, None, p, d, p, None) == INV
    assert run(impl._h, s, p, g, p, None, p, None) == INV
    for off in (1, 2, 3):  # bases and pitches must be multiples of 4
        assert run(impl._h, s + off, p, g, p, d, p, None) == INV
        assert run(impl._h, s, p, g + off, p, d, p, None) == INV
        assert run(impl._h, s, p, g, p, d + off, p, None) == INV
        assert run(impl._h, s, p + off, g, p, d, p, None) == INV
        assert run(impl._h, s, p, g, p + off, d, p, None) == INV
        assert run(impl._h, s, p, g, p, d, p + off, None) == INV
    for short in ((p - 4, p, p), (p, p - 4, p), (p, p, p - 4)):  # pitches are at least width * 4
        assert run(impl._h, s, short[0], g, short[1], d, short[2], None) == INV, short
    assert rows(None, s, p, g, p, d, p, h, 0, 0, h, None) == INV
    for band in ((h, 0, 4, 4), (h, 0, -1, h), (h, 0, 0, h + 1), (-1, 0, 0, h)):  # out_rows, src_row0, lo, hi
        assert rows(impl._h, s, p, g, p, d, p, *band, None) == INV, band
    assert run(impl._h, s, p, g, p, s, p, None) == AL  # d_dst == d_src
    assert run(impl._h, s, p, g, p, g, p, None) == AL  # d_dst == d_guide
    assert launched_kernels() == []  # none of them launched
    assert run(impl._h, s + 4, p, g + 4, p, d + 4, p, None) == 0  # any multiple of 4 works
    assert len(launched_kernels()) == 1
    assert run(impl._h, s, p, s, p, d, p, None) == 0  # d_guide == d_src is allowed
    assert len(launched_kernels()) == 1
    dev.torch_.cuda.synchronize()
    # a ksize above the cap: no handle can hold one while the cap is the handle's own (31); below that the run refuses
    cap = L.vip_bilateral_f32_max_ksize_joint()
    if cap < L.vip_bilateral_f32_max_ksize():
        big = _BilateralF32Impl(w, h, cap + 2, 10.0, 3.0, 10.0)
        assert run(big._h, s, p, g, p, d, p, None) == KS
    else:
        assert L.vip_bilateral_f32_create(ctypes.byref(_lib._c_void_p()), w, h, cap + 2, 10.0, 3.0, 10.0, 0) == KS

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    flt = vip.CudaBilateralFilterF32(w, h, 5, 10.0, 3.0, 10.0)
    assert code(flt.joint_bilateral_filter, d_src, d_guide, d_src) == AL
    assert code(flt.joint_bilateral_filter, d_src, d_guide, d_guide) == AL
    assert code(impl.run_rows_joint, d_src, d_guide, d_dst, h, 0, 4, 4) == INV
    with pytest.raises(ValueError):  # float32, width * height * 4 bytes
        flt.joint_bilateral_filter(d_src, dev.empty((h, w // 2), np.float32), d_dst)
    with pytest.raises(ValueError):
        flt.joint_bilateral_filter(d_src, dev.put(np.zeros((h, w), np.uint8)), d_dst)


# ---- launch log and kernel timing see the kernel ----
@pytest.mark.parametrize("k", [1, 9])
def test_launch_log_and_timing(dev, k):
    impl = _impl(67, 33, k, vip.VIP_NUMERICS_CUDA)
    d_src, d_guide = dev.put(_source(67, 33).copy()), dev.put(_guide(67, 33).copy())
    d_dst = dev.empty((33, 67), np.float32)
    launched_kernels()
    impl.joint_bilateral_filter(d_src, d_guide, d_dst)
    names = launched_kernels()
    assert len(names) == 1 and f"bilateral_f32_joint_kernel<{k // 2}, true>" in names[0], names
    with kernel_timing(1) as kt:
        impl.joint_bilateral_filter(d_src, d_guide, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "bilateral_f32_joint_kernel" in rec[0][0] and rec[0][1] > 0, rec
