"""GPU parity of the self-guided bilateral filter on an f32 one-channel image
(csrc/vip_bilateral_f32.hpp; include/vip.h vip_bilateral_f32_run).

Bar: every output equals tests/bilateral_f32_oracle.py bit for bit (compared as uint32), in both
numerics profiles. vip::bilateral_f32_kernel<R, FMA> has its own copy of the persistent tile loop,
so the frames of more tiles than the device has CUs (tests/round_shapes.py) are here too.
"""
import ctypes
import functools

import numpy as np
import pytest

import bilateral_f32_oracle as bo
import round_shapes as rs
import various_image_processings_amd as vip
from f32_oracle import f2u8
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _BilateralF32Impl, _BilateralImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
SENTINEL = 0xA5A5A5A5
TH = 64  # bilateral_f32_kernel's tile height: 16 waves x 4 rows at every radius (csrc/vip_bilateral_f32.hpp bf32_waves)


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
def _source(w, h, stat):
    rng = np.random.default_rng(977 * w + 31 * h + len(stat))
    if stat == "depth":
        f = rng.uniform(0.5, 10.0, (h, w))
    elif stat == "signed":
        f = rng.standard_normal((h, w)) * 1000
    elif stat == "tiny":  # +-[1e-36, 1e-30], products with the weights go subnormal
        f = rng.choice([-1.0, 1.0], (h, w)) * 10.0 ** rng.uniform(-36, -30, (h, w))
    elif stat == "ramp":  # a smooth ramp plus noise of a few bins: scaled differences fall in neighbouring bins
        y, x = np.mgrid[0:h, 0:w]
        f = 0.01 * x + 0.007 * y + rng.uniform(0.0, 0.03, (h, w))
    elif stat == "levels":  # two levels more than value_range apart: t clamps to N
        f = np.where(rng.random((h, w)) < 0.5, 1.0, 100.0) + rng.uniform(0.0, 0.5, (h, w))
    elif stat == "huge":  # +-3e38 among moderate values: d overflows to +Inf and clamps
        f = rng.uniform(-5.0, 5.0, (h, w))
        f[rng.random((h, w)) < 0.1] = 3e38
        f[rng.random((h, w)) < 0.1] = -3e38
    elif stat == "ends":  # multiples of 2^-7 in [0, 8]: with value_range 8 (scale 128) t is an integer up to N exactly
        f = rng.integers(0, 1025, (h, w)) / 128.0
        f[::5, ::7], f[::5, 1::7] = 0.0, 8.0
    else:
        assert stat == "integer"
        f = rng.integers(0, 256, (h, w))
    f = np.ascontiguousarray(f, dtype=np.float32)
    f.setflags(write=False)
    return f


# (sigma_space, sigma_color, value_range) per statistic: differences reach well into the table, and past
# its end where said. tiny: sigma_space 0.5 makes the outer spatial weights small enough that f_n * w is subnormal
PARAMS = {
    "depth": (10.0, 3.0, 9.5), "signed": (10.0, 1500.0, 8000.0), "tiny": (0.5, 1e-15, 2e-30),
    "ramp": (10.0, 0.05, 1.0), "levels": (10.0, 5.0, 20.0), "huge": (10.0, 3.0, 10.0), "ends": (10.0, 3.0, 8.0),
    "integer": (10.0, 30.0, 1024.0),
}


@functools.lru_cache(maxsize=None)
def _want(w, h, k, profile, stat="depth", vr=None):
    ss, sc, vr = PARAMS[stat][0], PARAMS[stat][1], (PARAMS[stat][2] if vr is None else vr)
    out = bo.bilateral(_source(w, h, stat), k, ss, sc, vr, profile)
    out.setflags(write=False)
    return out


def _impl(w, h, k, numerics, stat="depth", vr=None):
    ss, sc, vr = PARAMS[stat][0], PARAMS[stat][1], (PARAMS[stat][2] if vr is None else vr)
    return _BilateralF32Impl(w, h, k, ss, sc, vr, numerics)


def _run(dev, f, impl):
    h, w = f.shape
    d_dst = dev.put(np.full((h, w), SENTINEL, np.uint32).view(np.float32))
    impl.bilateral_filter(dev.put(f.copy()), d_dst)  # f is read-only: torch wants a writable array
    return dev.get(d_dst)


def _check(dev, w, h, k, numerics, profile, stat="depth", vr=None):
    launched_kernels()
    got = _run(dev, _source(w, h, stat), _impl(w, h, k, numerics, stat, vr=vr))
    names = launched_kernels()
    assert names == [f"void vip::bilateral_f32_kernel<{k // 2}, {_fma(numerics)}>"] or \
        names == [f"vip::bilateral_f32_kernel<{k // 2}, {_fma(numerics)}>"], names
    want = _want(w, h, k, profile, stat, vr=vr)
    assert np.array_equal(_bits(got), _bits(want)), (w, h, k, stat, _mismatch(got, want))


# ---- every ksize on 37 x 23, the launched instantiation asserted ----
@pytest.mark.parametrize("k", range(1, 32, 2))
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_every_ksize(dev, k, numerics, profile):
    _check(dev, 37, 23, k, numerics, profile)


# ---- ragged frames: one pixel, a few, one pixel over a tile each way, three tile columns ----
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (129, 65), (259, 70)])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ragged_frames(dev, w, h, k, numerics, profile):
    _check(dev, w, h, k, numerics, profile)


# ---- source statistics ----
@pytest.mark.parametrize("stat", ["depth", "signed", "tiny", "ramp", "levels", "huge"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_source_statistics(dev, stat, numerics, profile):
    """tiny: gradual underflow (denormal mode 3) is part of the definition. ramp: neighbouring
    bins, a nonzero interpolation fraction at nearly every tap. levels: differences past
    value_range, t clamps to N. huge: 3e38 - (-3e38) overflows to +Inf, which clamps as well."""
    w, h = 67, 33
    f = _source(w, h, stat)
    vr = PARAMS[stat][2]
    with np.errstate(over="ignore"):
        t = np.abs(f[:, 1:] - f[:, :-1]) * bo.scale_of(vr)
    if stat == "ramp":
        assert (t < 64).all() and len(np.unique(t.astype(np.int32))) > 20 and (t != np.floor(t)).mean() > 0.9
    if stat == "levels":
        assert (t > bo.BINS).mean() > 0.3 and (t < bo.BINS).mean() > 0.3
    if stat == "huge":
        assert np.isinf(t).any() and np.isfinite(f).all()
    _check(dev, w, h, 9, numerics, profile, stat)


# ---- table ends: value_range 8 on multiples of 2^-7 puts differences exactly on t = N (and on
# every other integer); value_range 8 (1 + 2^-20) puts the same differences just below it ----
@pytest.mark.parametrize("vr", [8.0, 8.0 * (1 + 2.0 ** -20)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_table_ends(dev, vr, numerics, profile):
    w, h = 67, 33
    f = _source(w, h, "ends")
    t = np.abs(f[:, 1:] - f[:, :-1]) * bo.scale_of(vr)
    if vr == 8.0:
        assert (t == bo.BINS).any() and (t == np.floor(t)).all()
    else:
        assert (t < bo.BINS).all() and (t > bo.BINS - 1).any()
    _check(dev, w, h, 9, numerics, profile, "ends", vr=vr)


# ---- pitch and alignment, through the C ABI ----
def _pitched(dev, a, pitch, offset):
    """Device buffer holding the rows of `a` (2-D bytes) at `offset` + r * pitch; (tensor, address)."""
    rows, rowbytes = a.shape
    host = np.full(offset + rows * pitch + 16, 0x5A, np.uint8)
    for r in range(rows):
        host[offset + r * pitch: offset + r * pitch + rowbytes] = a[r]
    t = dev.put(host)
    return t, t.data_ptr() + offset


# (offset, pitch in floats) of source and destination: dense; base and pitch multiples of 16;
# multiples of 4 only (pitch 4 w + 4, base offset 4)
@pytest.mark.parametrize("off,pf", [(0, 131), (0, 132), (4, 132)])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment(dev, k, off, pf, numerics, profile):
    w, h = 131, 70
    f = _source(w, h, "depth")
    impl = _impl(w, h, k, numerics)
    t_src, p_src = _pitched(dev, f.view(np.uint8).reshape(h, 4 * w), 4 * pf, off)
    words = off // 4 + h * pf + 4
    d_dst = dev.put(np.full(words, SENTINEL, np.uint32).view(np.int32))
    assert t_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    rc = _lib.lib().vip_bilateral_f32_run(impl._h, p_src, 4 * pf, d_dst.data_ptr() + off, 4 * pf, None)
    assert rc == 0, rc
    raw = dev.get(d_dst).view(np.uint32)
    body = raw[off // 4: off // 4 + h * pf].reshape(h, pf)
    want = _want(w, h, k, profile)
    assert np.array_equal(body[:, :w], _bits(want)), _mismatch(body[:, :w].view(np.float32), want)
    assert (body[:, w:] == SENTINEL).all()  # the row padding is the caller's
    assert (raw[:off // 4] == SENTINEL).all() and (raw[off // 4 + h * pf:] == SENTINEL).all()
    del t_src


# ---- a row band on 129 x 200: rows 6..190 with neighbours clamped to [5, 195) ----
@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_row_band(dev, k, numerics, profile):
    w, h = 129, 200
    out_rows, src_row0, row_lo, row_hi = 185, 6, 5, 195
    f = _source(w, h, "depth")
    impl = _impl(w, h, k, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w), SENTINEL, np.uint32).view(np.float32))
    impl.run_rows(dev.put(f.copy()), d_dst, out_rows, src_row0, row_lo, row_hi)
    out = dev.get(d_dst)
    want = bo.bilateral_rows(f, out_rows, src_row0, row_lo, row_hi, k, *PARAMS["depth"], profile)
    assert np.array_equal(_bits(out[:out_rows]), _bits(want)), _mismatch(out[:out_rows], want)
    assert (_bits(out[out_rows:]) == SENTINEL).all()  # rows past out_rows are untouched


# ---- the u8 tie on the device ----
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_integer_source_rounds_to_the_u8_filter(dev, numerics, profile):
    """value_range 1024, f = float32(g): u8(dst + 0.5f) is vip_bilateral_run_c1 run on the same device."""
    w, h, k = 259, 70, 9
    f = _source(w, h, "integer")
    u8 = _BilateralImpl(w, h, k, 10.0, 30.0, numerics)
    d_u8 = dev.empty((h, w))
    u8.bilateral_filter_c1(dev.put(f.astype(np.uint8)), d_u8)
    got = f2u8(_run(dev, f, _impl(w, h, k, numerics, "integer")) + np.float32(0.5))
    assert np.array_equal(got, dev.get(d_u8)), np.argwhere(got != dev.get(d_u8))[:5].tolist()


# ---- later rounds of the persistent loop (this kernel's own copy of it) ----
@pytest.fixture(scope="module")
def cus(dev):
    """The number csrc/vip_launch.hpp device_cus() reads."""
    return int(dev.torch_.cuda.get_device_properties(0).multi_processor_count)


def _frame(kind, cus):
    """(w, h) of the tall or wide frame, with its rounds asserted before any launch."""
    w, h = {"tall": rs.tall, "wide": rs.wide}[kind](cus, TH)
    tiles, full, last = rs.rounds(w, h, TH, cus)
    assert tiles > cus and full >= (2 if kind == "tall" else 1) and 0 < last < cus, (kind, w, h, tiles, full, last)
    assert 0 < h % TH < TH
    return w, h


def _rounds_check(dev, cus, kind, k, numerics, profile):
    w, h = _frame(kind, cus)
    f = _source(w, h, "depth")
    ss, sc, vr = PARAMS["depth"]
    launched_kernels()
    got = _run(dev, f, _impl(w, h, k, numerics))
    names = launched_kernels()
    assert len(names) == 1 and f"vip::bilateral_f32_kernel<{k // 2}, {_fma(numerics)}>" in names[0], names
    want = rs.in_bands(lambda p: bo.bilateral(p, k, ss, sc, vr, profile), k // 2, f, threads=16)
    assert np.array_equal(_bits(got), _bits(want)), (kind, w, h, k, _mismatch(got, want))


@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_rounds_tall(dev, cus, k, numerics, profile):
    _rounds_check(dev, cus, "tall", k, numerics, profile)


def test_rounds_wide(dev, cus):
    _rounds_check(dev, cus, "wide", 5, *PROFILES[0])


def test_rounds_band(dev, cus):
    """One band on the tall frame: it lies one row inside [row_lo, row_hi), narrower than the frame
    at both ends, and is more than two rounds tall."""
    numerics, profile = PROFILES[1]
    h, row_lo, row_hi, src_row0, out_rows = rs.band(cus, TH)
    w = rs.tall(cus, TH)[0]
    tiles, full, last = rs.rounds(w, out_rows, TH, cus)
    assert full >= 2 and 0 < last < cus and 0 < out_rows % TH < TH, (tiles, full, last)
    f = _source(w, h, "depth")
    ss, sc, vr = PARAMS["depth"]
    impl = _impl(w, h, 5, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w), SENTINEL, np.uint32).view(np.float32))
    impl.run_rows(dev.put(f.copy()), d_dst, out_rows, src_row0, row_lo, row_hi)
    out = dev.get(d_dst)
    crop = np.ascontiguousarray(f[row_lo:row_hi])
    want = rs.in_bands(lambda p: bo.bilateral(p, 5, ss, sc, vr, profile), 2, crop, threads=16)
    want = want[src_row0 - row_lo:src_row0 - row_lo + out_rows]
    assert np.array_equal(_bits(out[:out_rows]), _bits(want)), _mismatch(out[:out_rows], want)
    assert (_bits(out[out_rows:]) == SENTINEL).all()


# ---- non-finite input: values only; the kernel's index clamp keeps every table read inside the table ----
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_non_finite_input_stays_local(dev, numerics, profile):
    """A NaN, a +Inf and a -Inf in a 129 x 65 depth frame at ksize 9: every output farther than the
    radius from all three equals the oracle of the clean frame; nothing is asserted about the others."""
    w, h, k = 129, 65, 9
    clean = _source(w, h, "depth")
    f = clean.copy()
    spots = [(10, 20), (40, 100), (63, 127)]
    for (y, x), v in zip(spots, (np.nan, np.inf, -np.inf)):
        f[y, x] = v
    got = _run(dev, f, _impl(w, h, k, numerics))
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
    d_src, d_dst = dev.put(np.zeros((h + 1, w), np.float32)), dev.empty((h + 1, w), np.float32)
    s, d, p = d_src.data_ptr(), d_dst.data_ptr(), 4 * w
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING
    run, rows = L.vip_bilateral_f32_run, L.vip_bilateral_f32_run_rows
    launched_kernels()
    assert run(None, s, p, d, p, None) == INV
    assert run(impl._h, None, p, d, p, None) == INV
    assert run(impl._h, s, p, None, p, None) == INV
    for off in (1, 2, 3):  # bases and pitches must be multiples of 4
        assert run(impl._h, s + off, p, d, p, None) == INV
        assert run(impl._h, s, p, d + off, p, None) == INV
        assert run(impl._h, s, p + off, d, p, None) == INV
        assert run(impl._h, s, p, d, p + off, None) == INV
    assert rows(None, s, p, d, p, h, 0, 0, h, None) == INV
    for band in ((h, 0, 4, 4), (h, 0, -1, h), (h, 0, 0, h + 1), (-1, 0, 0, h)):  # out_rows, src_row0, lo, hi
        assert rows(impl._h, s, p, d, p, *band, None) == INV, band
    assert run(impl._h, s, p, s, p, None) == AL
    assert launched_kernels() == []  # none of them launched
    assert run(impl._h, s + 4, p, d + 4, p, None) == 0  # any multiple of 4 works
    assert len(launched_kernels()) == 1
    dev.torch_.cuda.synchronize()
    handle = ctypes.byref(_lib._c_void_p())
    create = L.vip_bilateral_f32_create
    assert create(handle, w, h, 33, 10.0, 3.0, 10.0, 0) == KS
    assert create(handle, w, h, 4, 10.0, 3.0, 10.0, 0) == KS
    for vr in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
        assert create(handle, w, h, 5, 10.0, 3.0, vr, 0) == INV, vr
    assert create(handle, 0, h, 5, 10.0, 3.0, 10.0, 0) == INV and create(None, w, h, 5, 10.0, 3.0, 10.0, 0) == INV

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    flt = vip.CudaBilateralFilterF32(w, h, 5, 10.0, 3.0, 10.0)
    assert code(flt.bilateral_filter, d_src, d_src) == AL
    assert code(impl.run_rows, d_src, d_dst, h, 0, 4, 4) == INV
    assert code(vip.CudaBilateralFilterF32, w, h, 33) == KS
    with pytest.raises(ValueError):  # float32, width * height * 4 bytes
        flt.bilateral_filter(d_src, dev.empty((h, w // 2), np.float32))
    with pytest.raises(ValueError):
        flt.bilateral_filter(dev.put(np.zeros((h, w), np.uint8)), d_dst)


# ---- launch log and kernel timing see the kernel ----
@pytest.mark.parametrize("k", [1, 9])
def test_launch_log_and_timing(dev, k):
    impl = _impl(67, 33, k, vip.VIP_NUMERICS_CUDA)
    d_src, d_dst = dev.put(_source(67, 33, "depth").copy()), dev.empty((33, 67), np.float32)
    launched_kernels()
    impl.bilateral_filter(d_src, d_dst)
    names = launched_kernels()
    assert len(names) == 1 and f"bilateral_f32_kernel<{k // 2}, true>" in names[0], names
    with kernel_timing(1) as kt:
        impl.bilateral_filter(d_src, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "bilateral_f32_kernel" in rec[0][0] and rec[0][1] > 0, rec
