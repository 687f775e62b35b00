"""GPU parity of the self-guided bilateral filter on an f32 image of 2 and 3 interleaved channels
(csrc/vip_bilateral_f32c.hpp; include/vip.h vip_bilateral_f32_run_c).

Bar: every output equals tests/bilateral_f32c_oracle.py bit for bit (compared as uint32), in both
numerics profiles. vip::bilateral_f32c_kernel<R, C, FMA> has its own copy of the persistent tile
loop, so the frames of more tiles than the device has CUs (tests/round_shapes.py) are here too,
with this kernel's own tile heights.
"""
import functools

import numpy as np
import pytest

import bilateral_f32_oracle as bo
import bilateral_f32c_oracle as bc
import round_shapes as rs
import various_image_processings_amd as vip
from f32_oracle import f2u8
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _BilateralF32Impl, _BilateralImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
CHANNELS = [2, 3]
SENTINEL = 0xA5A5A5A5


def tile_rows(ch, radius):
    """bilateral_f32c_kernel's tile height, 4 rows per wave (csrc/vip_bilateral_f32c.hpp bf32c_max_waves and
    Bf32cForm: what the registers hold, then what LDS allows beside the 65,600-byte table)."""
    assert ch in (2, 3) and 1 <= radius <= 7
    max_waves = (16 if radius <= 2 else 12) if ch == 2 else (12 if radius <= 2 else 8)
    waves = rs.pick_waves(radius, ch, max_waves, 1025 * 2 * 8)
    assert waves >= 8
    return rs.RPW * waves


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mismatch(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    first = [(tuple(i), float(a[tuple(i)]), float(b[tuple(i)])) for i in d[:4]]
    return f"{len(d)} mismatches of {a.size}, first (index, got, want) {first}"


def _fma(numerics):
    return "true" if numerics == vip.VIP_NUMERICS_CUDA else "false"


def _kernel(ch, k, numerics):
    if k == 1:
        return f"vip::bilateral_f32c_k1_kernel<{ch}, {_fma(numerics)}>"
    return f"vip::bilateral_f32c_kernel<{k // 2}, {ch}, {_fma(numerics)}>"


# ---- inputs and their oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _source(w, h, ch, stat):
    """Per-channel data: every channel is drawn on its own."""
    rng = np.random.default_rng(977 * w + 31 * h + 7 * ch + len(stat))
    shape = (h, w, ch)
    if stat == "depth":
        f = rng.uniform(0.5, 10.0, shape)
    elif stat == "signed":
        f = rng.standard_normal(shape) * 1000
    elif stat == "tiny":  # +-[1e-36, 1e-30], products with the weights go subnormal
        f = rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-36, -30, shape)
    elif stat == "levels":  # two levels per channel more than value_range apart: t clamps to N
        f = np.where(rng.random(shape) < 0.5, 1.0, 100.0) + rng.uniform(0.0, 0.5, shape)
    elif stat == "huge":  # +-3e38 among moderate values: a difference or the sum of two overflows to +Inf
        f = rng.uniform(-5.0, 5.0, shape)
        f[rng.random(shape) < 0.1] = 3e38
        f[rng.random(shape) < 0.1] = -3e38
        f[1::3, ::4, :2], f[1::3, 1::4, :2] = 2e38, 0.0  # two finite differences of 2e38 whose sum overflows
    elif stat == "ends":  # multiples of 2^-7 in [0, 8]: with value_range 8 ch (scale 128 / ch) ...
        f = rng.integers(0, 1025, shape) / 128.0
        f[::5, ::7], f[::5, 1::7] = 0.0, 8.0  # ... neighbours at distance 8 ch exactly: t = N
    else:
        assert stat == "integer"
        f = rng.integers(0, 256, shape)
    f = np.ascontiguousarray(f, dtype=np.float32)
    f.setflags(write=False)
    return f


# (sigma_space, sigma_color, value_range per channel) per statistic, as tests/test_gpu_bilateral_f32.py; the
# value_range passed is C times the last (the L1 distance over C channels), except "integer" (1024: bin width 1)
PARAMS = {
    "depth": (10.0, 3.0, 9.5), "signed": (10.0, 1500.0, 8000.0), "tiny": (0.5, 1e-15, 2e-30),
    "levels": (10.0, 5.0, 20.0), "huge": (10.0, 3.0, 10.0), "ends": (10.0, 3.0, 8.0),
    "integer": (10.0, 30.0, 1024.0),
}


def _params(ch, stat, vr=None):
    ss, sc, per = PARAMS[stat]
    if vr is None:
        vr = per if stat == "integer" else per * ch
    return ss, sc, vr


@functools.lru_cache(maxsize=None)
def _want(w, h, ch, k, profile, stat="depth", vr=None):
    out = bc.bilateral(_source(w, h, ch, stat), k, *_params(ch, stat, vr), profile)
    out.setflags(write=False)
    return out


def _impl(w, h, ch, k, numerics, stat="depth", vr=None):
    return _BilateralF32Impl(w, h, k, *_params(ch, stat, vr), numerics)


def _run(dev, f, impl):
    h, w, ch = f.shape
    d_dst = dev.put(np.full((h, w, ch), SENTINEL, np.uint32).view(np.float32))
    impl.bilateral_filter_c(dev.put(f.copy()), ch, d_dst)  # f is read-only: torch wants a writable array
    return dev.get(d_dst)


def _check(dev, w, h, ch, k, numerics, profile, stat="depth", vr=None):
    launched_kernels()
    got = _run(dev, _source(w, h, ch, stat), _impl(w, h, ch, k, numerics, stat, vr=vr))
    names = launched_kernels()
    assert names in ([_kernel(ch, k, numerics)], ["void " + _kernel(ch, k, numerics)]), names
    want = _want(w, h, ch, k, profile, stat, vr=vr)
    assert np.array_equal(_bits(got), _bits(want)), (w, h, ch, k, stat, _mismatch(got, want))


# ---- every ksize on 37 x 23, the launched instantiation asserted ----
@pytest.mark.parametrize("k", range(1, 16, 2))
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_every_ksize(dev, ch, k, numerics, profile):
    _check(dev, 37, 23, ch, k, numerics, profile)


# ---- ragged frames: one pixel, a few, one pixel over a tile each way, three tile columns ----
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (129, 65), (259, 70)])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ragged_frames(dev, w, h, ch, k, numerics, profile):
    _check(dev, w, h, ch, k, numerics, profile)


# ---- source statistics ----
@pytest.mark.parametrize("stat", ["depth", "signed", "tiny", "levels", "huge"])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_source_statistics(dev, stat, ch, numerics, profile):
    """tiny: gradual underflow (denormal mode 3) is part of the definition. levels: distances past
    value_range, t clamps to N. huge: a difference (3e38 - -3e38) and a sum of two finite differences
    (2e38 + 2e38) overflow to +Inf, which clamps as well."""
    w, h = 67, 33
    f = _source(w, h, ch, stat)
    scale = bo.scale_of(_params(ch, stat)[2])
    with np.errstate(over="ignore"):
        diff = np.abs(f[:, 1:] - f[:, :-1])
        d = (diff[..., 0] + diff[..., 1]).astype(np.float32)
        if ch == 3:
            d = (d + diff[..., 2]).astype(np.float32)
        t = d * scale
    if stat == "levels":
        assert (t > bo.BINS).mean() > 0.3 and (t < bo.BINS).mean() > 0.1
    if stat == "huge":
        assert np.isfinite(f).all() and np.isinf(diff).any() and (np.isinf(d) & np.isfinite(diff).all(axis=2)).any()
    _check(dev, w, h, ch, 9, numerics, profile, stat)


# ---- table ends: value_range 8 C on multiples of 2^-7 puts distances exactly on t = N (and every t on a
# multiple of 1 / C); value_range 8 C (1 + 2^-20) puts the same distances just below it ----
@pytest.mark.parametrize("over", [0.0, 2.0 ** -20])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_table_ends(dev, over, ch, numerics, profile):
    w, h = 67, 33
    vr = 8.0 * ch * (1 + over)
    f = _source(w, h, ch, "ends")
    t = np.abs(f[:, 1:] - f[:, :-1]).sum(axis=2, dtype=np.float32) * bo.scale_of(vr)
    if over == 0:
        assert (t == bo.BINS).any() and (t <= bo.BINS).all()
    else:
        assert (t < bo.BINS).all() and (t > bo.BINS - 1).any()
    _check(dev, w, h, ch, 9, numerics, profile, "ends", vr=vr)


# ---- pitch and alignment, through the C ABI ----
def _pitched(dev, a, pitch, offset):
    """Device buffer holding the rows of `a` (2-D bytes) at `offset` + r * pitch; (tensor, address)."""
    rows, rowbytes = a.shape
    host = np.full(offset + rows * pitch + 16, 0x5A, np.uint8)
    for r in range(rows):
        host[offset + r * pitch: offset + r * pitch + rowbytes] = a[r]
    t = dev.put(host)
    return t, t.data_ptr() + offset


# (offset, padding floats) of source and destination on a 131-pixel row (131 C floats: 16-byte multiples
# only with C = 3 padded by 3): dense; base and pitch multiples of 16; multiples of 4 only (base offset 4)
@pytest.mark.parametrize("off,pad", [(0, 0), (0, "to16"), (4, "to16"), (0, 5)])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment(dev, ch, k, off, pad, numerics, profile):
    w, h = 131, 70
    row = w * ch
    pf = row + (-row % 4 + 4 if pad == "to16" else pad)  # pitch in floats
    assert (pf % 4 == 0) == (pad == "to16") and pf >= row
    f = _source(w, h, ch, "depth")
    impl = _impl(w, h, ch, k, numerics)
    t_src, p_src = _pitched(dev, f.view(np.uint8).reshape(h, 4 * row), 4 * pf, off)
    words = off // 4 + h * pf + 4
    d_dst = dev.put(np.full(words, SENTINEL, np.uint32).view(np.int32))
    assert t_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    rc = _lib.lib().vip_bilateral_f32_run_c(impl._h, p_src, 4 * pf, ch, d_dst.data_ptr() + off, 4 * pf, None)
    assert rc == 0, rc
    raw = dev.get(d_dst).view(np.uint32)
    body = raw[off // 4: off // 4 + h * pf].reshape(h, pf)
    want = _want(w, h, ch, k, profile).reshape(h, row)
    assert np.array_equal(body[:, :row], _bits(want)), _mismatch(body[:, :row].view(np.float32), want)
    assert (body[:, row:] == SENTINEL).all()  # the row padding is the caller's
    assert (raw[:off // 4] == SENTINEL).all() and (raw[off // 4 + h * pf:] == SENTINEL).all()
    del t_src


# ---- a row band on 129 x 200: rows 6..190 with neighbours clamped to [5, 195) ----
@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_row_band(dev, ch, k, numerics, profile):
    w, h = 129, 200
    out_rows, src_row0, row_lo, row_hi = 185, 6, 5, 195
    f = _source(w, h, ch, "depth")
    impl = _impl(w, h, ch, k, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w, ch), SENTINEL, np.uint32).view(np.float32))
    impl.run_rows_c(dev.put(f.copy()), ch, d_dst, out_rows, src_row0, row_lo, row_hi)
    out = dev.get(d_dst)
    want = bc.bilateral_rows(f, out_rows, src_row0, row_lo, row_hi, k, *_params(ch, "depth"), profile)
    assert np.array_equal(_bits(out[:out_rows]), _bits(want)), _mismatch(out[:out_rows], want)
    assert (_bits(out[out_rows:]) == SENTINEL).all()  # rows past out_rows are untouched


# ---- identity 1 on the device: the tie to the 8-bit colour filter ----
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_integer_source_rounds_to_the_u8_colour_filter(dev, numerics, profile):
    """value_range 1024, f = float32(g): u8(dst + 0.5f) is vip_bilateral_run run on the same device."""
    w, h, k = 259, 70, 9
    f = _source(w, h, 3, "integer")
    u8 = _BilateralImpl(w, h, k, 10.0, 30.0, numerics)
    d_u8 = dev.empty((h, w, 3))
    u8.bilateral_filter(dev.put(f.astype(np.uint8)), d_u8)
    got = f2u8(_run(dev, f, _impl(w, h, 3, k, numerics, "integer")) + np.float32(0.5))
    assert np.array_equal(got, dev.get(d_u8)), np.argwhere(got != dev.get(d_u8))[:5].tolist()


# ---- identity 2 on the device: the tie to the one-channel filter ----
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_constant_other_channels_give_the_one_channel_filter(dev, ch, numerics, profile):
    w, h, k = 259, 70, 9
    f = np.empty((h, w, ch), np.float32)
    f[..., 0] = _source(w, h, ch, "depth")[..., 0]
    f[..., 1] = np.float32(-3.25)
    if ch == 3:
        f[..., 2] = np.float32(1e30)
    impl = _BilateralF32Impl(w, h, k, 10.0, 3.0, 9.5, numerics)
    d_one = dev.put(np.full((h, w), SENTINEL, np.uint32).view(np.float32))
    impl.bilateral_filter(dev.put(np.ascontiguousarray(f[..., 0])), d_one)
    got = _run(dev, f, impl)
    one = dev.get(d_one)
    assert np.array_equal(_bits(got[..., 0]), _bits(one)), _mismatch(got[..., 0], one)


# ---- channels = 1 is the one-channel entry point ----
@pytest.mark.parametrize("k", [9, 31])
def test_one_channel_forwards(dev, k):
    w, h = 67, 33
    f = np.ascontiguousarray(_source(w, h, 2, "depth")[..., 0])
    impl = _BilateralF32Impl(w, h, k, 10.0, 3.0, 9.5)
    d_src = dev.put(f)
    d_a = dev.put(np.full((h, w), SENTINEL, np.uint32).view(np.float32))
    d_b = dev.put(np.full((h + 1, w), SENTINEL, np.uint32).view(np.float32))
    for call in (lambda: impl.bilateral_filter_c(d_src, 1, d_a), lambda: impl.run_rows_c(d_src, 1, d_b, h, 0, 0, h)):
        launched_kernels()  # the log holds each distinct kernel since it was last read
        call()
        names = launched_kernels()
        assert len(names) == 1 and f"vip::bilateral_f32_kernel<{k // 2}, true>" in names[0], names
    want = bo.bilateral(f, k, 10.0, 3.0, 9.5, 0)
    assert np.array_equal(_bits(dev.get(d_a)), _bits(want))
    assert np.array_equal(_bits(dev.get(d_b)[:h]), _bits(want)) and (_bits(dev.get(d_b)[h:]) == SENTINEL).all()
    assert _lib.lib().vip_bilateral_f32_max_ksize_c(1) == 31


# ---- later rounds of the persistent loop (this kernel's own copy of it) ----
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


@pytest.mark.parametrize("kind", ["tall", "wide"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_rounds(dev, cus, kind, ch, k, numerics, profile):
    w, h = _frame(kind, cus, tile_rows(ch, k // 2))
    f = _source(w, h, ch, "depth")
    args = (k, *_params(ch, "depth"), profile)
    launched_kernels()
    got = _run(dev, f, _impl(w, h, ch, k, numerics))
    names = launched_kernels()
    assert len(names) == 1 and _kernel(ch, k, numerics) in names[0], names
    want = rs.in_bands(lambda p: bc.bilateral(p, *args), k // 2, f, threads=16)
    assert np.array_equal(_bits(got), _bits(want)), (kind, w, h, ch, k, _mismatch(got, want))


@pytest.mark.parametrize("ch", CHANNELS)
def test_rounds_band(dev, cus, ch):
    """One band on the tall frame: it lies one row inside [row_lo, row_hi), narrower than the frame
    at both ends, and is more than two rounds tall."""
    numerics, profile = PROFILES[1]
    k = 5
    th = tile_rows(ch, k // 2)
    h, row_lo, row_hi, src_row0, out_rows = rs.band(cus, th)
    w = rs.tall(cus, th)[0]
    tiles, full, last = rs.rounds(w, out_rows, th, cus)
    assert full >= 2 and 0 < last < cus and 0 < out_rows % th < th, (tiles, full, last)
    f = _source(w, h, ch, "depth")
    args = (k, *_params(ch, "depth"), profile)
    impl = _impl(w, h, ch, k, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w, ch), SENTINEL, np.uint32).view(np.float32))
    impl.run_rows_c(dev.put(f.copy()), ch, d_dst, out_rows, src_row0, row_lo, row_hi)
    out = dev.get(d_dst)
    crop = np.ascontiguousarray(f[row_lo:row_hi])
    want = rs.in_bands(lambda p: bc.bilateral(p, *args), k // 2, crop, threads=16)
    want = want[src_row0 - row_lo:src_row0 - row_lo + out_rows]
    assert np.array_equal(_bits(out[:out_rows]), _bits(want)), _mismatch(out[:out_rows], want)
    assert (_bits(out[out_rows:]) == SENTINEL).all()


# ---- non-finite input: values only; the kernel's index clamp keeps every table read inside the table ----
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_non_finite_input_stays_local(dev, ch, numerics, profile):
    """A NaN, a +Inf and a -Inf, each in a different channel (C = 2: channels 0, 1, 0), in a 129 x 65
    frame at ksize 9: every output farther than the radius from all three equals the oracle of the
    clean frame; nothing is asserted about the others."""
    w, h, k = 129, 65, 9
    clean = _source(w, h, ch, "depth")
    f = clean.copy()
    spots = [(10, 20), (40, 100), (63, 127)]
    for c, ((y, x), v) in enumerate(zip(spots, (np.nan, np.inf, -np.inf))):
        f[y, x, c % ch] = v
    got = _run(dev, f, _impl(w, h, ch, k, numerics))
    yy, xx = np.mgrid[0:h, 0:w]
    far = np.ones((h, w), bool)
    for y, x in spots:
        far &= (np.abs(yy - y) > k // 2) | (np.abs(xx - x) > k // 2)
    want = _want(w, h, ch, k, profile)
    assert far.sum() > h * w - 3 * k * k
    assert np.array_equal(_bits(got)[far], _bits(want)[far]), _mismatch(got[far], want[far])


# ---- argument errors: the C ABI's codes, without a launch ----
def test_argument_errors(dev):
    w, h, ch = 16, 8, 3
    impl = _BilateralF32Impl(w, h, 5, 10.0, 3.0, 10.0)
    d_src, d_dst = dev.put(np.zeros((h + 1, w, ch), np.float32)), dev.empty((h + 1, w, ch), np.float32)
    s, d, p = d_src.data_ptr(), d_dst.data_ptr(), 4 * w * ch
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING
    run, rows = L.vip_bilateral_f32_run_c, L.vip_bilateral_f32_run_rows_c
    launched_kernels()
    for bad in (0, 4, -1, 5):  # 4 channels are deliberately not offered
        assert run(impl._h, s, p, bad, d, p, None) == INV, bad
        assert rows(impl._h, s, p, bad, d, p, h, 0, 0, h, None) == INV, bad
    for c in (1, 2, 3):
        assert run(None, s, p, c, d, p, None) == INV
        assert rows(None, s, p, c, d, p, h, 0, 0, h, None) == INV
        assert run(impl._h, None, p, c, d, p, None) == INV
        assert run(impl._h, s, p, c, None, p, None) == INV
        for off in (1, 2, 3):  # bases and pitches must be multiples of 4
            assert run(impl._h, s + off, p, c, d, p, None) == INV
            assert run(impl._h, s, p, c, d + off, p, None) == INV
            assert run(impl._h, s, p + off, c, d, p, None) == INV
            assert run(impl._h, s, p, c, d, p + off, None) == INV
        for band in ((h, 0, 4, 4), (h, 0, -1, h), (h, 0, 0, h + 1), (-1, 0, 0, h)):  # out_rows, src_row0, lo, hi
            assert rows(impl._h, s, p, c, d, p, *band, None) == INV, (c, band)
        assert run(impl._h, s, p, c, s, p, None) == AL
    for c in (2, 3):  # a pitch smaller than a row of width * channels floats
        assert run(impl._h, s, 4 * w * c - 4, c, d, p, None) == INV
        assert run(impl._h, s, p, c, d, 4 * w * c - 4, None) == INV
    big = _BilateralF32Impl(w, h, 17, 10.0, 3.0, 10.0)  # fine for one channel, above the cap for 2 and 3
    assert run(big._h, s, p, 3, d, p, None) == KS and run(big._h, s, p, 2, d, p, None) == KS
    assert rows(big._h, s, p, 3, d, p, h, 0, 0, h, None) == KS
    assert launched_kernels() == []  # none of them launched
    assert run(big._h, s, p, 1, d, p, None) == 0
    assert run(impl._h, s + 4, p, 3, d + 4, p, None) == 0  # any multiple of 4 works
    assert len(launched_kernels()) == 2
    dev.torch_.cuda.synchronize()
    assert [L.vip_bilateral_f32_max_ksize_c(c) for c in (-1, 0, 1, 2, 3, 4, 5)] == [0, 0, 31, 15, 15, 0, 0]

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    flt = vip.CudaBilateralFilterF32(w, h, 5, 10.0, 3.0, 10.0)
    assert code(flt.bilateral_filter_c, d_src, 3, d_src) == AL
    assert code(flt.bilateral_filter_c, d_src, 4, d_dst) == INV
    assert code(impl.run_rows_c, d_src, 3, d_dst, h, 0, 4, 4) == INV
    assert code(vip.CudaBilateralFilterF32(w, h, 17).bilateral_filter_c, d_src, 3, d_dst) == KS
    with pytest.raises(ValueError):  # float32, width * height * channels * 4 bytes
        flt.bilateral_filter_c(d_src, 3, dev.empty((h, w), np.float32))
    with pytest.raises(ValueError):
        flt.bilateral_filter_c(dev.put(np.zeros((h, w, 3), np.uint8)), 3, d_dst)


# ---- launch log and kernel timing see the kernel ----
@pytest.mark.parametrize("ch,k", [(2, 1), (3, 9)])
def test_launch_log_and_timing(dev, ch, k):
    impl = _impl(67, 33, ch, k, vip.VIP_NUMERICS_CUDA)
    d_src, d_dst = dev.put(_source(67, 33, ch, "depth").copy()), dev.empty((33, 67, ch), np.float32)
    launched_kernels()
    impl.bilateral_filter_c(d_src, ch, d_dst)
    names = launched_kernels()
    assert len(names) == 1 and _kernel(ch, k, vip.VIP_NUMERICS_CUDA) in names[0], names
    with kernel_timing(1) as kt:
        impl.bilateral_filter_c(d_src, ch, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "bilateral_f32c_k" in rec[0][0] and rec[0][1] > 0, rec
