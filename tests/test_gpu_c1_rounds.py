"""GPU parity of the persistent one-channel kernels past one tile per workgroup: vip::gray_kernel,
gray_adaptive_kernel, joint_f32_kernel, joint_conf_f32_kernel and upsample_f32_kernel on frames of
more tiles than the device has CUs (tests/round_shapes.py: tall() -- two full rounds and a partial
third in one tile column, every vector path off; wide() -- one full round and a partial second
over three tile columns, every vector path on).

The sibling files (test_gpu_gray*.py, test_gpu_joint_f32.py, test_gpu_joint_conf.py,
test_gpu_upsample.py) stay below one round, where the tile loop (csrc/vip_gray.hip:64-111 and its
four copies) leaves at its first `break`: the in-loop prefetch, the commit over planes other waves
have just read, the two barriers, xcd_tile's map in a later round and its identity map in a
partial last one, and the row skip on a prefetched tile run only here.

Bar: the siblings'. Every output equals the family's oracle bit for bit over the whole frame (the
float outputs compared as uint32). Each test asserts rounds() for its own shape before it
launches, and the launched kernel's name after. The inputs are the siblings' generators.
"""
import functools

import numpy as np
import pytest

import conf_oracle as co
import f32_oracle
import gray_adaptive_oracle as gao
import gray_oracle
import round_shapes as rs
import upsample_oracle as uo
import various_image_processings_amd as vip
from various_image_processings_amd.filters import _AdaptiveImpl, _BilateralImpl, _UpsampleImpl, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
HOLE = -1.0
SENTINEL = 0xA5
SENTINEL32 = 0xA5A5A5A5
THREADS = 8  # the oracles' row bands (oracle.bilateral / adaptive threads=, round_shapes.in_bands)


def _alternate(cases):
    """The wide cases: one profile each, CUDA / CPP alternating down the table (the CPU oracles of
    a 1.5 Mpx frame are what this file costs)."""
    return [pytest.param(*c, *PROFILES[i % 2], id="-".join(map(str, c)) + ("-cuda" if i % 2 == 0 else "-cpp"))
            for i, c in enumerate(cases)]


@pytest.fixture(scope="module")
def cus(dev):
    """The number csrc/vip_launch.hpp device_cus() reads."""
    return int(dev.torch_.cuda.get_device_properties(0).multi_processor_count)


def _frame(kind, cus, th):
    """(w, h) of the tall or wide frame, with its rounds asserted."""
    w, h = {"tall": rs.tall, "wide": rs.wide}[kind](cus, th)
    tiles, full, last = rs.rounds(w, h, th, cus)
    assert tiles > cus and full >= (2 if kind == "tall" else 1) and 0 < last < cus, (kind, w, h, tiles, full, last)
    assert 0 < h % th < th
    return w, h


def _one_kernel(want):
    names = launched_kernels()
    assert names and all(want in n for n in names), (want, names)


def _fma(numerics):
    return "true" if numerics == vip.VIP_NUMERICS_CUDA else "false"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mismatch(a, b):
    d = np.argwhere(a != b)
    return f"{len(d)} mismatches of {a.size}, first {d[:5].tolist()}, rows {d[:, 0].min()}..{d[:, 0].max()}"


def _equal(got, want, tag):
    if got.dtype == np.float32:
        got, want = _bits(got), _bits(want)
    assert got.shape == want.shape and np.array_equal(got, want), (tag, _mismatch(got, want))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _gch(guide):
    return 1 if guide.ndim == 2 else 3


# ---- inputs and their oracle outputs: computed once per case, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _gray_frames(w, h):
    """tests/test_gpu_gray.py _frames: (source, gray guide, 3-channel guide), uniform."""
    rng = np.random.default_rng(1000 * w + h)
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    gg = rng.integers(0, 256, (h, w), dtype=np.uint8)
    g3 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return _ro(g, gg, g3)


def _gray_guide(form, w, h):
    return {"plain": None, "gray": _gray_frames(w, h)[1], "rgb": _gray_frames(w, h)[2]}[form]


@functools.lru_cache(maxsize=None)
def _gray_want(form, w, h, k, profile):
    g, guide = _gray_frames(w, h)[0], _gray_guide(form, w, h)
    if guide is None:
        return _ro(gray_oracle.bilateral(g, k, 10.0, 30.0, profile, threads=THREADS))
    return _ro(gray_oracle.joint_bilateral(g, guide, k, 10.0, 30.0, profile, threads=THREADS))


@functools.lru_cache(maxsize=None)
def _adaptive_want(w, h, k, profile):
    return _ro(gao.adaptive(gao.frame(w, h), k, 10.0, 30.0, profile, threads=THREADS))


@functools.lru_cache(maxsize=None)
def _depth(w, h):
    """tests/test_gpu_joint_f32.py _source(w, h, "depth")."""
    rng = np.random.default_rng(977 * w + 31 * h + len("depth"))
    return _ro(np.ascontiguousarray(rng.uniform(0.5, 10.0, (h, w)), dtype=np.float32))


@functools.lru_cache(maxsize=None)
def _f32_guide(form, w, h):
    rng = np.random.default_rng(1000 * w + h + (7 if form == "rgb" else 0))
    return _ro(rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _f32_want(form, w, h, k, profile):
    return _ro(rs.in_bands(lambda f, g: f32_oracle.joint_bilateral(f, g, k, 10.0, 30.0, profile), k // 2,
                           _depth(w, h), _f32_guide(form, w, h), threads=THREADS))


@functools.lru_cache(maxsize=None)
def _holes(w, h):
    return _ro(co.confidence("holes", w, h))


@functools.lru_cache(maxsize=None)
def _conf_want(form, w, h, k, profile):
    return _ro(*rs.in_bands(lambda f, c, g: co.joint_bilateral_conf(f, c, g, k, 10.0, 30.0, profile, HOLE), k // 2,
                            _depth(w, h), _holes(w, h), _f32_guide(form, w, h), threads=THREADS))


@functools.lru_cache(maxsize=None)
def _up_inputs(form, w, h, s):
    """tests/test_gpu_upsample.py _field(w, h, s) and _guides(form, w, h, s)."""
    lw, lh = uo.low_size(w, h, s)
    rng = np.random.default_rng(977 * w + 31 * h + s + len("depth"))
    f = np.ascontiguousarray(rng.uniform(0.5, 10.0, (lh, lw)), dtype=np.float32)
    rng = np.random.default_rng(1000 * w + h + 17 * s + (7 if form == "rgb" else 0))
    tail = () if form == "gray" else (3,)
    g_lo = rng.integers(0, 256, (lh, lw) + tail, dtype=np.uint8)
    g_hi = rng.integers(0, 256, (h, w) + tail, dtype=np.uint8)
    return _ro(f, g_lo, g_hi)


@functools.lru_cache(maxsize=None)
def _up_want(form, w, h, s, k, profile):
    return _ro(uo.upsample(*_up_inputs(form, w, h, s), s, k, 1.0, 30.0, profile))


def _put(dev, a):
    return dev.put(np.array(a))  # a writable copy: the shared arrays are read-only


def _fresh(dev, h, w, dtype=np.uint8):
    """A destination filled with the sentinel, not an uninitialised one: the allocator hands a freed
    block back, and a tile the kernel never wrote would show an earlier case's correct pixels."""
    if dtype == np.uint8:
        return dev.put(np.full((h, w), SENTINEL, np.uint8))
    return dev.put(np.full((h, w), SENTINEL32, np.uint32).view(np.float32))


# ---- gray plain / joint: vip::gray_kernel<R, GUIDE, FMA>, 64-row tiles ----
def _check_gray(dev, cus, kind, form, k, numerics, profile):
    th = rs.tile_rows("gray_kernel", k // 2, {"plain": 0, "gray": 1, "rgb": 3}[form])
    w, h = _frame(kind, cus, th)
    g, guide = _gray_frames(w, h)[0], _gray_guide(form, w, h)
    impl = _BilateralImpl(w, h, k, 10.0, 30.0, numerics)
    d_dst = _fresh(dev, h, w)
    launched_kernels()
    if guide is None:
        impl.bilateral_filter_c1(_put(dev, g), d_dst)
    else:
        impl.joint_bilateral_filter_c1(_put(dev, g), _put(dev, guide), _gch(guide), d_dst)
    _one_kernel(f"vip::gray_kernel<{k // 2}, {0 if guide is None else _gch(guide)}, {_fma(numerics)}>")
    _equal(dev.get(d_dst), _gray_want(form, w, h, k, profile), (kind, form, w, h, k))


@pytest.mark.parametrize("form,k", [("plain", 5), ("plain", 31), ("gray", 5), ("rgb", 5), ("rgb", 31)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_gray_tall(dev, cus, form, k, numerics, profile):
    _check_gray(dev, cus, "tall", form, k, numerics, profile)


@pytest.mark.parametrize("form,numerics,profile", _alternate([("plain",), ("gray",), ("rgb",)]))
def test_gray_wide(dev, cus, form, numerics, profile):
    _check_gray(dev, cus, "wide", form, 5, numerics, profile)


# ---- gray adaptive: vip::gray_adaptive_kernel<R, FMA>, 64-row tiles ----
def _check_adaptive(dev, cus, kind, k, numerics, profile):
    w, h = _frame(kind, cus, rs.tile_rows("gray_adaptive_kernel", k // 2, 0))
    impl = _AdaptiveImpl(w, h, k, 10.0, 30.0, numerics)
    d_dst = _fresh(dev, h, w)
    launched_kernels()
    impl.execute_c1(_put(dev, gao.frame(w, h)), d_dst)
    _one_kernel(f"vip::gray_adaptive_kernel<{k // 2}, {_fma(numerics)}>")
    _equal(dev.get(d_dst), _adaptive_want(w, h, k, profile), (kind, w, h, k))


@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_gray_adaptive_tall(dev, cus, k, numerics, profile):
    _check_adaptive(dev, cus, "tall", k, numerics, profile)


@pytest.mark.parametrize("numerics,profile", [PROFILES[1]])  # the table's fourth wide row
def test_gray_adaptive_wide(dev, cus, numerics, profile):
    _check_adaptive(dev, cus, "wide", 5, numerics, profile)


# ---- joint f32: vip::joint_f32_kernel<R, GUIDE, FMA>, 64- or 48-row tiles ----
def _check_f32(dev, cus, kind, form, k, th, numerics, profile):
    gch = 1 if form == "gray" else 3
    assert rs.tile_rows("joint_f32_kernel", k // 2, gch) == th
    w, h = _frame(kind, cus, th)
    impl = _BilateralImpl(w, h, k, 10.0, 30.0, numerics)
    d_dst = _fresh(dev, h, w, np.float32)
    launched_kernels()
    impl.joint_bilateral_filter_f32(_put(dev, _depth(w, h)), _put(dev, _f32_guide(form, w, h)), gch, d_dst)
    _one_kernel(f"vip::joint_f32_kernel<{k // 2}, {gch}, {_fma(numerics)}>")
    _equal(dev.get(d_dst), _f32_want(form, w, h, k, profile), (kind, form, w, h, k))


@pytest.mark.parametrize("form,k,th", [("gray", 5, 64), ("gray", 27, 48), ("rgb", 5, 64), ("rgb", 21, 48)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_f32_tall(dev, cus, form, k, th, numerics, profile):
    _check_f32(dev, cus, "tall", form, k, th, numerics, profile)


@pytest.mark.parametrize("form,numerics,profile", _alternate([("gray",), ("rgb",)]))
def test_joint_f32_wide(dev, cus, form, numerics, profile):
    _check_f32(dev, cus, "wide", form, 5, 64, numerics, profile)


# ---- joint conf: vip::joint_conf_f32_kernel<R, GUIDE, FMA>, 64-, 48- or 32-row tiles ----
def _check_conf(dev, cus, kind, form, k, th, numerics, profile):
    """dst and weight against the oracle, and dst again without the weight output."""
    gch = 1 if form == "gray" else 3
    assert rs.tile_rows("joint_conf_f32_kernel", k // 2, gch) == th
    w, h = _frame(kind, cus, th)
    impl = _BilateralImpl(w, h, k, 10.0, 30.0, numerics)
    d_in = _put(dev, _depth(w, h)), _put(dev, _holes(w, h)), _put(dev, _f32_guide(form, w, h))
    d_dst, d_wgt, d_alone = (_fresh(dev, h, w, np.float32) for _ in range(3))
    launched_kernels()
    impl.joint_bilateral_filter_conf_f32(*d_in, gch, d_dst, HOLE, d_wgt)
    impl.joint_bilateral_filter_conf_f32(*d_in, gch, d_alone, HOLE, None)
    _one_kernel(f"vip::joint_conf_f32_kernel<{k // 2}, {gch}, {_fma(numerics)}>")
    want, want_k = _conf_want(form, w, h, k, profile)
    tag = (kind, form, w, h, k)
    _equal(dev.get(d_dst), want, tag + ("dst",))
    _equal(dev.get(d_wgt), want_k, tag + ("weight",))
    _equal(dev.get(d_alone), want, tag + ("dst without d_weight",))


@pytest.mark.parametrize("form,k,th", [("gray", 5, 64), ("gray", 9, 48), ("gray", 21, 32),
                                       ("rgb", 5, 64), ("rgb", 7, 48), ("rgb", 19, 32)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_conf_tall(dev, cus, form, k, th, numerics, profile):
    _check_conf(dev, cus, "tall", form, k, th, numerics, profile)


@pytest.mark.parametrize("form,numerics,profile", _alternate([("gray",), ("rgb",)]))
def test_joint_conf_wide(dev, cus, form, numerics, profile):
    _check_conf(dev, cus, "wide", form, 5, 64, numerics, profile)


# ---- upsample: vip::upsample_f32_kernel<R, S, GUIDE, FMA>, 64-row output tiles ----
def _check_upsample(dev, cus, kind, form, s, k, numerics, profile):
    gch = 1 if form == "gray" else 3
    w, h = _frame(kind, cus, rs.tile_rows("upsample_f32_kernel", k // 2, gch))
    f, g_lo, g_hi = _up_inputs(form, w, h, s)
    impl = _UpsampleImpl(w, h, s, k, 1.0, 30.0, numerics)
    assert (impl.low_width(), impl.low_height()) == uo.low_size(w, h, s) == f.shape[::-1]
    d_dst = _fresh(dev, h, w, np.float32)
    launched_kernels()
    impl.upsample_f32(_put(dev, f), _put(dev, g_lo), _put(dev, g_hi), gch, d_dst)
    _one_kernel(f"vip::upsample_f32_kernel<{k // 2}, {s}, {gch}, {_fma(numerics)}>")
    _equal(dev.get(d_dst), _up_want(form, w, h, s, k, profile), (kind, form, w, h, s, k))


@pytest.mark.parametrize("form", ["gray", "rgb"])
@pytest.mark.parametrize("k", [5, 9])
@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_upsample_tall(dev, cus, numerics, profile, s, k, form):
    _check_upsample(dev, cus, "tall", form, s, k, numerics, profile)


@pytest.mark.parametrize("form,numerics,profile", _alternate([("gray",), ("rgb",)]))
def test_upsample_wide(dev, cus, form, numerics, profile):
    _check_upsample(dev, cus, "wide", form, 4, 5, numerics, profile)


# ---- row bands on the tall frame, ksize 5: the band lies one row inside [row_lo, row_hi), which
# is narrower than the frame at both ends, and is more than two rounds tall; the first tile's
# loads clamp to row_lo and the last tile's, which come through the prefetch, to row_hi - 1 ----
def _band(cus, th):
    h, row_lo, row_hi, src_row0, out_rows = rs.band(cus, th)
    tiles, full, last = rs.rounds(9, out_rows, th, cus)
    assert full >= 2 and 0 < last < cus and 0 < out_rows % th < th, (tiles, full, last)
    assert 0 < row_lo and src_row0 - 2 < row_lo and src_row0 + out_rows + 2 > row_hi and row_hi < h
    return 9, h, row_lo, row_hi, src_row0, out_rows


@pytest.mark.parametrize("form", ["plain", "rgb"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_gray_band(dev, cus, form, numerics, profile):
    """vip_bilateral_run_rows_c1."""
    w, h, row_lo, row_hi, src_row0, out_rows = _band(cus, 64)
    g, guide = _gray_frames(w, h)[0], _gray_guide(form, w, h)
    impl = _BilateralImpl(w, h, 5, 10.0, 30.0, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w), SENTINEL, np.uint8))
    launched_kernels()
    impl.run_rows_c1(_put(dev, g), d_dst, out_rows, src_row0, row_lo, row_hi,
                     d_guide=None if guide is None else _put(dev, guide), guide_channels=3)
    _one_kernel(f"vip::gray_kernel<2, {0 if guide is None else 3}, {_fma(numerics)}>")
    out = dev.get(d_dst)
    want = rs.gray_band(np.ascontiguousarray(g[row_lo:row_hi]),
                        None if guide is None else np.ascontiguousarray(guide[row_lo:row_hi]),
                        src_row0 - row_lo, out_rows, 5, 10.0, 30.0, profile)
    _equal(out[:out_rows], want, (form, w, h))
    assert (out[out_rows:] == SENTINEL).all()  # rows past out_rows are untouched


@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_gray_adaptive_band(dev, cus, numerics, profile):
    """vip_adaptive_run_rows_c1."""
    w, h, row_lo, row_hi, src_row0, out_rows = _band(cus, 64)
    g = gao.frame(w, h)
    impl = _AdaptiveImpl(w, h, 5, 10.0, 30.0, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w), SENTINEL, np.uint8))
    launched_kernels()
    impl.run_rows_c1(_put(dev, g), d_dst, out_rows, src_row0, row_lo, row_hi)
    _one_kernel(f"vip::gray_adaptive_kernel<2, {_fma(numerics)}>")
    out = dev.get(d_dst)
    want = rs.adaptive_band(np.ascontiguousarray(g[row_lo:row_hi]), src_row0 - row_lo, out_rows, 5, 10.0, 30.0, profile)
    _equal(out[:out_rows], want, (w, h))
    assert (out[out_rows:] == SENTINEL).all()


@pytest.mark.parametrize("form", ["gray", "rgb"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_f32_band(dev, cus, form, numerics, profile):
    """vip_joint_bilateral_run_rows_f32; its oracle has no band form: the rows of the filter of
    rows [row_lo, row_hi) alone."""
    w, h, row_lo, row_hi, src_row0, out_rows = _band(cus, 64)
    f, guide = _depth(w, h), _f32_guide(form, w, h)
    impl = _BilateralImpl(w, h, 5, 10.0, 30.0, numerics)
    d_dst = dev.put(np.full((out_rows + 2, w), SENTINEL32, np.uint32).view(np.float32))
    launched_kernels()
    impl.run_rows_f32(_put(dev, f), _put(dev, guide), _gch(guide), d_dst, out_rows, src_row0, row_lo, row_hi)
    _one_kernel(f"vip::joint_f32_kernel<2, {_gch(guide)}, {_fma(numerics)}>")
    out = dev.get(d_dst)
    want = f32_oracle.joint_bilateral(f[row_lo:row_hi], guide[row_lo:row_hi], 5, 10.0, 30.0, profile)
    _equal(out[:out_rows], want[src_row0 - row_lo:src_row0 - row_lo + out_rows], (form, w, h))
    assert (_bits(out[out_rows:]) == SENTINEL32).all()
