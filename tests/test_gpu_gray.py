"""GPU parity of the single-channel (8-bit gray) bilateral / joint-bilateral filters
(csrc/vip_gray.hip; include/vip.h vip_bilateral_run_c1 and friends).

Bar: every output equals tests/gray_oracle.py (the embedding (g, 0, 0) over the 3-channel
oracle) bit for bit, in both numerics profiles and under both kernel selections: the
radius-specialised vip::gray_kernel (128 x 64 tiles, radius 1..15) and the runtime-radius
vip::gray_rt_kernel (64 x 64 tiles; radius 0 and 16..32, or every radius under
VIP_PATH_RUNTIME).
Frames of more tiles than the device has CUs (gray_kernel's later rounds): tests/test_gpu_c1_rounds.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import gray_oracle
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _BilateralImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
PATHS = [vip.VIP_PATH_AUTO, vip.VIP_PATH_RUNTIME]
FORMS = ["plain", "gray", "rgb"]
SENTINEL = 0xA5


def _mismatch(a, b):
    d = np.argwhere(a != b)
    return f"{len(d)} mismatches, first {d[:5].tolist()}"


@pytest.fixture
def path(request):
    vip.set_stencil_path(request.param)
    yield request.param
    vip.set_stencil_path(vip.VIP_PATH_AUTO)


# ---- inputs and their oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _frames(w, h, stat="uniform"):
    """(source, gray guide, 3-channel guide) of a w x h frame."""
    rng = np.random.default_rng(1000 * w + h)
    if stat == "uniform":
        g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif stat == "narrow":
        g = rng.integers(100, 120, (h, w), dtype=np.uint8)
    elif stat == "step":  # two levels (40 | 210) with +-3 noise
        g = np.where(np.arange(w)[None, :] < w // 2, 40, 210) + rng.integers(-3, 4, (h, w))
        g = g.astype(np.uint8)
    else:
        g = np.full((h, w), 255, np.uint8)
    gg = rng.integers(0, 256, (h, w), dtype=np.uint8)
    g3 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return g, gg, g3


def _guide(form, w, h, stat="uniform"):
    g, gg, g3 = _frames(w, h, stat)
    return {"plain": None, "gray": gg, "rgb": g3}[form]


@functools.lru_cache(maxsize=None)
def _want(form, w, h, k, profile, ss=10.0, sc=30.0, stat="uniform"):
    g = _frames(w, h, stat)[0]
    guide = _guide(form, w, h, stat)
    if guide is None:
        out = gray_oracle.bilateral(g, k, ss, sc, profile)
    else:
        out = gray_oracle.joint_bilateral(g, guide, k, ss, sc, profile)
    out.setflags(write=False)
    return out


def _run(dev, g, k, numerics, guide=None, ss=10.0, sc=30.0):
    h, w = g.shape
    impl = _BilateralImpl(w, h, k, ss, sc, numerics)
    d_dst = dev.empty((h, w))
    if guide is None:
        impl.bilateral_filter_c1(dev.put(g), d_dst)
    else:
        impl.joint_bilateral_filter_c1(dev.put(g), dev.put(guide), 1 if guide.ndim == 2 else 3, d_dst)
    return dev.get(d_dst)


def _check(dev, form, w, h, k, numerics, profile, ss=10.0, sc=30.0, stat="uniform"):
    got = _run(dev, _frames(w, h, stat)[0], k, numerics, _guide(form, w, h, stat), ss, sc)
    want = _want(form, w, h, k, profile, ss, sc, stat)
    assert np.array_equal(got, want), (form, w, h, k, _mismatch(got, want))


# ---- ksize sweep on 131 x 70: crosses the seams of 64- and 128-pixel tiles both ways ----
@pytest.mark.parametrize("k", [1, 3, 5, 15, 17, 31, 33, 65])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_plain_ksize_sweep(dev, path, k, numerics, profile):
    _check(dev, "plain", 131, 70, k, numerics, profile)


@pytest.mark.parametrize("form", ["gray", "rgb"])
@pytest.mark.parametrize("k", [1, 5, 15, 17, 47])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_ksize_sweep(dev, path, form, k, numerics, profile):
    _check(dev, form, 131, 70, k, numerics, profile)


# ---- shapes: tiny frames, and one pixel either side of both kernels' tile widths (128, 64)
# and one row either side of their tile height (64) ----
SHAPES = [(1, 1), (2, 3), (3, 1), (64, 64), (67, 5), (127, 3), (129, 3), (63, 3), (65, 3), (9, 63), (9, 65)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_shapes(dev, path, w, h, k, numerics, profile):
    for form in FORMS:
        _check(dev, form, w, h, k, numerics, profile)


# ---- sigmas: the default; a LUT that is zero from d = 25; one never small; only d = 0 ----
@pytest.mark.parametrize("ss,sc", [(10.0, 30.0), (4.0, 3.0 ** 0.5), (1.5, 200.0), (0.3, 0.1)])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_sigmas(dev, path, ss, sc, numerics, profile):
    for form in FORMS:
        _check(dev, form, 67, 33, 9, numerics, profile, ss, sc)


@pytest.mark.parametrize("stat", ["uniform", "narrow", "step", "const255"])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_input_statistics(dev, path, stat, numerics, profile):
    for form in FORMS:
        _check(dev, form, 67, 33, 9, numerics, profile, stat=stat)


# ---- pitch and alignment, through the C ABI ----
def _rows_c1(h, src, sp, guide, gp, gch, dst, dp, out_rows, src_row0, row_lo, row_hi):
    return _lib.lib().vip_bilateral_run_rows_c1(h, src, sp, guide, gp, gch, dst, dp, out_rows, src_row0, row_lo,
                                                row_hi, None)


def _pitched(dev, a, pitch, offset):
    """Device buffer holding rows of `a` (2-D bytes) at `offset` + r * pitch; returns (tensor, address)."""
    rows, rowbytes = a.shape
    host = np.full(offset + rows * pitch + 8, 0x5A, np.uint8)
    for r in range(rows):
        host[offset + r * pitch: offset + r * pitch + rowbytes] = a[r]
    t = dev.put(host)
    return t, t.data_ptr() + offset


# dst pitch w + 5 = 136: rows start word aligned (word stores and a byte tail in the last
# tile column); 139: they do not (byte stores)
@pytest.mark.parametrize("dst_pitch", [131 + 5, 139])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment(dev, path, k, dst_pitch, numerics, profile):
    w, h = 131, 70
    g, gg, g3 = _frames(w, h)
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    t_src, p_src = _pitched(dev, g, w + 3, 1)                       # base + 1 byte, pitch w + 3
    t_gg, p_gg = _pitched(dev, gg, w + 1, 3)
    t_g3, p_g3 = _pitched(dev, g3.reshape(h, 3 * w), 3 * w + 1, 0)  # guide pitch 3w + 1
    for form, pg, gp, gch in (("plain", None, 0, 0), ("gray", p_gg, w + 1, 1), ("rgb", p_g3, 3 * w + 1, 3)):
        d_dst = dev.put(np.full((h, dst_pitch), SENTINEL, np.uint8))
        rc = _rows_c1(impl._h, p_src, w + 3, pg, gp, gch, d_dst.data_ptr(), dst_pitch, h, 0, 0, h)
        assert rc == 0, (form, rc)
        out = dev.get(d_dst)
        want = _want(form, w, h, k, profile)
        assert np.array_equal(out[:, :w], want), (form, _mismatch(out[:, :w], want))
        assert (out[:, w:] == SENTINEL).all(), form  # the row padding is the caller's
    del t_src, t_gg, t_g3


# ---- row bands (131 x 70, ksize 15) ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_bands_concatenate_to_the_frame(dev, path, form, numerics, profile):
    w, h, k = 131, 70, 15
    g = _frames(w, h)[0]
    guide = _guide(form, w, h)
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    d_src = dev.put(g)
    d_guide = None if guide is None else dev.put(guide)
    parts = []
    for r0, r1 in ((0, 23), (23, 24), (24, 70)):
        d_dst = dev.put(np.full((r1 - r0 + 2, w), SENTINEL, np.uint8))
        impl.run_rows_c1(d_src, d_dst, r1 - r0, r0, 0, h, d_guide=d_guide, guide_channels=3 if form == "rgb" else 1)
        out = dev.get(d_dst)
        assert (out[r1 - r0:] == SENTINEL).all()  # rows past out_rows are untouched
        parts.append(out[:r1 - r0])
    got = np.concatenate(parts)
    want = _want(form, w, h, k, profile)
    assert np.array_equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_band_clamps_to_its_row_range(dev, path, form, numerics, profile):
    """row_lo = 10, row_hi = 50: the band is the filter of rows 10..49 alone."""
    w, h, k = 131, 70, 15
    g = _frames(w, h)[0]
    guide = _guide(form, w, h)
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    d_dst = dev.put(np.full((42, w), SENTINEL, np.uint8))
    impl.run_rows_c1(dev.put(g), d_dst, 40, 10, 10, 50, d_guide=None if guide is None else dev.put(guide),
                     guide_channels=3 if form == "rgb" else 1)
    out = dev.get(d_dst)
    crop = np.ascontiguousarray(g[10:50])
    if guide is None:
        want = gray_oracle.bilateral(crop, k, profile=profile)
    else:
        want = gray_oracle.joint_bilateral(crop, np.ascontiguousarray(guide[10:50]), k, profile=profile)
    assert np.array_equal(out[:40], want), _mismatch(out[:40], want)
    assert (out[40:] == SENTINEL).all()


# ---- argument errors: the C ABI's codes, and VipError in Python ----
def test_argument_errors(dev):
    w, h = 16, 8
    impl = _BilateralImpl(w, h, 5)
    big = _BilateralImpl(w, h, 49)  # above the joint filter's largest ksize (47)
    d_src, d_dst = dev.put(np.zeros((h, w), np.uint8)), dev.empty((h, w))
    d_g1, d_g3 = dev.put(np.zeros((h, w), np.uint8)), dev.put(np.zeros((h, w, 3), np.uint8))
    s, d, g1, g3 = d_src.data_ptr(), d_dst.data_ptr(), d_g1.data_ptr(), d_g3.data_ptr()
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING
    assert L.vip_bilateral_run_c1(None, s, w, d, w, None) == INV
    assert L.vip_bilateral_run_c1(impl._h, None, w, d, w, None) == INV
    assert L.vip_bilateral_run_c1(impl._h, s, w, None, w, None) == INV
    assert L.vip_joint_bilateral_run_c1(impl._h, s, w, None, w, 1, d, w, None) == INV
    assert L.vip_joint_bilateral_run_c1(None, s, w, g1, w, 1, d, w, None) == INV
    for gch in (0, 2, 4, -1):
        assert L.vip_joint_bilateral_run_c1(impl._h, s, w, g1, w, gch, d, w, None) == INV
    assert _rows_c1(None, s, w, None, 0, 0, d, w, h, 0, 0, h) == INV
    for band in ((h, 0, 4, 4), (h, 0, -1, h), (h, 0, 0, h + 1), (-1, 0, 0, h)):  # out_rows, src_row0, lo, hi
        assert _rows_c1(impl._h, s, w, None, 0, 0, d, w, *band) == INV, band
    assert L.vip_joint_bilateral_run_c1(big._h, s, w, g1, w, 1, d, w, None) == KS
    assert L.vip_joint_bilateral_run_c1(big._h, s, w, g3, 3 * w, 3, d, w, None) == KS
    assert L.vip_bilateral_run_c1(big._h, s, w, d, w, None) == 0  # the plain filter runs at ksize 49
    assert L.vip_bilateral_run_c1(impl._h, s, w, s, w, None) == AL
    assert L.vip_joint_bilateral_run_c1(impl._h, s, w, g1, w, 1, s, w, None) == AL
    assert L.vip_joint_bilateral_run_c1(impl._h, s, w, g1, w, 1, g1, w, None) == AL
    dev.torch_.cuda.synchronize()

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    f = vip.CudaBilateralFilter(w, h, 5)
    assert code(f.bilateral_filter_c1, d_src, d_src) == AL
    assert code(f.joint_bilateral_filter_c1, d_src, d_g1, 1, d_g1) == AL
    assert code(f.joint_bilateral_filter_c1, d_src, d_g1, 2, d_dst) == INV
    assert code(impl.run_rows_c1, d_src, d_dst, h, 0, 4, 4) == INV
    assert code(big.joint_bilateral_filter_c1, d_src, d_g3, 3, d_dst) == KS
    with pytest.raises(ValueError):  # a 3-channel guide needs width * height * 3 bytes
        f.joint_bilateral_filter_c1(d_src, d_g1, 3, d_dst)


# ---- launch log and kernel timing see the gray kernels ----
@pytest.mark.parametrize("k", [9, 33])
def test_launch_log_and_timing(dev, k):
    g = _frames(67, 33)[0]
    impl = _BilateralImpl(67, 33, k)
    d_src, d_dst = dev.put(g), dev.empty((33, 67))
    launched_kernels()
    impl.bilateral_filter_c1(d_src, d_dst)
    names = launched_kernels()
    assert names and all("gray_" in n for n in names), names
    with kernel_timing(1) as kt:
        impl.bilateral_filter_c1(d_src, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "gray_" in rec[0][0] and rec[0][1] > 0, rec
