"""GPU parity of the single-channel (8-bit gray) adaptive bilateral filter
(csrc/vip_gray_adaptive.hip; include/vip.h vip_adaptive_run_c1 and vip_adaptive_run_rows_c1).

Bar: every output equals tests/gray_adaptive_oracle.py (the embedding (g, 0, 0) over the
3-channel adaptive oracle) bit for bit, in both numerics profiles and under both kernel
selections: the radius-specialised vip::gray_adaptive_kernel (128 x 64 tiles, radius 1..15) and
the runtime-radius vip::gray_adaptive_rt_kernel (64 x 64 tiles; radius 0 and 16..31, or every
radius under VIP_PATH_RUNTIME).
Frames of more tiles than the device has CUs (gray_adaptive_kernel's later rounds): tests/test_gpu_c1_rounds.py.
"""
import functools

import numpy as np
import pytest

import gray_adaptive_oracle as gao
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _AdaptiveImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
PATHS = [vip.VIP_PATH_AUTO, vip.VIP_PATH_RUNTIME]
SENTINEL = 0xA5


def _mismatch(a, b):
    d = np.argwhere(a != b)
    return f"{len(d)} mismatches, first {d[:5].tolist()}"


@pytest.fixture
def path(request):
    vip.set_stencil_path(request.param)
    yield request.param
    vip.set_stencil_path(vip.VIP_PATH_AUTO)


# ---- oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _want(w, h, k, profile, ss=10.0, sc=30.0, stat="uniform"):
    out = gao.adaptive(gao.frame(w, h, stat), k, ss, sc, profile, threads=8 if k > 31 else 1)
    out.setflags(write=False)
    return out


def _put(dev, a):
    return dev.put(np.array(a))  # a writable copy: the shared frames are read-only


def _check(dev, w, h, k, numerics, profile, ss=10.0, sc=30.0, stat="uniform"):
    impl = _AdaptiveImpl(w, h, k, ss, sc, numerics)
    d_dst = dev.empty((h, w))
    impl.execute_c1(_put(dev, gao.frame(w, h, stat)), d_dst)
    got = dev.get(d_dst)
    want = _want(w, h, k, profile, ss, sc, stat)
    assert np.array_equal(got, want), (w, h, k, _mismatch(got, want))


# ---- ksize sweep on 131 x 70: crosses the seams of 64- and 128-pixel tiles both ways. The
# separable box sums serve every specialised radius (1..15), so their bound is the one between
# the two kernels: 31 | 33; 17 and 19 stay from the sweep the issue lists ----
@pytest.mark.parametrize("k", [1, 3, 5, 15, 17, 19, 31, 33])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_sweep(dev, path, k, numerics, profile):
    _check(dev, 131, 70, k, numerics, profile)


# the largest ksize; AUTO only (RUNTIME would run the same kernel again)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_63(dev, numerics, profile):
    vip.set_stencil_path(vip.VIP_PATH_AUTO)
    _check(dev, 131, 70, 63, numerics, profile)


# every specialised radius is its own instantiation; AUTO only (RUNTIME never launches them)
@pytest.mark.parametrize("radius", range(1, 16))
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_every_specialised_radius(dev, radius, numerics, profile):
    vip.set_stencil_path(vip.VIP_PATH_AUTO)
    _check(dev, 67, 33, 2 * radius + 1, numerics, profile)


# ---- shapes: tiny frames, and one pixel either side of both kernels' tile widths (128, 64)
# and one row either side of their tile height (64) ----
SHAPES = [(1, 1), (2, 3), (3, 1), (64, 64), (67, 5), (127, 3), (129, 3), (63, 3), (65, 3), (9, 63), (9, 65)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_shapes(dev, path, w, h, k, numerics, profile):
    _check(dev, w, h, k, numerics, profile)


# ---- sigmas: the default; a LUT that is zero from d = 25; one that is non-zero up to 510;
# only d = 0 (most windows then have sumk = 0) ----
@pytest.mark.parametrize("ss,sc", [(10.0, 30.0), (4.0, 3.0 ** 0.5), (1.5, 200.0), (0.3, 0.1)])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_sigmas(dev, path, ss, sc, numerics, profile):
    _check(dev, 67, 33, 9, numerics, profile, ss, sc)


# ---- input statistics, each also under a LUT that is non-zero up to 510, so that a wrong
# high index shows ----
@pytest.mark.parametrize("stat", gao.STATS)
@pytest.mark.parametrize("ss,sc", [(10.0, 30.0), (1.5, 200.0)])
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_input_statistics(dev, path, stat, ss, sc, numerics, profile):
    _check(dev, 67, 33, 9, numerics, profile, ss, sc, stat)


# ---- pitch and alignment, through the C ABI ----
def _rows_c1(h, src, sp, dst, dp, out_rows, src_row0, row_lo, row_hi):
    return _lib.lib().vip_adaptive_run_rows_c1(h, src, sp, dst, dp, out_rows, src_row0, row_lo, row_hi, None)


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
    impl = _AdaptiveImpl(w, h, k, numerics=numerics)
    t_src, p_src = _pitched(dev, gao.frame(w, h), w + 3, 1)  # base + 1 byte, pitch w + 3
    d_dst = dev.put(np.full((h, dst_pitch), SENTINEL, np.uint8))
    rc = _rows_c1(impl._h, p_src, w + 3, d_dst.data_ptr(), dst_pitch, h, 0, 0, h)
    assert rc == 0, rc
    out = dev.get(d_dst)
    want = _want(w, h, k, profile)
    assert np.array_equal(out[:, :w], want), _mismatch(out[:, :w], want)
    assert (out[:, w:] == SENTINEL).all()  # the row padding is the caller's
    del t_src


# ---- row bands (131 x 70, ksize 15) ----
@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_bands_concatenate_to_the_frame(dev, path, numerics, profile):
    w, h, k = 131, 70, 15
    impl = _AdaptiveImpl(w, h, k, numerics=numerics)
    d_src = _put(dev, gao.frame(w, h))
    parts = []
    for r0, r1 in ((0, 23), (23, 24), (24, 70)):
        d_dst = dev.put(np.full((r1 - r0 + 2, w), SENTINEL, np.uint8))
        impl.run_rows_c1(d_src, d_dst, r1 - r0, r0, 0, h)
        out = dev.get(d_dst)
        assert (out[r1 - r0:] == SENTINEL).all()  # rows past out_rows are untouched
        parts.append(out[:r1 - r0])
    got = np.concatenate(parts)
    want = _want(w, h, k, profile)
    assert np.array_equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_band_clamps_to_its_row_range(dev, path, numerics, profile):
    """row_lo = 10, row_hi = 50: the band is the filter of rows 10..49 alone."""
    w, h, k = 131, 70, 15
    g = gao.frame(w, h)
    impl = _AdaptiveImpl(w, h, k, numerics=numerics)
    d_dst = dev.put(np.full((42, w), SENTINEL, np.uint8))
    impl.run_rows_c1(_put(dev, g), d_dst, 40, 10, 10, 50)
    out = dev.get(d_dst)
    want = gao.adaptive(np.ascontiguousarray(g[10:50]), k, profile=profile)
    assert np.array_equal(out[:40], want), _mismatch(out[:40], want)
    assert (out[40:] == SENTINEL).all()


# ---- argument errors: the C ABI's codes, and VipError in Python ----
def test_argument_errors(dev):
    w, h = 16, 8
    impl = _AdaptiveImpl(w, h, 5)
    d_src, d_dst = dev.put(np.zeros((h, w), np.uint8)), dev.empty((h, w))
    s, d = d_src.data_ptr(), d_dst.data_ptr()
    L = _lib.lib()
    INV, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_ALIASING
    assert L.vip_adaptive_run_c1(None, s, w, d, w, None) == INV
    assert L.vip_adaptive_run_c1(impl._h, None, w, d, w, None) == INV
    assert L.vip_adaptive_run_c1(impl._h, s, w, None, w, None) == INV
    assert _rows_c1(None, s, w, d, w, h, 0, 0, h) == INV
    for band in ((h, 0, 4, 4), (h, 0, -1, h), (h, 0, 0, h + 1), (-1, 0, 0, h)):  # out_rows, src_row0, lo, hi
        assert _rows_c1(impl._h, s, w, d, w, *band) == INV, band
    assert L.vip_adaptive_run_c1(impl._h, s, w, s, w, None) == AL
    assert _rows_c1(impl._h, s, w, s, w, h, 0, 0, h) == AL
    assert L.vip_adaptive_run_c1(impl._h, s, w, d, w, None) == 0
    dev.torch_.cuda.synchronize()

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    f = vip.CudaAdaptiveBilateralFilter(w, h, 5)
    assert code(f.execute_c1, d_src, d_src) == AL
    assert code(impl.execute_c1, d_src, d_src) == AL
    assert code(impl.run_rows_c1, d_src, d_dst, h, 0, 4, 4) == INV
    short = dev.empty((h - 1, w))
    with pytest.raises(ValueError):  # d_dst needs width * height bytes
        f.execute_c1(d_src, short)
    with pytest.raises(ValueError):
        impl.run_rows_c1(short, d_dst, h, 0, 0, h)


# ---- launch log and kernel timing see the gray adaptive kernels ----
@pytest.mark.parametrize("k", [9, 33])
def test_launch_log_and_timing(dev, k):
    vip.set_stencil_path(vip.VIP_PATH_AUTO)
    impl = _AdaptiveImpl(67, 33, k)
    d_src, d_dst = _put(dev, gao.frame(67, 33)), dev.empty((33, 67))
    launched_kernels()
    impl.execute_c1(d_src, d_dst)
    names = launched_kernels()
    want = "gray_adaptive_kernel<4, " if k == 9 else "gray_adaptive_rt_kernel<"
    assert len(names) == 1 and want in names[0], names
    with kernel_timing(1) as kt:
        impl.execute_c1(d_src, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "gray_adaptive" in rec[0][0] and rec[0][1] > 0, rec
    got = dev.get(d_dst)
    assert np.array_equal(got, _want(67, 33, k, 0)), _mismatch(got, _want(67, 33, k, 0))
