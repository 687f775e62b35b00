"""GPU parity of joint bilateral upsampling (csrc/vip_upsample.hip; include/vip.h
vip_upsample_run_f32).

Bar: every output equals tests/upsample_oracle.py bit for bit (compared as uint32), in both
numerics profiles, with a gray and with a 3-channel guide pair, at every scale.
Frames of more tiles than the device has CUs (upsample_f32_kernel's later rounds): tests/test_gpu_c1_rounds.py.
"""
import functools

import numpy as np
import pytest

import upsample_oracle as uo
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _UpsampleImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
FORMS = ["gray", "rgb"]
SENTINEL = 0xA5A5A5A5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mismatch(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    first = [(tuple(i), float(a[tuple(i)]), float(b[tuple(i)])) for i in d[:4]]
    return f"{len(d)} mismatches, first (index, got, want) {first}"


# ---- inputs and their oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _field(w, h, s, stat="depth"):
    lw, lh = uo.low_size(w, h, s)
    rng = np.random.default_rng(977 * w + 31 * h + s + len(stat))
    if stat == "depth":
        f = rng.uniform(0.5, 10.0, (lh, lw))
    elif stat == "signed":
        f = rng.standard_normal((lh, lw)) * 1000
    elif stat == "sparse":  # 70 % exact zeros
        f = np.where(rng.random((lh, lw)) < 0.7, 0.0, rng.uniform(1.0, 2.0, (lh, lw)))
    else:  # tiny: +-[1e-36, 1e-30], products with the weights go subnormal
        assert stat == "tiny"
        f = rng.choice([-1.0, 1.0], (lh, lw)) * 10.0 ** rng.uniform(-36, -30, (lh, lw))
    return np.ascontiguousarray(f, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _guides(form, w, h, s):
    rng = np.random.default_rng(1000 * w + h + 17 * s + (7 if form == "rgb" else 0))
    lw, lh = uo.low_size(w, h, s)
    tail = () if form == "gray" else (3,)
    return rng.integers(0, 256, (lh, lw) + tail, dtype=np.uint8), rng.integers(0, 256, (h, w) + tail, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _want(form, w, h, s, k, profile, ss=1.0, sc=30.0, stat="depth"):
    g_lo, g_hi = _guides(form, w, h, s)
    out = uo.upsample(_field(w, h, s, stat), g_lo, g_hi, s, k, ss, sc, profile)
    out.setflags(write=False)
    return out


def _gch(guide):
    return 1 if guide.ndim == 2 else 3


def _run(dev, f, g_lo, g_hi, s, k, numerics, ss=1.0, sc=30.0):
    h, w = g_hi.shape[:2]
    impl = _UpsampleImpl(w, h, s, k, ss, sc, numerics)
    assert (impl.low_width(), impl.low_height()) == uo.low_size(w, h, s) == f.shape[::-1]
    d_dst = dev.empty((h, w), np.float32)
    impl.upsample_f32(dev.put(f), dev.put(g_lo), dev.put(g_hi), _gch(g_hi), d_dst)
    return dev.get(d_dst)


def _check(dev, form, w, h, s, k, numerics, profile, ss=1.0, sc=30.0, stat="depth"):
    g_lo, g_hi = _guides(form, w, h, s)
    got = _run(dev, _field(w, h, s, stat), g_lo, g_hi, s, k, numerics, ss, sc)
    want = _want(form, w, h, s, k, profile, ss, sc, stat)
    assert np.array_equal(_bits(got), _bits(want)), (form, w, h, s, k, stat, _mismatch(got, want))


# ---- 131 x 70: no multiple of any scale (the ceil cells, both clamps), and it crosses the
# 128-column and 64-row seams of the kernel's tiles ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 3, 5, 7, 9])
@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_scale_ksize_guide(dev, numerics, profile, s, k, form):
    _check(dev, form, 131, 70, s, k, numerics, profile)


# ---- smaller than a tile; a 1 x 1 low-resolution image (every tap clamps to one sample); an
# exact multiple of the scale ----
@pytest.mark.parametrize("w,h,s", [(37, 19, 2), (37, 19, 4), (37, 19, 8), (5, 3, 8), (16, 8, 8), (1, 1, 2)])
@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_small_outputs(dev, numerics, profile, w, h, s, k):
    for form in FORMS:
        _check(dev, form, w, h, s, k, numerics, profile)


# ---- several tiles in each direction, more tiles than one round of a small grid needs ----
@pytest.mark.parametrize("w,h,s", [(389, 70, 4), (131, 197, 2)])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_several_tiles(dev, numerics, profile, w, h, s):
    for form in FORMS:
        _check(dev, form, w, h, s, 5, numerics, profile)


@pytest.mark.parametrize("stat", ["depth", "signed", "tiny", "sparse"])
@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_source_statistics(dev, numerics, profile, s, stat):
    """tiny: gradual underflow (denormal mode 3) is part of the definition."""
    for form in FORMS:
        _check(dev, form, 67, 33, s, 5, numerics, profile, stat=stat)


# ---- the two branches of the epilogue ----
@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_mixed_frame_takes_both_branches(dev, numerics, profile, s):
    w, h = 131, 70
    g_lo, g_hi = _guides("gray", w, h, s)
    f = _field(w, h, s)
    want, zero = uo.upsample(f, g_lo, g_hi, s, 3, 1.0, 3.0, profile, with_fallback=True)
    assert 0 < zero.mean() < 0.5, zero.mean()
    got = _run(dev, f, g_lo, g_hi, s, 3, numerics, 1.0, 3.0)
    assert np.array_equal(_bits(got), _bits(want)), _mismatch(got, want)


@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_all_fallback_returns_the_nearest_sample(dev, numerics, profile, s):
    w, h = 131, 70
    lw, lh = uo.low_size(w, h, s)
    f = _field(w, h, s)
    got = _run(dev, f, np.zeros((lh, lw), np.uint8), np.full((h, w), 255, np.uint8), s, 5, numerics, 1.0, 1.0)
    want = f[(np.arange(h) // s)[:, None], (np.arange(w) // s)[None, :]]
    assert np.array_equal(_bits(got), _bits(want)), _mismatch(got, want)


@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_constant_field_is_reproduced(dev, numerics, profile):
    """What smoke() runs, needing no oracle: products by 2.0 are exact."""
    for s in uo.SCALES:
        g_lo, g_hi = _guides("rgb", 50, 50, s)
        lw, lh = uo.low_size(50, 50, s)
        got = _run(dev, np.full((lh, lw), 2.0, np.float32), g_lo, g_hi, s, 5, numerics, 1.5, 30.0)
        assert (got == np.float32(2.0)).all(), s


# ---- pitch and alignment, through the C ABI ----
def _pitched(dev, a, pitch, offset):
    """Device buffer holding the rows of `a` (2-D bytes) at `offset` + r * pitch; (tensor, address)."""
    rows, rowbytes = a.shape
    host = np.full(offset + rows * pitch + 16, 0x5A, np.uint8)
    for r in range(rows):
        host[offset + r * pitch: offset + r * pitch + rowbytes] = a[r]
    t = dev.put(host)
    return t, t.data_ptr() + offset


# (source offset, source pitch in floats beyond the row, dst offset, dst pitch in floats): a source
# pitch that is a multiple of 4 but not of 16, a dst base offset by 4 bytes, guide bases offset by
# one byte with odd pitches; then every base and pitch a multiple of 16 (float4 loads and stores)
@pytest.mark.parametrize("src_off,src_pad,dst_off,dst_pf", [(4, 1, 0, 134), (0, 1, 4, 134), (0, 0, 0, 136)])
@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment(dev, numerics, profile, s, src_off, src_pad, dst_off, dst_pf):
    w, h, k = 131, 70, 5
    lw, lh = uo.low_size(w, h, s)
    src_pf = lw + src_pad if src_pad else -(-lw // 4) * 4
    assert (4 * src_pf) % 16 != 0 or not src_pad
    impl = _UpsampleImpl(w, h, s, k, 1.0, 30.0, numerics)
    t_src, p_src = _pitched(dev, _field(w, h, s).view(np.uint8).reshape(lh, 4 * lw), 4 * src_pf, src_off)
    assert t_src.data_ptr() % 16 == 0
    for form, gch in (("gray", 1), ("rgb", 3)):
        g_lo, g_hi = _guides(form, w, h, s)
        goff = 1 if dst_pf != 136 else 0                     # the last case: dword-aligned guides
        glp, ghp = gch * lw + goff, gch * w + goff
        if not goff:
            glp, ghp = -(-glp // 4) * 4, -(-ghp // 4) * 4
        t_gl, p_gl = _pitched(dev, g_lo.reshape(lh, gch * lw), glp, goff)
        t_gh, p_gh = _pitched(dev, g_hi.reshape(h, gch * w), ghp, goff)
        words = dst_off // 4 + h * dst_pf + 4
        d_dst = dev.put(np.full(words, SENTINEL, np.uint32).view(np.int32))
        assert d_dst.data_ptr() % 16 == 0
        rc = _lib.lib().vip_upsample_run_f32(impl._h, p_src, 4 * src_pf, p_gl, glp, p_gh, ghp, gch,
                                             d_dst.data_ptr() + dst_off, 4 * dst_pf, None)
        assert rc == 0, (form, rc)
        raw = dev.get(d_dst).view(np.uint32)
        body = raw[dst_off // 4: dst_off // 4 + h * dst_pf].reshape(h, dst_pf)
        want = _want(form, w, h, s, k, profile)
        assert np.array_equal(body[:, :w], _bits(want)), (form, _mismatch(body[:, :w].view(np.float32), want))
        assert (body[:, w:] == SENTINEL).all(), form  # the row padding is the caller's
        assert (raw[:dst_off // 4] == SENTINEL).all() and (raw[dst_off // 4 + h * dst_pf:] == SENTINEL).all(), form
        del t_gl, t_gh
    del t_src


# ---- argument errors: the C ABI's codes, and VipError / ValueError in Python ----
def test_argument_errors(dev):
    import ctypes
    w, h, s = 16, 8, 4
    lw, lh = 4, 2
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING

    def create(*a):
        hnd = ctypes.c_void_p()
        rc = L.vip_upsample_create(ctypes.byref(hnd), *a)
        if rc == 0:
            assert L.vip_upsample_destroy(hnd) == 0
        return rc

    assert create(w, h, s, 5, 1.0, 30.0, 0) == 0
    assert L.vip_upsample_create(None, w, h, s, 5, 1.0, 30.0, 0) == INV
    assert create(0, h, s, 5, 1.0, 30.0, 0) == INV and create(w, -1, s, 5, 1.0, 30.0, 0) == INV
    for bad in (0, 1, 3, 5, 6, 16, -2):
        assert create(w, h, bad, 5, 1.0, 30.0, 0) == INV, bad
    for bad in (0, 2, 4, 8, 11, 13, -1):
        assert create(w, h, s, bad, 1.0, 30.0, 0) == KS, bad
    assert L.vip_upsample_destroy(None) == 0
    assert L.vip_max_ksize(vip.VIP_FILTER_UPSAMPLE) == 9

    a, b = ctypes.c_int(), ctypes.c_int()
    for ww, hh, sc in ((131, 70, 2), (131, 70, 4), (131, 70, 8), (16, 8, 8), (5, 3, 8), (1, 1, 2)):
        assert L.vip_upsample_low_size(ww, hh, sc, ctypes.byref(a), ctypes.byref(b)) == 0
        assert (a.value, b.value) == (-(-ww // sc), -(-hh // sc))
    assert L.vip_upsample_low_size(16, 8, 3, ctypes.byref(a), ctypes.byref(b)) == INV
    assert L.vip_upsample_low_size(0, 8, 2, ctypes.byref(a), ctypes.byref(b)) == INV
    assert L.vip_upsample_low_size(16, 8, 2, None, ctypes.byref(b)) == INV

    impl = _UpsampleImpl(w, h, s, 5)
    d_src = dev.put(np.zeros((lh + 1, lw + 4), np.float32))
    d_dst = dev.empty((h + 1, w + 4), np.float32)
    d_l1, d_l3 = dev.put(np.zeros((lh, lw), np.uint8)), dev.put(np.zeros((lh, lw, 3), np.uint8))
    d_g1, d_g3 = dev.put(np.zeros((h, w), np.uint8)), dev.put(np.zeros((h, w, 3), np.uint8))
    src, dst, l1, l3, g1, g3 = (t.data_ptr() for t in (d_src, d_dst, d_l1, d_l3, d_g1, d_g3))
    sp, dp = 4 * lw, 4 * w
    run = L.vip_upsample_run_f32
    assert run(impl._h, src, sp, l1, lw, g1, w, 1, dst, dp, None) == 0
    assert run(impl._h, src, sp, l3, 3 * lw, g3, 3 * w, 3, dst, dp, None) == 0
    assert run(None, src, sp, l1, lw, g1, w, 1, dst, dp, None) == INV
    assert run(impl._h, None, sp, l1, lw, g1, w, 1, dst, dp, None) == INV
    assert run(impl._h, src, sp, None, lw, g1, w, 1, dst, dp, None) == INV
    assert run(impl._h, src, sp, l1, lw, None, w, 1, dst, dp, None) == INV
    assert run(impl._h, src, sp, l1, lw, g1, w, 1, None, dp, None) == INV
    for off in (1, 2, 3):  # float bases and pitches must be multiples of 4
        assert run(impl._h, src + off, sp, l1, lw, g1, w, 1, dst, dp, None) == INV
        assert run(impl._h, src, sp + off, l1, lw, g1, w, 1, dst, dp, None) == INV
        assert run(impl._h, src, sp, l1, lw, g1, w, 1, dst + off, dp, None) == INV
        assert run(impl._h, src, sp, l1, lw, g1, w, 1, dst, dp + off, None) == INV
    assert run(impl._h, src + 4, sp + 4, l1, lw, g1, w, 1, dst + 4, dp + 4, None) == 0  # any multiple of 4 works
    for gch in (0, 2, 4, -1):
        assert run(impl._h, src, sp, l1, lw, g1, w, gch, dst, dp, None) == INV
    # a pitch smaller than a row
    assert run(impl._h, src, sp - 4, l1, lw, g1, w, 1, dst, dp, None) == INV
    assert run(impl._h, src, sp, l1, lw - 1, g1, w, 1, dst, dp, None) == INV
    assert run(impl._h, src, sp, l1, lw, g1, w - 1, 1, dst, dp, None) == INV
    assert run(impl._h, src, sp, l3, 3 * lw - 1, g3, 3 * w, 3, dst, dp, None) == INV
    assert run(impl._h, src, sp, l3, 3 * lw, g3, 3 * w - 1, 3, dst, dp, None) == INV
    assert run(impl._h, src, sp, l1, lw, g1, w, 1, dst, dp - 4, None) == INV
    assert run(impl._h, src, sp, l1, lw, g1, w, 1, src, dp, None) == AL
    assert run(impl._h, src, sp, dst, lw, g1, w, 1, dst, dp, None) == AL
    assert run(impl._h, src, sp, l1, lw, dst, w, 1, dst, dp, None) == AL
    dev.torch_.cuda.synchronize()

    def code(fn, *args, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*args, **kw)
        return e.value.code

    assert code(vip.CudaJointBilateralUpsample, w, h, 3) == INV
    assert code(vip.CudaJointBilateralUpsample, w, h, 4, 11) == KS
    f = vip.CudaJointBilateralUpsample(w, h, s, 5)
    assert (f.low_width(), f.low_height()) == (lw, lh)
    d_out, d_in = dev.empty((h, w), np.float32), dev.put(np.zeros((lh, lw), np.float32))
    assert code(f.upsample_f32, d_in, d_l1, d_g1, 2, d_out) == INV
    assert code(f.upsample_f32, d_out, d_l1, d_g1, 1, d_out) == AL
    with pytest.raises(ValueError):  # a 3-channel guide needs width * height * 3 bytes
        f.upsample_f32(d_in, d_l3, d_g1, 3, d_out)
    with pytest.raises(ValueError):  # the low-resolution guide too
        f.upsample_f32(d_in, d_l1, d_g3, 3, d_out)
    with pytest.raises(ValueError):  # the source is float32
        f.upsample_f32(d_l3, d_l1, d_g1, 1, d_out)
    with pytest.raises(ValueError):
        f.upsample_f32(d_in, d_l1, d_g1, 1, dev.empty((h, w // 2), np.float32))


# ---- launch log, kernel timing, streams ----
@pytest.mark.parametrize("s,k,form", [(2, 9, "rgb"), (4, 5, "gray"), (8, 1, "rgb")])
def test_launch_log_and_timing(dev, s, k, form):
    w, h = 67, 33
    g_lo, g_hi = _guides(form, w, h, s)
    impl = _UpsampleImpl(w, h, s, k)
    args = (dev.put(_field(w, h, s)), dev.put(g_lo), dev.put(g_hi), _gch(g_hi), dev.empty((h, w), np.float32))
    launched_kernels()
    impl.upsample_f32(*args)
    names = launched_kernels()
    want = f"vip::upsample_f32_kernel<{k // 2}, {s}, {_gch(g_hi)}, true>"
    assert len(names) == 1 and want in names[0], names
    with kernel_timing(4) as kt:
        impl.upsample_f32(*args)
        impl.upsample_f32(*args)
    rec = kt.records()
    assert len(rec) == 2 and all("vip::upsample_f32_kernel<" in n and ms > 0 for n, ms in rec), rec


@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_one_handle_on_two_streams(dev, numerics, profile):
    torch = dev.torch_
    w, h, s, k = 389, 197, 4, 5
    impl = _UpsampleImpl(w, h, s, k, 1.0, 30.0, numerics)
    ins = []
    for form in FORMS:
        g_lo, g_hi = _guides(form, w, h, s)
        ins.append((dev.put(_field(w, h, s)), dev.put(g_lo), dev.put(g_hi), _gch(g_hi)))
    serial = [dev.empty((h, w), np.float32) for _ in ins]
    for a, d in zip(ins, serial):
        impl.upsample_f32(*a, d)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in ins]
    both = [dev.empty((h, w), np.float32) for _ in ins]
    for a, d, st in zip(ins, both, streams):
        impl.upsample_f32(*a, d, stream=st)
    for st in streams:
        st.synchronize()
    for form, a, b in zip(FORMS, serial, both):
        assert np.array_equal(_bits(dev.get(a)), _bits(dev.get(b))), form
        assert np.array_equal(_bits(dev.get(a)), _bits(_want(form, w, h, s, k, profile))), form
