"""GPU parity of the joint bilateral filter on an interleaved f32 source of 2..4 channels under an
8-bit guide (csrc/vip_joint_f32c.hip; include/vip.h vip_joint_bilateral_run_f32c).

Bar: every channel equals tests/f32c_oracle.py (tests/f32_oracle.py per channel) bit for bit, compared
as uint32, in both numerics profiles, with a gray and with a 3-channel guide; and equals
vip_joint_bilateral_run_f32 on the de-interleaved plane, kernel against kernel. The channels of every
source differ (depth, signed, tiny, depth, seeded per channel), so a swapped or repeated channel
fails. Destinations are pre-filled with a sentinel.
"""
import functools

import numpy as np
import pytest

import f32_oracle
import f32c_oracle as fo
import round_shapes as rs
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _BilateralImpl, kernel_timing, launched_kernels

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
FORMS = ["gray", "rgb"]
CHANNELS = [2, 3, 4]
SENTINEL = 0xA5A5A5A5
THREADS = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mismatch(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    first = [(tuple(i), float(a[tuple(i)]), float(b[tuple(i)])) for i in d[:4]]
    return f"{len(d)} mismatches of {a.size}, first (index, got, want) {first}"


def _gch(form):
    return 1 if form == "gray" else 3


# ---- inputs and their oracle outputs: computed once, shared, never written to ----
@functools.lru_cache(maxsize=None)
def _plane(w, h, stat, c):
    p = fo.plane(w, h, stat, c)
    p.setflags(write=False)
    return p


def _source(w, h, ch, stat=None):
    return np.ascontiguousarray(np.stack([_plane(w, h, stat or fo.STATS[c], c) for c in range(ch)], axis=2))


@functools.lru_cache(maxsize=None)
def _guide(form, w, h):
    rng = np.random.default_rng(1000 * w + h + (7 if form == "rgb" else 0))
    g = rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _want_plane(form, w, h, k, profile, stat, c):
    """The oracle of channel c: planes are shared between the channel counts."""
    out = f32_oracle.joint_bilateral(_plane(w, h, stat, c), _guide(form, w, h), k, 10.0, 30.0, profile)
    out.setflags(write=False)
    return out


def _want(form, w, h, ch, k, profile, stat=None):
    return np.stack([_want_plane(form, w, h, k, profile, stat or fo.STATS[c], c) for c in range(ch)], axis=2)


def _fresh(dev, h, w, ch):
    """A destination filled with the sentinel (tests/test_gpu_c1_rounds.py _fresh says why)."""
    return dev.put(np.full((h, w, ch), SENTINEL, np.uint32).view(np.float32))


def _run(dev, f, guide, k, numerics):
    h, w, ch = f.shape
    impl = _BilateralImpl(w, h, k, 10.0, 30.0, numerics)
    d_dst = _fresh(dev, h, w, ch)
    impl.joint_bilateral_filter_f32c(dev.put(f), ch, dev.put(np.array(guide)), 1 if guide.ndim == 2 else 3, d_dst)
    return dev.get(d_dst)


def _check(dev, form, w, h, ch, k, numerics, profile, stat=None):
    got = _run(dev, _source(w, h, ch, stat), _guide(form, w, h), k, numerics)
    want = _want(form, w, h, ch, k, profile, stat)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), \
        ((form, w, h, ch, k, stat), _mismatch(got, want))


def _kernel_name(k, ch, gch, numerics):
    fma = "true" if numerics == vip.VIP_NUMERICS_CUDA else "false"
    if k == 1:
        return f"vip::joint_f32c_k1_kernel<{ch}, {fma}>"
    return f"vip::joint_f32c_kernel<{k // 2}, {ch}, {gch}, {fma}>"


def _one_kernel(want):
    names = launched_kernels()
    assert names and all(want in n for n in names), (want, names)


def _per_plane_on_the_device(dev, f, guide, k, numerics):
    """C calls of the f32 filter on the de-interleaved planes, re-interleaved."""
    h, w, ch = f.shape
    impl = _BilateralImpl(w, h, k, 10.0, 30.0, numerics)
    d_guide = dev.put(np.array(guide))
    out = []
    for c in range(ch):
        d_ref = dev.put(np.full((h, w), SENTINEL, np.uint32).view(np.float32))
        impl.joint_bilateral_filter_f32(dev.put(f[..., c]), d_guide, 1 if guide.ndim == 2 else 3, d_ref)
        out.append(dev.get(d_ref))
    return np.stack(out, axis=2)


# ---- ksize sweep on 131 x 70: crosses the 128-pixel tile seam and the seams of the 64-, 48- and
# 32-row tiles; the base ksizes plus the ksize either side of every wave-count or LUT-copy switch
# of that C and guide (f32c_oracle.switch_ksizes: csrc/vip_joint_f32c.hip F32cForm) ----
def _sweep():
    for ch in CHANNELS:
        for form in FORMS:
            ks = {1, 3, 5, 15} | ({31} if ch == 2 else set()) | set(fo.switch_ksizes(ch, _gch(form)))
            for k in sorted(ks):
                yield pytest.param(ch, form, k, id=f"c{ch}-{form}-k{k}")


def test_the_switches_are_the_ones_the_sweep_names():
    """What the source chooses (16 | 12 | 8 waves, 32 | 16 | 8 LUT copies), as ksizes either side."""
    assert fo.switch_ksizes(2, 1) == [7, 9, 19, 21]            # waves 16 | 12 at R 3 | 4, 12 | 8 at 9 | 10
    assert fo.switch_ksizes(2, 3) == [5, 7, 17, 19, 27, 29]    # waves at 2 | 3 and 8 | 9, copies 16 | 8 at 13 | 14
    assert fo.switch_ksizes(3, 1) == [9, 11]                   # waves 12 | 8 at R 4 | 5
    assert fo.switch_ksizes(3, 3) == [3, 5]                    # waves 12 | 8 at R 1 | 2 (LDS)
    assert fo.switch_ksizes(4, 1) == [13, 15]                  # copies 32 | 16 at R 6 | 7
    assert fo.switch_ksizes(4, 3) == [9, 11]                   # copies 16 | 8 at R 4 | 5


@pytest.mark.parametrize("ch,form,k", list(_sweep()))
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_sweep(dev, ch, form, k, numerics, profile):
    launched_kernels()
    _check(dev, form, 131, 70, ch, k, numerics, profile)
    _one_kernel(_kernel_name(k, ch, _gch(form), numerics))


# ---- shapes at ksize 5 and the largest ksize of that C: tiny frames, one pixel either side of the
# tile width, one row either side of every tile height in use (64, 48, 32) ----
SHAPES = [(1, 1), (2, 3), (3, 1), (63, 3), (65, 3), (127, 3), (129, 3),
          (9, 31), (9, 33), (9, 47), (9, 49), (9, 63), (9, 65)]


def test_the_tile_heights_in_use():
    ths = {fo.tile_rows(ch, k // 2, g) for ch in CHANNELS for g in (1, 3) for k in (5, fo.MAX_KSIZE[ch])}
    assert ths <= {32, 48, 64} and {th + d for th in ths for d in (-1, 1)} <= {h for _, h in SHAPES}


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_shapes(dev, w, h, ch, numerics, profile):
    for form in FORMS:
        for k in (5, fo.MAX_KSIZE[ch]):
            _check(dev, form, w, h, ch, k, numerics, profile)


# ---- source statistics on 67 x 33, ksize 9: every channel tiny (subnormal products; gradual
# underflow is part of the definition), every channel signed ----
@pytest.mark.parametrize("stat", ["tiny", "signed"])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_source_statistics(dev, stat, ch, numerics, profile):
    for form in FORMS:
        _check(dev, form, 67, 33, ch, 9, numerics, profile, stat=stat)


# ---- the tie of the definition, kernel against kernel ----
@pytest.mark.parametrize("w,h,k", [(67, 33, 9), (131, 70, 15)])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_each_channel_is_the_f32_filter_on_the_device(dev, w, h, k, ch, numerics, profile):
    f = _source(w, h, ch)
    for form in FORMS:
        guide = _guide(form, w, h)
        got = _run(dev, f, guide, k, numerics)
        ref = _per_plane_on_the_device(dev, f, guide, k, numerics)
        assert np.array_equal(_bits(got), _bits(ref)), ((form, ch, k), _mismatch(got, ref))


@pytest.mark.parametrize("k", [1, 9, 33])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_one_channel_forwards_to_the_f32_filter(dev, k, numerics, profile):
    """channels 1: the f32 call's kernels (ksize 33 is above every multi-channel cap) and its bits."""
    w, h = 67, 33
    f = _source(w, h, 1)
    fma = "true" if numerics == vip.VIP_NUMERICS_CUDA else "false"
    for form in FORMS:
        guide = _guide(form, w, h)
        launched_kernels()
        got = _run(dev, f, guide, k, numerics)
        _one_kernel(f"vip::joint_f32_kernel<{k // 2}, {_gch(form)}, {fma}>" if 3 <= k <= 31
                    else f"vip::joint_f32_rt_kernel<{_gch(form)}, {fma}>")
        ref = _per_plane_on_the_device(dev, f, guide, k, numerics)
        assert np.array_equal(_bits(got), _bits(ref)), (form, k, _mismatch(got, ref))


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


# which float array is only 4-byte aligned (base + 4, pitch = 4 mod 16) while the other is 16-byte
# aligned with a padded pitch = 0 mod 16; "none": both are 16-byte aligned and padded
@pytest.mark.parametrize("odd", ["none", "src", "dst"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_pitch_and_alignment(dev, ch, k, odd, numerics, profile):
    w, h = 131, 70
    row = w * ch                                  # floats of a row
    padded = (row + 3) // 4 * 4 + 4               # 0 mod 4 floats, and more than a row
    geo = {n: ((4, padded + 1) if n == odd else (0, padded)) for n in ("src", "dst")}  # byte offset, pitch in floats
    f = _source(w, h, ch)
    impl = _BilateralImpl(w, h, k, numerics=numerics)
    t_src, p_src = _pitched(dev, f.view(np.uint8).reshape(h, 4 * row), 4 * geo["src"][1], geo["src"][0])
    t_gg, p_gg = _pitched(dev, _guide("gray", w, h), w + 1, 1)                        # base + 1, pitch w + 1
    t_g3, p_g3 = _pitched(dev, _guide("rgb", w, h).reshape(h, 3 * w), 3 * w + 1, 1)  # base + 1, pitch 3w + 1
    run = _lib.lib().vip_joint_bilateral_run_f32c
    doff, dpf = geo["dst"]
    for form, pg, gp in (("gray", p_gg, w + 1), ("rgb", p_g3, 3 * w + 1)):
        d_dst = dev.put(np.full(doff // 4 + h * dpf + 4, SENTINEL, np.uint32).view(np.int32))
        assert d_dst.data_ptr() % 16 == 0
        rc = run(impl._h, p_src, 4 * geo["src"][1], ch, pg, gp, _gch(form), d_dst.data_ptr() + doff, 4 * dpf, None)
        assert rc == 0, (form, rc)
        raw = dev.get(d_dst).view(np.uint32)
        body = raw[doff // 4: doff // 4 + h * dpf].reshape(h, dpf)
        assert (body[:, row:] == SENTINEL).all(), (form, odd, "row padding written")
        assert (raw[:doff // 4] == SENTINEL).all() and (raw[doff // 4 + h * dpf:] == SENTINEL).all(), (form, odd)
        want = _want(form, w, h, ch, k, profile)
        got = body[:, :row].reshape(h, w, ch)
        assert np.array_equal(got, _bits(want)), (form, odd, _mismatch(got.view(np.float32), want))
    del t_src, t_gg, t_g3


# ---- argument errors: the C ABI's codes, and VipError / ValueError in Python ----
def test_argument_errors(dev):
    w, h = 16, 8
    L = _lib.lib()
    INV, KS, AL = _lib.VIP_ERR_INVALID_ARGUMENT, _lib.VIP_ERR_UNSUPPORTED_KSIZE, _lib.VIP_ERR_ALIASING
    impl = _BilateralImpl(w, h, 5)
    d_src, d_dst = dev.put(np.zeros((h + 1, w, 4), np.float32)), dev.empty((h + 1, w, 4), np.float32)
    d_g1, d_g3 = dev.put(np.zeros((h, w), np.uint8)), dev.put(np.zeros((h, w, 3), np.uint8))
    s, d, g1, g3 = d_src.data_ptr(), d_dst.data_ptr(), d_g1.data_ptr(), d_g3.data_ptr()

    for ch in (1, 2, 3, 4):
        p = 4 * w * ch

        def run(hd=impl._h, s=s, sp=p, ch=ch, g=g1, gp=w, gch=1, d=d, dp=p):
            return L.vip_joint_bilateral_run_f32c(hd, s, sp, ch, g, gp, gch, d, dp, None)

        assert run() == 0
        assert run(g=g3, gp=3 * w, gch=3) == 0
        assert run(hd=None) == INV
        for null in ("s", "g", "d"):
            assert run(**{null: None}) == INV, (ch, null)
        for gch in (0, 2, 4, -1):
            assert run(gch=gch) == INV
        for off in (1, 2, 3):                                   # float bases and pitches: multiples of 4
            for name, base in (("s", s), ("d", d)):
                assert run(**{name: base + off}) == INV, (ch, name, off)
                assert run(**{name + "p": p + off}) == INV, (ch, name, off)
        assert run(s=s + 4, d=d + 4) == 0                       # any multiple of 4 works
        if ch > 1:                                              # a pitch smaller than a row (one channel: the f32 call's checks)
            assert run(sp=p - 4) == INV and run(dp=p - 4) == INV
            assert run(gp=w - 1) == INV
            assert run(g=g3, gp=3 * w - 1, gch=3) == INV
        assert run(d=s) == AL and run(d=g1) == AL               # dst equals an input
        for k in (fo.MAX_KSIZE[ch], fo.MAX_KSIZE[ch] + 2):      # the cap of this channel count, and above it
            hk = _BilateralImpl(w, h, k)
            assert run(hd=hk._h) == (0 if k <= fo.MAX_KSIZE[ch] else KS), (ch, k)
            assert run(hd=hk._h, g=g3, gp=3 * w, gch=3) == (0 if k <= fo.MAX_KSIZE[ch] else KS), (ch, k)
    for ch in (0, 5, -1):
        assert L.vip_joint_bilateral_run_f32c(impl._h, s, 4 * w, ch, g1, w, 1, d, 4 * w, None) == INV
    assert [L.vip_joint_f32c_max_ksize(c) for c in range(6)] == [INV, 47, 31, 15, 15, INV]
    assert L.vip_max_ksize(vip.VIP_FILTER_JOINT_F32C) == 31
    dev.torch_.cuda.synchronize()

    def code(fn, *a, **kw):
        with pytest.raises(vip.VipError) as e:
            fn(*a, **kw)
        return e.value.code

    f = vip.CudaBilateralFilter(w, h, 5)
    big = vip.CudaBilateralFilter(w, h, 17)
    assert code(f.joint_bilateral_filter_f32c, d_src, 2, d_g1, 1, d_src) == AL
    assert code(f.joint_bilateral_filter_f32c, d_src, 2, d_g1, 2, d_dst) == INV
    assert code(f.joint_bilateral_filter_f32c, d_src, 5, d_g1, 1, d_dst) == INV
    assert code(f.joint_bilateral_filter_f32c, d_src, 0, d_g1, 1, d_dst) == INV
    assert code(big.joint_bilateral_filter_f32c, d_src, 3, d_g3, 3, d_dst) == KS
    big.joint_bilateral_filter_f32c(d_src, 2, d_g3, 3, d_dst)   # ksize 17 is inside the two-channel cap
    with pytest.raises(ValueError):  # a 3-channel guide needs width * height * 3 bytes
        f.joint_bilateral_filter_f32c(d_src, 2, d_g1, 3, d_dst)
    with pytest.raises(ValueError):  # the source is float32
        f.joint_bilateral_filter_f32c(d_g3, 2, d_g1, 1, d_dst)
    with pytest.raises(ValueError):  # four channels need width * height * 4 floats
        f.joint_bilateral_filter_f32c(d_src, 4, d_g1, 1, dev.empty((h, w, 3), np.float32))
    with pytest.raises(ValueError):
        f.joint_bilateral_filter_f32c(dev.empty((h, w, 2), np.float32), 3, d_g1, 1, d_dst)


# ---- later rounds: frames of more tiles than the device has CUs (tests/round_shapes.py) ----
@pytest.fixture(scope="module")
def cus(dev):
    return int(dev.torch_.cuda.get_device_properties(0).multi_processor_count)


def _frame(kind, cus, th):
    """(w, h) of the tall or wide frame, with its rounds asserted (as tests/test_gpu_c1_rounds.py)."""
    w, h = {"tall": rs.tall, "wide": rs.wide}[kind](cus, th)
    tiles, full, last = rs.rounds(w, h, th, cus)
    assert tiles > cus and full >= (2 if kind == "tall" else 1) and 0 < last < cus, (kind, w, h, tiles, full, last)
    assert 0 < h % th < th
    return w, h


def _in_bands(plane, guide, k, profile):
    return rs.in_bands(lambda f, g: f32_oracle.joint_bilateral(f, g, k, 10.0, 30.0, profile), k // 2, plane, guide,
                       threads=THREADS)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_tall(dev, cus, ch, form, numerics, profile):
    """Two full rounds and a partial third in one tile column, 9 pixels wide: every vector path off."""
    k = 5
    w, h = _frame("tall", cus, fo.tile_rows(ch, k // 2, _gch(form)))
    f, guide = _source(w, h, ch), _guide(form, w, h)
    launched_kernels()
    got = _run(dev, f, guide, k, numerics)
    _one_kernel(_kernel_name(k, ch, _gch(form), numerics))
    want = np.stack([_in_bands(f[..., c], guide, k, profile) for c in range(ch)], axis=2)
    assert np.array_equal(_bits(got), _bits(want)), ((ch, form, w, h), _mismatch(got, want))


WIDE = [pytest.param(ch, form, *PROFILES[i % 2], id=f"c{ch}-{form}-" + ("cuda" if i % 2 == 0 else "cpp"))
        for i, (ch, form) in enumerate((c, f) for c in (2, 4) for f in FORMS)]


@pytest.mark.parametrize("ch,form,numerics,profile", WIDE)
def test_wide(dev, cus, ch, form, numerics, profile):
    """One full round and a partial second over three tile columns, every vector path on: all
    channels against the device's per-plane route, the last channel against the CPU oracle."""
    k = 5
    w, h = _frame("wide", cus, fo.tile_rows(ch, k // 2, _gch(form)))
    f, guide = _source(w, h, ch), _guide(form, w, h)
    launched_kernels()
    got = _run(dev, f, guide, k, numerics)
    _one_kernel(_kernel_name(k, ch, _gch(form), numerics))
    ref = _per_plane_on_the_device(dev, f, guide, k, numerics)
    assert np.array_equal(_bits(got), _bits(ref)), ((ch, form, w, h), _mismatch(got, ref))
    want = _in_bands(f[..., ch - 1], guide, k, profile)
    assert np.array_equal(_bits(got[..., ch - 1]), _bits(want)), ((ch, form, w, h), _mismatch(got[..., ch - 1], want))


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_1_on_a_frame_taller_than_the_grid(dev, ch, numerics, profile):
    """The elementwise ksize-1 kernel strides its rows over grid.y, which stops at 65535."""
    launched_kernels()
    _check(dev, "gray", 3, 65541, ch, 1, numerics, profile)
    _one_kernel(_kernel_name(1, ch, 1, numerics))


# ---- launch log and kernel timing see the kernels ----
@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("ch", CHANNELS)
def test_launch_log_and_timing(dev, ch, k):
    impl = _BilateralImpl(67, 33, k)
    d_src, d_guide = dev.put(_source(67, 33, ch)), dev.put(np.array(_guide("rgb", 67, 33)))
    d_dst = _fresh(dev, 33, 67, ch)
    launched_kernels()
    impl.joint_bilateral_filter_f32c(d_src, ch, d_guide, 3, d_dst)
    names = launched_kernels()
    assert len(names) == 1 and _kernel_name(k, ch, 3, vip.VIP_NUMERICS_CUDA) in names[0], names
    with kernel_timing(1) as kt:
        impl.joint_bilateral_filter_f32c(d_src, ch, d_guide, 3, d_dst)
    rec = kt.records()
    assert len(rec) == 1 and "joint_f32c" in rec[0][0] and rec[0][1] > 0, rec
