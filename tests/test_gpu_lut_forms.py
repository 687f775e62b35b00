"""GPU parity at the colour LUT's form switches and at its top entries (tests/lut_frames.py).

Bar: every output equals the oracle of the same numerics profile bit for bit.

A. Both sides of each switch, with the launched form asserted from vip_launched_kernels: the
   joint filter's folded 32-entry tables behind the saturating 16-bit address against the
   768-entry LUT (launch_bilateral_r: lut_nonzero <= DZ(R), radius 1..6), and the adaptive
   filter's 512-entry saturating LUT against the 1536-entry one (launch_adaptive_r:
   lut_nonzero <= 511; adaptive_frames_kernel switches the same way). The weights near a zero
   point are ~1e-45 and cannot move a u8 output: what these cases detect is a wrong address,
   which reads something that is not zero. The same frames carry the small distances, whose
   weights show, densely on either side of the switch.
B. The LUT's last entries (d = 765, adaptive 1529, gray 255 / 509) under a sigma_color that
   gives them a visible weight (1000: wc[765] ~ 0.75), in every filter family.
C. Flat frames at the ends of the byte range: the largest sumk, the clamped pack at 255.
D. The row padding of a pitched destination stays untouched.

tests/test_lut_frames.py checks on the CPU that the frames reach these distances and that every
adaptive case here keeps sumk > 0.
"""
import numpy as np
import pytest

import f32_oracle
import gray_adaptive_oracle as gao
import gray_oracle
import lut_frames as lf
import upsample_oracle as uo
import various_image_processings_amd as vip
from various_image_processings_amd import _lib
from various_image_processings_amd.filters import _AdaptiveImpl, _BilateralImpl, _UpsampleImpl

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
W, H = lf.W, lf.H
SS = 10.0
FOLDED, UNFOLDED = "32, true, 16, true>", "768, false, 16, false>"
ADA_SAT, ADA_FULL = "512, true>", "1536, false>"
K_SAT_MAX_R = 6  # vip_launch.hpp kSatMaxR: no folded form past it


def disc_r2_count(R):
    return len({x * x + y * y for x in range(R + 1) for y in range(R + 1) if x * x + y * y <= R * R})


def DZ(R):
    """SatLut<R, ...>::DZ (vip_stencil.hpp), restated as tests/test_satlut.py does: the largest
    distance whose folded entries the 16-bit address reaches before it saturates."""
    return min((65535 - 124) // (disc_r2_count(R) * 128), 31)


def _mismatch(a, b):
    d = np.argwhere(a != b)
    return f"{len(d)} mismatches, first {d[:5].tolist()}" + (f" got {a[tuple(d[0])]} want {b[tuple(d[0])]}" if len(d) else "")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _put(dev, a):
    return dev.put(np.array(a))  # a writable copy: the shared frames are read-only


# ---- 3-channel runs through the C ABI; pad > 0: pitched buffers, source padding 0xA5,
# destination padding 0x5A (tests/test_gpu_fuzz.py) ----
def _pitched(dev, img, pad, fill):
    h, w, _ = img.shape
    buf = dev.empty((h, w * 3 + pad))
    buf.fill_(fill)
    buf[:, :w * 3] = _put(dev, img.reshape(h, w * 3))
    return buf


def _run3(dev, kind, img, k, sc, numerics, guide=None, pad=0):
    """(output, destination padding, launched kernel names) of one bilateral / joint / adaptive run."""
    h, w, _ = img.shape
    pitch = w * 3 + pad
    src, dst = _pitched(dev, img, pad, 0xA5), _pitched(dev, np.zeros_like(img), pad, 0x5A)
    lib = _lib.lib()
    vip.launched_kernels()  # clears the list
    if kind == "adaptive":
        impl = _AdaptiveImpl(w, h, k, SS, sc, numerics)
        _lib.check("vip_adaptive_run", lib.vip_adaptive_run(impl._h, src.data_ptr(), pitch, dst.data_ptr(), pitch, None))
    elif guide is None:
        impl = _BilateralImpl(w, h, k, SS, sc, numerics)
        _lib.check("vip_bilateral_run", lib.vip_bilateral_run(impl._h, src.data_ptr(), pitch, dst.data_ptr(), pitch, None))
    else:
        impl = _BilateralImpl(w, h, k, SS, sc, numerics)
        gbuf = _pitched(dev, guide, pad, 0xA5)
        _lib.check("vip_joint_bilateral_run", lib.vip_joint_bilateral_run(
            impl._h, src.data_ptr(), pitch, gbuf.data_ptr(), pitch, dst.data_ptr(), pitch, None))
    names = vip.launched_kernels()
    a = dev.get(dst)
    return np.ascontiguousarray(a[:, :w * 3]).reshape(h, w, 3), a[:, w * 3:], names


def _one_kernel(names, prefix, suffix):
    assert len(names) == 1 and names[0].startswith(prefix) and names[0].endswith(suffix), (names, prefix, suffix)
    return names[0]


# oracle outputs: computed once, shared (part D runs cases of A and B again), never written to
_cache = {}


def _want(key, fn):
    if key not in _cache:
        out = fn()
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


GUIDES = {"noise_guide": lambda w=W: lf.noise_guide(w=w), "two_level_noisy": lf.two_level_noisy, "two_level": lf.two_level}


def _joint_want(oracle, gname, k, sc, profile):
    return _want(("joint", gname, k, sc, profile),
                 lambda: oracle.joint_bilateral(lf.random_source(), GUIDES[gname](), k, SS, sc, profile))


def _plain_want(oracle, fname, w, k, sc, profile):
    return _want(("plain", fname, w, k, sc, profile), lambda: oracle.bilateral(GUIDES[fname](w), k, SS, sc, profile))


# =============================== A. both sides of each switch ===============================
def _joint_zero_points(R):
    if R > K_SAT_MAX_R:
        return (25,)                  # the texture filter's zero point: folded for R <= 6 only
    return (31, 32) if DZ(R) == 31 else (DZ(R), DZ(R) + 1, 31)  # R = 6: tables exist at 31, and must not be used


@pytest.mark.parametrize("gname", ["noise_guide", "two_level_noisy"])
@pytest.mark.parametrize("R", range(1, 8))
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_switch(dev, oracle, numerics, profile, R, gname):
    k = 2 * R + 1
    assert [DZ(r) for r in range(1, 7)] == [31, 31, 31, 31, 31, 26]
    for zp in _joint_zero_points(R):
        sc = lf.sigma_with_zero_point(768, zp, profile)
        got, _, names = _run3(dev, "joint", lf.random_source(), k, sc, numerics, guide=GUIDES[gname]())
        folded = R <= K_SAT_MAX_R and zp <= DZ(R)
        name = _one_kernel(names, f"void vip::bilateral_kernel<{R}, ", FOLDED if folded else UNFOLDED)
        print(f"joint R={R} k={k} lut_nonzero={zp} sigma_color={sc!r} profile={profile}: {name}")
        want = _joint_want(oracle, gname, k, sc, profile)
        assert np.array_equal(got, want), (R, zp, gname, _mismatch(got, want))


@pytest.mark.parametrize("R", [4, 6])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_switch_row_band(dev, oracle, numerics, profile, R):
    """vip_bilateral_run_rows with a guide: 51 rows from row 7."""
    k, row0, rows = 2 * R + 1, 7, 51
    src, guide = lf.random_source(), lf.noise_guide()
    d_src, d_guide = _put(dev, src), _put(dev, guide)
    for zp in _joint_zero_points(R):
        sc = lf.sigma_with_zero_point(768, zp, profile)
        impl = _BilateralImpl(W, H, k, SS, sc, numerics)
        d_dst = dev.empty((rows, W, 3))
        vip.launched_kernels()
        impl.run_rows(d_src, d_dst, rows, row0, 0, H, d_guide=d_guide)
        _one_kernel(vip.launched_kernels(), f"void vip::bilateral_kernel<{R}, ", FOLDED if zp <= DZ(R) else UNFOLDED)
        got = dev.get(d_dst)
        want = oracle.joint_bilateral_rows(src, guide, row0, rows, k, SS, sc, profile)
        assert np.array_equal(got, want), (R, zp, _mismatch(got, want))
        assert np.array_equal(want, _joint_want(oracle, "noise_guide", k, sc, profile)[row0:row0 + rows])


@pytest.mark.parametrize("zp", lf.ADAPTIVE_SWITCH)
@pytest.mark.parametrize("k", lf.ADAPTIVE_SWITCH_KSIZES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_adaptive_switch(dev, oracle, numerics, profile, k, zp):
    sc = lf.sigma_with_zero_point(1536, zp, profile)
    got, _, names = _run3(dev, "adaptive", lf.blocks(), k, sc, numerics)
    name = _one_kernel(names, f"void vip::adaptive_kernel<{k // 2}, ", ADA_SAT if zp <= 511 else ADA_FULL)
    print(f"adaptive k={k} lut_nonzero={zp} sigma_color={sc!r} profile={profile}: {name}")
    want = _want(("adaptive", "blocks", k, sc, profile), lambda: oracle.adaptive(lf.blocks(), k, SS, sc, profile))
    assert np.array_equal(got, want), (k, zp, _mismatch(got, want))


@pytest.mark.parametrize("zp", lf.ADAPTIVE_SWITCH)
@pytest.mark.parametrize("k", lf.ADAPTIVE_BATCH_KSIZES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_adaptive_switch_three_frames(dev, oracle, numerics, profile, k, zp):
    """run_rows_batch: one adaptive_frames_kernel launch over three frames."""
    sc = lf.sigma_with_zero_point(1536, zp, profile)
    frames = lf.blocks_batch()
    impl = _AdaptiveImpl(W, H, k, SS, sc, numerics)
    srcs, dsts = [_put(dev, f) for f in frames], [dev.empty((H, W, 3)) for _ in frames]
    vip.launched_kernels()
    impl.run_rows_batch(srcs, dsts, H, 0, 0, H)
    name = _one_kernel(vip.launched_kernels(), f"void vip::adaptive_frames_kernel<{k // 2}, ",
                       ADA_SAT if zp <= 511 else ADA_FULL)
    print(f"adaptive, 3 frames, k={k} lut_nonzero={zp} profile={profile}: {name}")
    for f, frame in enumerate(frames):
        got, want = dev.get(dsts[f]), oracle.adaptive(frame, k, SS, sc, profile)
        assert np.array_equal(got, want), (k, zp, f, _mismatch(got, want))


# =============================== B. the LUT's last entries, visible ===============================
TOP_SIGMAS = (1000.0, 200.0)


@pytest.mark.parametrize("w", [129, 257])  # 257: the wide 256-pixel tiles are chosen
@pytest.mark.parametrize("k", [3, 15, 31, 41])  # 41: the runtime-radius kernel
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_plain_top_entries(dev, oracle, numerics, profile, k, w):
    for fname in ("two_level", "two_level_noisy"):
        for sc in TOP_SIGMAS:
            got, _, names = _run3(dev, "bilateral", GUIDES[fname](w), k, sc, numerics)
            want = _plain_want(oracle, fname, w, k, sc, profile)
            assert np.array_equal(got, want), (fname, sc, names, _mismatch(got, want))


@pytest.mark.parametrize("k", [3, 15])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_plain_top_entries_forced_tiles(dev, oracle, numerics, profile, k):
    """4 waves per workgroup, 256-pixel tiles (vip_bilateral_set_waves / _set_wide)."""
    vip.set_bilateral_waves(4)
    vip.set_bilateral_wide(2)
    try:
        got, _, names = _run3(dev, "bilateral", lf.two_level_noisy(257), k, 1000.0, numerics)
    finally:
        vip.set_bilateral_waves(0)
        vip.set_bilateral_wide(0)
    _one_kernel(names, f"void vip::bilateral_kernel<{k // 2}, 4, ", "768, false, 64, false>")
    want = _plain_want(oracle, "two_level_noisy", 257, k, 1000.0, profile)
    assert np.array_equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("k", [5, 15, 25])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_top_entries(dev, oracle, numerics, profile, k):
    for sc in TOP_SIGMAS:
        got, _, names = _run3(dev, "joint", lf.random_source(), k, sc, numerics, guide=lf.two_level())
        _one_kernel(names, f"void vip::bilateral_kernel<{k // 2}, ", UNFOLDED)
        want = _joint_want(oracle, "two_level", k, sc, profile)
        assert np.array_equal(got, want), (sc, _mismatch(got, want))


ADAPTIVE_TOP = [("lone_pixel", lambda: lf.lone_pixel(False), 15, 1e4), ("lone_pixel", lambda: lf.lone_pixel(False), 31, 1e4),
                ("lone_pixel_neg", lambda: lf.lone_pixel(True), 15, 1e4), ("lone_pixel_neg", lambda: lf.lone_pixel(True), 31, 1e4),
                ("two_level_noisy", lf.two_level_noisy, 9, 1000.0)]


@pytest.mark.parametrize("fname,frame,k,sc", ADAPTIVE_TOP, ids=[f"{c[0]}-{c[2]}" for c in ADAPTIVE_TOP])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_adaptive_top_entries(dev, oracle, numerics, profile, fname, frame, k, sc):
    img = frame()
    got, _, names = _run3(dev, "adaptive", img, k, sc, numerics)
    _one_kernel(names, f"void vip::adaptive_kernel<{k // 2}, ", ADA_FULL)
    want = oracle.adaptive(img, k, SS, sc, profile)
    assert np.array_equal(got, want), (fname, k, _mismatch(got, want))


# ---- the one-channel families: the same frames reduced to channel 0, each family's own oracle ----
def _gray_run(dev, g, k, sc, numerics, guide=None):
    """tests/test_gpu_gray.py's _run."""
    h, w = g.shape
    impl = _BilateralImpl(w, h, k, SS, sc, numerics)
    d_dst = dev.empty((h, w))
    if guide is None:
        impl.bilateral_filter_c1(_put(dev, g), d_dst)
    else:
        impl.joint_bilateral_filter_c1(_put(dev, g), _put(dev, guide), 1 if guide.ndim == 2 else 3, d_dst)
    return dev.get(d_dst)


@pytest.mark.parametrize("w", [129, 257])
@pytest.mark.parametrize("k", [3, 15, 31, 41])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_gray_plain_top_entries(dev, numerics, profile, k, w):
    for frame in (lf.two_level(w), lf.two_level_noisy(w)):
        g = lf.gray(frame)
        for sc in TOP_SIGMAS:
            got, want = _gray_run(dev, g, k, sc, numerics), gray_oracle.bilateral(g, k, SS, sc, profile)
            assert np.array_equal(got, want), (sc, _mismatch(got, want))


@pytest.mark.parametrize("form", ["gray", "rgb"])
@pytest.mark.parametrize("k", [5, 15, 25])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_gray_joint_top_entries(dev, numerics, profile, k, form):
    g = lf.gray(lf.random_source())
    guide = lf.gray(lf.two_level()) if form == "gray" else lf.two_level()
    for sc in TOP_SIGMAS:
        got = _gray_run(dev, g, k, sc, numerics, guide)
        want = gray_oracle.joint_bilateral(g, guide, k, SS, sc, profile)
        assert np.array_equal(got, want), (sc, _mismatch(got, want))


@pytest.mark.parametrize("fname,frame,k,sc", ADAPTIVE_TOP, ids=[f"{c[0]}-{c[2]}" for c in ADAPTIVE_TOP])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_gray_adaptive_top_entries(dev, numerics, profile, fname, frame, k, sc):
    """The lone pixel reaches d = 509 (ksize 31) of the 512-entry table."""
    g = lf.gray(frame())
    impl = _AdaptiveImpl(W, H, k, SS, sc, numerics)
    d_dst = dev.empty((H, W))
    impl.execute_c1(_put(dev, g), d_dst)
    got, want = dev.get(d_dst), gao.adaptive(g, k, SS, sc, profile)
    assert np.array_equal(got, want), (fname, k, _mismatch(got, want))


def _depth(w, h):
    """tests/test_gpu_joint_f32.py's `depth` source: uniform [0.5, 10)."""
    return np.ascontiguousarray(np.random.default_rng(977 * w + 31 * h).uniform(0.5, 10.0, (h, w)), dtype=np.float32)


@pytest.mark.parametrize("form", ["gray", "rgb"])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_joint_f32_top_entries(dev, numerics, profile, k, form):
    f = _depth(W, H)
    guide = lf.gray(lf.two_level()) if form == "gray" else lf.two_level()
    for sc in TOP_SIGMAS:
        impl = _BilateralImpl(W, H, k, SS, sc, numerics)
        d_dst = dev.empty((H, W), np.float32)
        impl.joint_bilateral_filter_f32(dev.put(f), _put(dev, guide), 1 if form == "gray" else 3, d_dst)
        got, want = dev.get(d_dst), f32_oracle.joint_bilateral(f, guide, k, SS, sc, profile)
        d = np.argwhere(_bits(got) != _bits(want))
        assert not len(d), (sc, len(d), [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in d[:4]])


def _upsample(dev, f, g_lo, g_hi, s, k, sc, numerics):
    h, w = g_hi.shape[:2]
    impl = _UpsampleImpl(w, h, s, k, 1.0, sc, numerics)
    assert (impl.low_width(), impl.low_height()) == uo.low_size(w, h, s) == f.shape[::-1]
    d_dst = dev.empty((h, w), np.float32)
    impl.upsample_f32(dev.put(f), _put(dev, g_lo), _put(dev, g_hi), 1 if g_hi.ndim == 2 else 3, d_dst)
    return dev.get(d_dst)


@pytest.mark.parametrize("form", ["gray", "rgb"])
@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_upsample_top_entries(dev, numerics, profile, s, form):
    """guide_hi is two_level, guide_lo its [::s, ::s] subsample: the cells across a checker edge
    are at d = 765 (gray 255)."""
    g_hi = lf.gray(lf.two_level()) if form == "gray" else lf.two_level()
    g_lo = np.ascontiguousarray(g_hi[::s, ::s])
    lw, lh = uo.low_size(W, H, s)
    f = _depth(lw, lh)
    for sc in TOP_SIGMAS:
        got = _upsample(dev, f, g_lo, g_hi, s, 5, sc, numerics)
        want = uo.upsample(f, g_lo, g_hi, s, 5, 1.0, sc, profile)
        d = np.argwhere(_bits(got) != _bits(want))
        assert not len(d), (sc, len(d), [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in d[:4]])


@pytest.mark.parametrize("s", uo.SCALES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_upsample_all_fallback_under_a_3_channel_guide(dev, numerics, profile, s):
    """0 against 255 in every channel: d = 765 at every tap, wc[765] = 0 at sigma_color 1, so every
    pixel takes the nearest sample."""
    lw, lh = uo.low_size(W, H, s)
    f = _depth(lw, lh)
    g_lo, g_hi = np.zeros((lh, lw, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    got = _upsample(dev, f, g_lo, g_hi, s, 5, 1.0, numerics)
    want, zero = uo.upsample(f, g_lo, g_hi, s, 5, 1.0, 1.0, profile, with_fallback=True)
    assert zero.all()
    assert np.array_equal(want, f[(np.arange(H) // s)[:, None], (np.arange(W) // s)[None, :]])
    assert np.array_equal(_bits(got), _bits(want)), _mismatch(_bits(got), _bits(want))


# =============================== C. flat frames ===============================
FLAT_SHAPES = [(v, W) for v in (0, 1, 254, 255)] + [(255, 1), (255, 9)]


@pytest.mark.parametrize("v,w", FLAT_SHAPES)
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_flat_frames_come_back(dev, oracle, numerics, profile, v, w):
    """The largest sumk values through the division and the clamped pack at the top byte value:
    the output is the oracle's, and the oracle's is the input."""
    img = lf.flat(v, w)
    for k in (3, 31, 65):
        got, _, _ = _run3(dev, "bilateral", img, k, 30.0, numerics)
        want = _want(("flat", v, w, k, profile), lambda: oracle.bilateral(img, k, SS, 30.0, profile))
        assert np.array_equal(want, img)
        assert np.array_equal(got, want), ("bilateral", k, _mismatch(got, want))
        g = lf.gray(img)
        got = _gray_run(dev, g, k, 30.0, numerics)
        want = _want(("flat gray", v, w, k, profile), lambda: gray_oracle.bilateral(g, k, SS, 30.0, profile))
        assert np.array_equal(want, g)
        assert np.array_equal(got, want), ("gray", k, _mismatch(got, want))
    for k in (3, 31, 63):
        got, _, _ = _run3(dev, "adaptive", img, k, 30.0, numerics)
        want = _want(("flat adaptive", v, w, k, profile), lambda: oracle.adaptive(img, k, SS, 30.0, profile))
        assert np.array_equal(want, img)
        assert np.array_equal(got, want), ("adaptive", k, _mismatch(got, want))


# =============================== D. write padding stays untouched ===============================
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_row_padding_is_not_written(dev, oracle, numerics, profile):
    """One case of A (the folded joint form, radius 4) and one of B through pitched buffers:
    pitch = width * 3 + 13, source padding 0xA5, destination padding 0x5A."""
    sc = lf.sigma_with_zero_point(768, 31, profile)
    got, tail, names = _run3(dev, "joint", lf.random_source(), 9, sc, numerics, guide=lf.noise_guide(), pad=13)
    _one_kernel(names, "void vip::bilateral_kernel<4, ", FOLDED)
    want = _joint_want(oracle, "noise_guide", 9, sc, profile)
    assert np.array_equal(got, want), _mismatch(got, want)
    assert tail.shape == (H, 13) and (tail == 0x5A).all(), "the row padding of the output was written"
    got, tail, _ = _run3(dev, "bilateral", lf.two_level_noisy(), 15, 1000.0, numerics, pad=13)
    want = _plain_want(oracle, "two_level_noisy", W, 15, 1000.0, profile)
    assert np.array_equal(got, want), _mismatch(got, want)
    assert tail.shape == (H, 13) and (tail == 0x5A).all(), "the row padding of the output was written"
