"""The centre row's shared pair weights and the constant centre tap (vip_stencil.hpp row_taps SHARE).

In the outputs' own row a thread forms the weight of two of its outputs once and both use it,
and the centre tap's weight is one value per launch. Nothing may change by a bit, so every case
compares the HIP output with the oracle of the same numerics profile by np.array_equal, on tiny
frames where the centre row's pairs meet the replicate border (widths below, at and just above a
thread's 8 outputs, 15, and 129 = one 128-pixel tile plus one column) and the tile seams (65
rows = one 64-row tile plus one row): the plain and the joint filter, pitched buffers, a row
band with an odd row count, a 3-frame launch, the texture filter's folded joint filter, a
frame of equal pixels (every pair at distance 0) and a two-value checkerboard (the pairs
alternate between two distances)."""
import numpy as np
import pytest

import various_image_processings_amd as vip
from various_image_processings_amd._lib import call
from various_image_processings_amd.filters import _BilateralImpl

pytestmark = pytest.mark.gpu

PROFILES = [(vip.VIP_NUMERICS_CUDA, 0), (vip.VIP_NUMERICS_CPP, 1)]
WIDTHS = [1, 7, 8, 9, 15, 129]
HEIGHTS = [1, 5, 65]


def _mismatch(a, b):
    d = np.argwhere(a != b)
    return f"{len(d)} mismatches, first {d[:5].tolist()}"


@pytest.fixture(scope="module")
def frames(oracle):
    """(source, guide) per shape, made once: the guide is another draw of the generator."""
    out = {}
    for h in HEIGHTS:
        for w in WIDTHS:
            a = oracle.random_u8(2 * h * w * 3)
            out[(h, w)] = (a[:h * w * 3].reshape(h, w, 3).copy(), a[h * w * 3:].reshape(h, w, 3).copy())
    return out


def _run(dev, img, k, numerics, guide=None, ss=10.0, sc=30.0):
    h, w, _ = img.shape
    impl = _BilateralImpl(w, h, k, ss, sc, numerics)
    d_dst = dev.empty((h, w, 3))
    if guide is None:
        impl.bilateral_filter(dev.put(img), d_dst)
    else:
        impl.joint_bilateral_filter(dev.put(img), dev.put(guide), d_dst)
    return dev.get(d_dst)


@pytest.mark.parametrize("k", [3, 9, 15])
@pytest.mark.parametrize("joint", [False, True], ids=["plain", "joint"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_tiny_frames(dev, oracle, frames, k, joint, numerics, profile):
    for (h, w), (img, guide) in frames.items():
        g = guide if joint else None
        got = _run(dev, img, k, numerics, guide=g)
        want = oracle.bilateral(img, k, profile=profile, guide=g)
        assert np.array_equal(got, want), (h, w, _mismatch(got, want))


@pytest.mark.parametrize("joint", [False, True], ids=["plain", "joint"])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_ksize_31_on_129x65(dev, oracle, frames, joint, numerics, profile):
    img, guide = frames[(65, 129)]
    g = guide if joint else None
    got = _run(dev, img, 31, numerics, guide=g)
    want = oracle.bilateral(img, 31, profile=profile, guide=g)
    assert np.array_equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("k", [3, 9, 15])
@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_equal_pixels_and_checkerboard(dev, oracle, frames, k, numerics, profile):
    """Equal pixels: every weight is ws * wc[0], the output is the input. Checkerboard of
    (10, 20, 30) and (40, 60, 90): pairs at odd distance have d = 120, at even distance d = 0."""
    for h, w in [(5, 9), (65, 129)]:
        flat = np.full((h, w, 3), 77, np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        board = np.where(((yy + xx) & 1)[..., None] == 0, np.array([10, 20, 30], np.uint8),
                         np.array([40, 60, 90], np.uint8)).astype(np.uint8)
        src = frames[(h, w)][0]
        got = _run(dev, flat, k, numerics)
        assert np.array_equal(got, flat) and np.array_equal(got, oracle.bilateral(flat, k, profile=profile)), (h, w)
        for img, g in [(board, None), (src, board), (src, flat), (board, src)]:
            got = _run(dev, img, k, numerics, guide=g)
            want = oracle.bilateral(img, k, profile=profile, guide=g)
            assert np.array_equal(got, want), (h, w, g is not None, _mismatch(got, want))


@pytest.mark.parametrize("joint", [False, True], ids=["plain", "joint"])
def test_pitched_buffers(dev, oracle, frames, joint):
    """129 x 65 in rows of 512 bytes (387 used), through the C ABI."""
    h, w, pitch, k = 65, 129, 512, 15
    img, guide = frames[(h, w)]

    def pitched(a):
        b = np.zeros((h, pitch), np.uint8)
        b[:, :w * 3] = a.reshape(h, w * 3)
        return dev.put(b)

    impl = _BilateralImpl(w, h, k)
    d_src, d_guide, d_dst = pitched(img), pitched(guide), dev.empty((h, pitch))
    if joint:
        call("vip_joint_bilateral_run", impl._h, d_src.data_ptr(), pitch, d_guide.data_ptr(), pitch, d_dst.data_ptr(),
             pitch, None)
    else:
        call("vip_bilateral_run", impl._h, d_src.data_ptr(), pitch, d_dst.data_ptr(), pitch, None)
    got = dev.get(d_dst)[:, :w * 3].reshape(h, w, 3)
    want = oracle.bilateral(img, k, guide=guide if joint else None)
    assert np.array_equal(got, want), _mismatch(got, want)


def test_row_band_with_odd_row_count(dev, oracle, frames):
    """vip_bilateral_run_rows: 51 output rows from row 7 of the 65-row frame, neighbour rows
    clamped to the frame: rows 7..57 of the whole frame's filter."""
    img, _ = frames[(65, 129)]
    impl = _BilateralImpl(129, 65, 15)
    out = dev.empty((51, 129, 3))
    impl.run_rows(dev.put(img), out, 51, 7, 0, 65)
    want = oracle.bilateral(img, 15)[7:58]
    got = dev.get(out)
    assert np.array_equal(got, want), _mismatch(got, want)


def test_three_frame_launch(dev, oracle, frames):
    """vip_bilateral_run_rows_batch: three frames in one launch of the multi-frame kernel."""
    img, guide = frames[(65, 129)]
    imgs = [img, guide, img[::-1, ::-1].copy()]
    impl = _BilateralImpl(129, 65, 15)
    dsts = [dev.empty((65, 129, 3)) for _ in imgs]
    impl.run_rows_batch([dev.put(x) for x in imgs], dsts, 65, 0, 0, 65)
    for f, x in enumerate(imgs):
        got, want = dev.get(dsts[f]), oracle.bilateral(x, 15)
        assert np.array_equal(got, want), (f, _mismatch(got, want))


@pytest.mark.parametrize("numerics,profile", PROFILES)
def test_texture_filter_k5(dev, oracle, numerics, profile):
    """The texture filter at k = 5 on 150 x 100: its joint filter (radius 4) runs on the folded tables."""
    img = oracle.random_image(150, 100)
    d_dst = dev.empty((100, 150, 3))
    vip.CudaBilateralTextureFilter(150, 100, 5, 2, numerics=numerics).execute(dev.put(img), d_dst)
    got, want = dev.get(d_dst), oracle.texture(img, 5, 2, profile)
    assert np.array_equal(got, want), _mismatch(got, want)
