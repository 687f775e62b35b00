"""The HIP path against the reference tests' OWN oracles (tests/golden/ref_oracles.npz: the
Ref* classes of test/adaptive_bilateral_filter.cu, test/bilateral_texture_filter.cu and
test/gradient.cu, compiled in place; tests/golden/make_ref_golden.py), at the tolerances the
reference's own CUDA tests apply to its kernels:

  adaptive      +-1 per channel   test/adaptive_bilateral_filter.cu:185-193 (exact share printed)
  blur / rtv    FLOAT_EQ (4 ulp)  test/bilateral_texture_filter.cu:253-262
  guide         EQ                test/bilateral_texture_filter.cu:279-283
  gradient      FLOAT_EQ          test/gradient.cu (CudaRandom* cases)

Frames beyond the fixture's 50x50 arrays (640x360, lenna) compare with the oracle's REF
profile, which tests/test_ref_pinned.py pins to those Ref oracles by sha256.

And against the reference's include/cpp CPU filters (tests/golden/ref_cpp_filters.npz:
bilateral_filter, joint_bilateral_filter, adaptive_bilateral_filter compiled whole where they
lie over our own stand-in for OpenCV's containers -- the reference's arithmetic text ran,
OpenCV's containers did not), on whole frames, borders included, with a guide distinct from
the source:

  VIP_NUMERICS_CPP    equal, bit for bit (include/cpp defines that profile)
  VIP_NUMERICS_CUDA   +-1 per channel (test/bilateral_filter.cu EXPECT_NEAR 1; exact share printed)

The 50x50 outputs are stored whole. The tile-crossing frame, 640x360 and lenna compare with
the oracle's CPP profile, which tests/test_ref_pinned.py pins to include/cpp by sha256. The
f32 multi-channel joint filter on float32(src), rounded, is tied to the same joint entries.
Nothing here reads oracle/_ref/ or the reference. Still unpinned, because nothing here can
execute it: the CUDA profile's fma contraction, and the whole-pipeline texture filter, whose
include/cpp form calls cv::ximgproc.
"""
import os
import sys

import numpy as np
import pytest

import various_image_processings_amd as vip
from conftest import GOLDEN
from various_image_processings_amd.filters import _TextureImpl

sys.path.insert(0, GOLDEN)
import make_ref_golden as mrg  # noqa: E402

pytestmark = pytest.mark.gpu
NUMERICS = [vip.VIP_NUMERICS_CUDA, vip.VIP_NUMERICS_CPP]


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "ref_oracles.npz")))


@pytest.fixture(scope="module")
def inputs(oracle):
    return mrg.inputs(oracle)


def ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _adaptive(dev, img, k, numerics):
    h, w, _ = img.shape
    d_dst = dev.empty((h, w, 3))
    vip.CudaAdaptiveBilateralFilter(w, h, k, numerics=numerics).execute(dev.put(img), d_dst)
    return dev.get(d_dst)


def _near1(got, want, what):
    d = np.abs(got.astype(int) - want.astype(int))
    print(f"{what}: max |d| {d.max()}, exact {100 * (d == 0).mean():.4f} %")
    assert d.max() <= 1, what
    return (d == 0).mean()


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("k", mrg.SMALL_K)
def test_adaptive_vs_reference_oracle(dev, fixture, inputs, k, numerics):
    _near1(_adaptive(dev, inputs["img50"], k, numerics), fixture[f"adaptive_k{k}"], f"adaptive k{k} numerics {numerics}")


@pytest.mark.parametrize("numerics", NUMERICS)
def test_adaptive_vs_reference_oracle_large(dev, oracle, inputs, lenna, numerics):
    for img, k in ((inputs["img640"], 9), (lenna, 15)):
        want = oracle.adaptive(img, k, profile=oracle.REF, threads=16)
        assert _near1(_adaptive(dev, img, k, numerics), want, f"adaptive {img.shape} k{k}") > 0.9999


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("k", mrg.SMALL_K)
def test_texture_stages_vs_reference_oracle(dev, fixture, inputs, k, numerics):
    t = _TextureImpl(50, 50, k, 1, numerics)
    d_b, d_r = dev.empty((50, 50, 3), np.float32), dev.empty((50, 50), np.float32)
    t.compute_blur_and_rtv(dev.put(inputs["img50"]), dev.put(inputs["mag50"]), d_b, d_r)
    assert ulps(dev.get(d_b), fixture[f"blurred_k{k}"]).max() <= 4
    assert ulps(dev.get(d_r), fixture[f"rtv_k{k}"]).max() <= 4
    d_g = dev.empty((50, 50, 3))
    t.compute_guide(dev.put(inputs["blur50"]), dev.put(inputs["rtv50"]), d_g)
    assert np.array_equal(dev.get(d_g), fixture[f"guide_k{k}"])


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("k", mrg.CHAIN_K)
def test_texture_stage_chain_640_vs_reference_oracle(dev, oracle, inputs, k, numerics):
    """Each HIP stage on the Ref chain's own inputs (a 640x360 frame, its Ref gradient, the Ref
    blur/rtv of it): magnitude and blur/rtv FLOAT_EQ, guide EQ."""
    img = inputs["img640"]
    mag = oracle.gradient(img, oracle.REF)
    d_m = dev.empty((360, 640), np.float32)
    vip.cuda_gradient(dev.put(img), d_m, 640, 360, 3, numerics=numerics)
    assert ulps(dev.get(d_m), mag).max() <= 4
    b, r = oracle.blur_rtv(img, mag, k, oracle.REF)
    t = _TextureImpl(640, 360, k, 1, numerics)
    d_b, d_r = dev.empty((360, 640, 3), np.float32), dev.empty((360, 640), np.float32)
    t.compute_blur_and_rtv(dev.put(img), dev.put(mag), d_b, d_r)
    assert ulps(dev.get(d_b), b).max() <= 4
    assert ulps(dev.get(d_r), r).max() <= 4
    d_g = dev.empty((360, 640, 3))
    t.compute_guide(dev.put(b), dev.put(r), d_g)
    assert np.array_equal(dev.get(d_g), oracle.guide(b, r, k, oracle.REF))


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("name", ["u8c1", "u8c3", "f32c1", "f32c3"])
def test_gradient_vs_reference_oracle(dev, fixture, inputs, name, numerics):
    src = inputs[name]
    d_dst = dev.empty((50, 50), np.float32)
    vip.cuda_gradient(dev.put(src), d_dst, 50, 50, src.shape[2], numerics=numerics)
    assert ulps(dev.get(d_dst), fixture[f"gradient_{name}"]).max() <= 4


# ---- include/cpp filters: tests/golden/ref_cpp_filters.npz ----
@pytest.fixture(scope="module")
def cppfix():
    return dict(np.load(os.path.join(GOLDEN, "ref_cpp_filters.npz")))


@pytest.fixture(scope="module")
def cpp_inputs(oracle, lenna):
    return mrg.cpp_inputs(oracle, lenna)


@pytest.fixture(scope="module")
def cpp_large(oracle, cpp_inputs):
    """The oracle's CPP profile on the digest cases, once for both numerics."""
    f = mrg.oracle_filters(oracle, oracle.CPP, threads=16)
    out = {(name, k): mrg.cpp_frame(f, cpp_inputs, name, k) for name, k in (("tile", 9), ("f640", 15))}
    out[("lenna", 11)] = dict(bilateral=f["bilateral"](cpp_inputs["lenna"][0], 11, 10.0, 30.0))
    return out


def _bilateral(dev, img, k, ss, sc, numerics, guide=None):
    h, w, _ = img.shape
    f = vip.CudaBilateralFilter(w, h, k, ss, sc, numerics=numerics)
    d_dst = dev.empty((h, w, 3))
    if guide is None:
        f.bilateral_filter(dev.put(img), d_dst)
    else:
        f.joint_bilateral_filter(dev.put(img), dev.put(guide), d_dst)
    return dev.get(d_dst)


def _cpp_check(got, want, numerics, what):
    """CPP numerics: the include/cpp bytes. CUDA numerics: the reference tests' +-1."""
    if numerics == vip.VIP_NUMERICS_CPP:
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (what, len(bad), bad[:5].tolist())
    else:
        _near1(got, want, what + " CUDA numerics")


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("k,ss,sc", mrg.CPP_BILATERAL)
def test_bilateral_vs_include_cpp(dev, cppfix, cpp_inputs, k, ss, sc, numerics):
    got = _bilateral(dev, cpp_inputs["f50"][0], k, ss, sc, numerics)
    _cpp_check(got, cppfix[mrg.bil_key(k, ss, sc)], numerics, mrg.bil_key(k, ss, sc))


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("k", mrg.CPP_JOINT_K)
def test_joint_bilateral_vs_include_cpp(dev, cppfix, cpp_inputs, k, numerics):
    img, guide = cpp_inputs["f50"]
    got = _bilateral(dev, img, k, 10.0, 30.0, numerics, guide=guide)
    _cpp_check(got, cppfix[f"cpp_joint_k{k}"], numerics, f"cpp_joint_k{k}")


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("k", mrg.CPP_ADAPTIVE_K)
def test_adaptive_vs_include_cpp(dev, cppfix, cpp_inputs, k, numerics):
    got = _adaptive(dev, cpp_inputs["f50"][0], k, numerics)
    _cpp_check(got, cppfix[f"cpp_adaptive_k{k}"], numerics, f"cpp_adaptive_k{k}")


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("name,k", [("tile", 9), ("f640", 15), ("lenna", 11)])
def test_filters_vs_include_cpp_large(dev, cppfix, cpp_inputs, cpp_large, name, k, numerics):
    """The 259x70 frame (every tile of the 3-channel kernels crossed, ksize 9), 640x360 (ksize
    15) and lenna (ksize 11, bilateral): the oracle's CPP profile carries the include/cpp
    digest (asserted), and the HIP outputs compare with it."""
    img, guide = cpp_inputs[name]
    for flt, want in cpp_large[(name, k)].items():
        assert np.array_equal(mrg.sha(want), cppfix[f"cpp_{flt}_{name}_k{k}_sha256"]), flt
        if flt == "adaptive":
            got = _adaptive(dev, img, k, numerics)
        else:
            got = _bilateral(dev, img, k, 10.0, 30.0, numerics, guide=guide if flt == "joint" else None)
        _cpp_check(got, want, numerics, f"cpp_{flt}_{name}_k{k}")


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("k", [9, 15])
def test_joint_f32c_rounded_vs_include_cpp(dev, cppfix, cpp_inputs, k, numerics):
    """The f32 family tied to the same execution: joint_bilateral_filter_f32c on the three
    channels of float32(src) under the 3-channel guide, rounded (uint8)(v + 0.5f) with the
    addition in float32 and a truncating cast, against include/cpp's joint filter."""
    img, guide = cpp_inputs["f50"]
    h, w, _ = img.shape
    d_dst = dev.empty((h, w, 3), np.float32)
    f = vip.CudaBilateralFilter(w, h, k, numerics=numerics)
    f.joint_bilateral_filter_f32c(dev.put(img.astype(np.float32)), 3, dev.put(guide), 3, d_dst)
    v = (dev.get(d_dst) + np.float32(0.5)).astype(np.float32)
    assert np.isfinite(v).all() and v.min() >= 0 and v.max() < 256
    _cpp_check(v.astype(np.int32).astype(np.uint8), cppfix[f"cpp_joint_k{k}"], numerics, f"f32c rounded joint k{k}")
