"""The oracle pinned to the reference's own test oracles (CPU).

tests/golden/ref_oracles.npz holds the outputs of the reference tests' CPU oracles --
RefAdaptiveBilateralFilterImpl (test/adaptive_bilateral_filter.cu:7-119),
RefBilateralTextureFilterImpl (test/bilateral_texture_filter.cu:8-113) and ref_gradient<T>
(test/gradient.cu:9-34) -- compiled from /root/reference where they lie
(oracle/ref_test_oracles.cpp, oracle/Makefile; tests/golden/make_ref_golden.py), on the
reference tests' own seed-42 inputs plus a 640x360 texture-stage chain and lenna.

Pinned here, bit for bit: the oracle's REF profile reproduces every entry; its CPP profile
reproduces the texture stages (blur/rtv, guide, the chain); the CUDA profile (what the HIP
product computes by default) equals the Ref guide and blur/rtv and stays within the
reference tests' own +-1 for the adaptive filter.

tests/golden/ref_cpp_filters.npz holds the outputs of the reference's include/cpp CPU filters
(bilateral_filter, joint_bilateral_filter, adaptive_bilateral_filter), compiled whole where
they lie over our own stand-in for OpenCV's containers (oracle/ref_cpp_filters.cpp,
oracle/cv_standin/): the reference's arithmetic text is what ran, OpenCV's containers are
not. Pinned here, bit for bit and on whole frames, borders included: the oracle's CPP profile
of bilateral, joint bilateral (guide distinct from the source) and adaptive; tests/f32_oracle.py
in the CPP profile, rounded, against the joint entries; and the REF profile of the plain
bilateral filter against the compiled RefAdaptiveBilateralFilterImpl on the pixels where that
filter's offset is exactly zero. The CUDA profile stays within the reference tests' +-1 of the
include/cpp outputs (exact shares printed).

Still unpinned, because nothing here can execute it: the CUDA profile's fma contraction
(src/*_impl.cu under nvcc), and the whole-pipeline texture filter, whose include/cpp form
calls cv::ximgproc.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_ref_golden as mrg  # noqa: E402

import f32_oracle  # noqa: E402

_REF_DIR = os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref")


class _Profile:
    """The oracle behind the five reference-oracle functions, in one numerics profile."""

    def __init__(self, o, profile):
        self.o, self.p = o, profile

    def adaptive(self, img, k):
        return self.o.adaptive(img, k, profile=self.p, threads=8 if img.shape[0] > 100 else 1)

    def blur_rtv(self, img, mag, k):
        return self.o.blur_rtv(img, mag, k, self.p)

    def guide(self, b, r, k):
        return self.o.guide(b, r, k, self.p)

    def gradient(self, x):
        return self.o.gradient(x, self.p)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "ref_oracles.npz")))


@pytest.fixture(scope="module")
def inputs(oracle):
    return mrg.inputs(oracle)


@pytest.fixture(scope="module")
def computed(oracle, inputs, lenna):
    return {p: mrg.compute(_Profile(oracle, p), inputs, lenna) for p in (oracle.REF, oracle.CPP, oracle.CUDA)}


def ulps(a, b):
    """Distance in float32 units in the last place (gtest's FLOAT_EQ allows 4)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def test_fixture_covers_every_reference_oracle(fixture):
    assert {f"adaptive_k{k}" for k in mrg.SMALL_K} <= set(fixture)
    assert {f"guide_k{k}" for k in mrg.SMALL_K} | {f"rtv_k{k}" for k in mrg.SMALL_K} <= set(fixture)
    assert {"gradient_u8c1", "gradient_u8c3", "gradient_f32c1", "gradient_f32c3"} <= set(fixture)
    assert fixture["adaptive_k9"].shape == (50, 50, 3) and fixture["guide_k15"].dtype == np.uint8


def test_cpp_profile_luts_equal_the_reference_lut_builder(oracle, fixture):
    """The CPP profile's space and colour LUTs (vipo_space_lut / vipo_color_lut) equal
    include/cpp's internal::pre_compute_kernels, compiled from the reference, bit for bit
    (bilateral 768, adaptive 1536 entries, ksize up to 65)."""
    got = mrg.compute_luts(lambda k, ss, sc, n: (oracle.space_lut(k, ss, oracle.CPP), oracle.color_lut(n, sc, oracle.CPP)))
    assert len(got) == 2 * len(mrg.LUT_CASES)
    assert [k for k in got if not np.array_equal(got[k], fixture[k])] == []


def test_ref_profile_equals_the_reference_oracles(oracle, fixture, computed):
    """Every entry -- adaptive, gradient u8/f32 x 1/3 ch, blur/rtv, guide, the 640x360 chain,
    adaptive on lenna -- bit for bit."""
    out = computed[oracle.REF]
    bad = [k for k in fixture if not k.startswith("cpp_lut") and not np.array_equal(fixture[k], out[k])]
    assert not bad, bad


def test_cpp_profile_equals_the_reference_texture_stages(oracle, fixture, computed):
    """include/cpp numerics (float epsilon, FLT_MAX seed, unfused blend) are the Ref texture
    stages' numerics: equal bit for bit, guide included -- so the oracle's
    (float)exp((double)x) equals glibc's expf (what std::exp(float) calls in the Ref guide)
    on every argument these inputs reach."""
    out = computed[oracle.CPP]
    keys = [k for k in fixture if k.startswith(("blurred", "rtv", "guide", "chain640"))]
    assert len(keys) == 2 * 3 + 1 + 3 * len(mrg.CHAIN_K)
    assert [k for k in keys if not np.array_equal(fixture[k], out[k])] == []


def test_cuda_profile_within_the_reference_tests_tolerances(oracle, fixture, computed, inputs, lenna):
    """The profile the HIP product computes by default (src/*_impl.cu numerics) against the
    Ref oracles at the tolerances the reference's own CUDA tests apply: guide exact EQ
    (test/bilateral_texture_filter.cu:283), blur/rtv and gradient FLOAT_EQ (:253-262,
    test/gradient.cu), adaptive +-1 (test/adaptive_bilateral_filter.cu:185-193)."""
    out = computed[oracle.CUDA]
    for k in mrg.SMALL_K:
        assert np.array_equal(out[f"guide_k{k}"], fixture[f"guide_k{k}"])
        assert ulps(out[f"blurred_k{k}"], fixture[f"blurred_k{k}"]).max() <= 4
        assert ulps(out[f"rtv_k{k}"], fixture[f"rtv_k{k}"]).max() <= 4
        d = np.abs(out[f"adaptive_k{k}"].astype(int) - fixture[f"adaptive_k{k}"].astype(int))
        assert d.max() <= 1
    for name in ("u8c1", "u8c3", "f32c1", "f32c3"):
        assert ulps(out[f"gradient_{name}"], fixture[f"gradient_{name}"]).max() <= 4
    # larger frames: the REF profile regenerates the Ref output (pinned above by sha256)
    for img, k in ((inputs["img640"], 9), (lenna, 15)):
        want = oracle.adaptive(img, k, profile=oracle.REF, threads=8)
        got = oracle.adaptive(img, k, profile=oracle.CUDA, threads=8)
        d = np.abs(got.astype(int) - want.astype(int))
        assert d.max() <= 1 and (d == 0).mean() > 0.9999


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref",
                                                    "libref_test_oracles.so")),
                    reason="reference test oracles not built here (the reference is not present)")
def test_fixture_is_what_the_reference_oracles_compute_now(fixture, inputs, lenna):
    """Re-derive the fixture from the compiled reference oracles: the committed file is current."""
    from oracle import ref_test_oracles as ref
    live = mrg.compute(ref, inputs, lenna)
    live.update(mrg.compute_luts(ref.cpp_luts))
    assert sorted(live) == sorted(fixture)
    assert [k for k in live if not np.array_equal(live[k], fixture[k])] == []


# ---- include/cpp filters: tests/golden/ref_cpp_filters.npz ----
@pytest.fixture(scope="module")
def cppfix():
    return dict(np.load(os.path.join(GOLDEN, "ref_cpp_filters.npz")))


@pytest.fixture(scope="module")
def cpp_inputs(oracle, lenna):
    return mrg.cpp_inputs(oracle, lenna)


@pytest.fixture(scope="module")
def cpp_computed(oracle, cpp_inputs):
    return {p: mrg.compute_cpp(mrg.oracle_filters(oracle, p), cpp_inputs) for p in (oracle.CPP, oracle.CUDA)}


def _near1(got, want, what):
    d = np.abs(got.astype(int) - want.astype(int))
    print(f"{what}: max |d| {d.max()}, exact {100 * (d == 0).mean():.4f} %")
    assert d.max() <= 1, what


def _whole(fix):
    return [k for k in fix if k.startswith("cpp_") and not k.endswith("_sha256")]


def test_cpp_fixture_covers_bilateral_joint_and_adaptive(cppfix, cpp_inputs):
    want = {mrg.bil_key(*c) for c in mrg.CPP_BILATERAL} | {f"cpp_joint_k{k}" for k in mrg.CPP_JOINT_K} \
        | {f"cpp_adaptive_k{k}" for k in mrg.CPP_ADAPTIVE_K}
    assert want == set(_whole(cppfix)) and len(want) == 11
    assert all(cppfix[k].shape == (50, 50, 3) and cppfix[k].dtype == np.uint8 for k in want)
    digests = {f"cpp_{f}_{n}_sha256" for f in mrg.FILTERS for n in ("tile_k9", "f640_k15")}
    assert digests | {"cpp_bilateral_lenna_k11_sha256"} == {k for k in cppfix if k.endswith("_sha256")}
    for name in ("f50", "tile", "f640"):  # a real guide: not the source
        img, guide = cpp_inputs[name]
        assert img.shape == guide.shape and (img != guide).mean() > 0.9
    assert cpp_inputs["tile"][0].shape == (70, 259, 3)  # > 256 wide, > 64 tall: every 3-channel tile


def test_cpp_profile_equals_the_include_cpp_filters(oracle, cppfix, cpp_computed):
    """Bilateral (ksize 9..65, three sigma pairs), joint under a distinct guide (9, 15, 47) and
    adaptive (9, 15, 63) on the 50x50 image whole, and all three on the tile-crossing frame,
    640x360 and (bilateral) lenna by sha256: the oracle's CPP profile is include/cpp, bit for bit."""
    out = cpp_computed[oracle.CPP]
    keys = [k for k in cppfix if k.startswith("cpp_")]
    assert sorted(keys) == sorted(out) and len(keys) == 18
    assert [k for k in keys if not np.array_equal(cppfix[k], out[k])] == []


def test_cuda_profile_within_1_of_the_include_cpp_filters(oracle, cppfix, cpp_inputs, cpp_computed):
    """The profile the HIP product computes by default against include/cpp execution at the
    reference tests' own tolerance for its CUDA kernels (test/bilateral_filter.cu EXPECT_NEAR
    1, test/adaptive_bilateral_filter.cu:185-193). The exact share of each case is printed
    (DESIGN.md section 2), not bounded. The larger frames compare with the CPP profile's
    outputs, which are the include/cpp ones by the digests asserted above."""
    out = cpp_computed[oracle.CUDA]
    for k in _whole(cppfix):
        _near1(out[k], cppfix[k], f"CUDA profile {k}")
    cuda, cpp = mrg.oracle_filters(oracle, oracle.CUDA), mrg.oracle_filters(oracle, oracle.CPP)
    for name, k in (("tile", 9), ("f640", 15)):
        want = mrg.cpp_frame(cpp, cpp_inputs, name, k)
        for flt, got in mrg.cpp_frame(cuda, cpp_inputs, name, k).items():
            assert np.array_equal(mrg.sha(want[flt]), cppfix[f"cpp_{flt}_{name}_k{k}_sha256"])
            _near1(got, want[flt], f"CUDA profile cpp_{flt}_{name}_k{k}")
    lenna = cpp_inputs["lenna"][0]
    want = cpp["bilateral"](lenna, 11, 10.0, 30.0)
    assert np.array_equal(mrg.sha(want), cppfix["cpp_bilateral_lenna_k11_sha256"])
    _near1(cuda["bilateral"](lenna, 11, 10.0, 30.0), want, "CUDA profile cpp_bilateral_lenna_k11")


@pytest.mark.parametrize("k", mrg.CPP_JOINT_K)
def test_f32_oracle_rounded_is_the_include_cpp_joint_filter(oracle, cppfix, cpp_inputs, k):
    """The f32 family tied to the same execution: tests/f32_oracle.py on float32(src[..., c])
    under the 3-channel guide, rounded (uint8)(v + 0.5f) with the addition in float32 and a
    truncating cast, is include/cpp's joint filter on channel c: bit for bit in the CPP
    profile (the same products and sums), within 1 in the CUDA profile (share printed)."""
    img, guide = cpp_inputs["f50"]
    want = cppfix[f"cpp_joint_k{k}"]
    for profile, name in ((oracle.CPP, "CPP"), (oracle.CUDA, "CUDA")):
        got = np.stack([f32_oracle.f2u8(f32_oracle.joint_bilateral(img[..., c].astype(np.float32), guide, k, 10.0, 30.0,
                                                                   profile) + np.float32(0.5)) for c in range(3)], axis=2)
        if profile == oracle.CPP:
            assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
        else:
            _near1(got, want, f"f32 oracle {name} profile, rounded, joint k{k}")


@pytest.mark.parametrize("name,k,side,amp,seed", mrg.HARMONIC)
def test_ref_profile_bilateral_equals_ref_adaptive_where_its_offset_is_zero(oracle, cppfix, name, k, side, amp, seed):
    """RefAdaptiveBilateralFilterImpl's second loop is the float-LUT bilateral loop at every
    pixel whose offset is 0.0f: where the clamped k x k box sum is k^2 times the centre in all
    three channels (exact in integers; the float sum stays below 2^24). The committed frames
    have many such pixels and still have content; the mask is recomputed here by that integer
    rule, not derived from the construction. Floors on the inputs: mask >= 5 % of the frame and
    >= 400 pixels; on the +-25 frames the filter changes >= 50 % of the masked pixels at
    sigma (10, 30); RefAdaptive differs from the bilateral on >= 50 % of the off-mask pixels
    (the mask matters) at the sigma pair where the offset weighs most -- at sigma_color 30 a
    +-4 frame's offsets of a few levels move few outputs, at sqrt(3) nearly all."""
    frame = cppfix[f"harmonic_{name}_frame"]
    assert frame.shape == (side, side, 3) and frame.dtype == np.uint8
    mask = mrg.offset_zero_mask(frame, k)
    assert np.array_equal(mask, cppfix[f"harmonic_{name}_mask"])
    assert mask.mean() >= 0.05 and mask.sum() >= 400, (mask.mean(), mask.sum())
    off_share = []
    for ss, sc in mrg.HARMONIC_SIGMAS:
        want = cppfix[mrg.harm_key(name, ss, sc)]
        got = oracle.bilateral(frame, k, ss, sc, profile=oracle.REF)
        changed = (want[mask] != frame[mask]).any(axis=1).mean()
        off_share.append((want[~mask] != got[~mask]).any(axis=1).mean())
        print(f"{name} sigma ({ss:g}, {sc:g}): mask {mask.sum()} px = {100 * mask.mean():.1f} %, masked pixels "
              f"changed {100 * changed:.1f} %, off-mask RefAdaptive != bilateral {100 * off_share[-1]:.1f} %")
        if amp == 25 and (ss, sc) == (10.0, 30.0):
            assert changed >= 0.5, changed
        bad = np.argwhere((want != got).any(axis=2) & mask)
        assert len(bad) == 0, (name, ss, sc, len(bad), bad[:5].tolist())
    assert max(off_share) >= 0.5, off_share


@pytest.mark.skipif(not (os.path.exists(os.path.join(_REF_DIR, "libref_cpp_filters.so"))
                         and os.path.exists(os.path.join(_REF_DIR, "libref_test_oracles.so"))),
                    reason="reference include/cpp filters not built here (the reference is not present)")
def test_cpp_fixture_is_what_the_include_cpp_filters_compute_now(cppfix, cpp_inputs):
    """Re-derive ref_cpp_filters.npz from the compiled include/cpp filters and RefAdaptive (on
    the committed harmonic frames): the committed file is current."""
    from oracle import ref_test_oracles as ref
    live = mrg.compute_cpp(mrg.ref_filters(ref), cpp_inputs)
    frames = {h[0]: cppfix[f"harmonic_{h[0]}_frame"] for h in mrg.HARMONIC}
    live.update(mrg.compute_harmonic(ref.adaptive, frames))
    live.update({f"harmonic_{n}_frame": f for n, f in frames.items()})
    assert sorted(live) == sorted(cppfix)
    assert [k for k in live if not np.array_equal(live[k], cppfix[k])] == []
