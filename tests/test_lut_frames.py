"""CPU checks of tests/lut_frames.py: the sigma finder, and that every frame reaches the colour
distances it exists for, so that tests/test_gpu_lut_forms.py is not vacuous.

Near a zero point the LUT's weights are ~1e-45 against a centre weight near 1: they cannot move
a u8 output, and a correct zero is not what the GPU tests detect. A wrong address is -- one that
reads a neighbouring table, plane words as floats, or a wrapped 16-bit product instead of the
zero -- and only a tap whose distance lies past the zero point forms such an address. Hence the
counts below: conditions on the inputs, not tolerances. They are printed (pytest -s) and copied
into DESIGN.md section 2. The conditions are stated over the k x k square, as the oracle indexes
its LUT; the kernels run over the disc, so the disc's counts are checked as well.
"""
import numpy as np
import pytest

import lut_frames as lf
from oracle import oracle as o

PROFILES = list(lf.PROFILES)

# zero point -> the sigma_color range that has it, from a scan of oracle.color_lut in steps of
# 0.005 (768 entries) and 0.002 (1536 entries); the same in both profiles
SCANNED = {(768, 26): (1.735, 1.80), (768, 27): (1.805, 1.87), (768, 31): (2.085, 2.145), (768, 32): (2.15, 2.215),
           (1536, 511): (35.368, 35.436), (1536, 512): (35.438, 35.504)}


@pytest.mark.parametrize("profile", PROFILES)
def test_finder(profile):
    for (n, target), (lo, hi) in SCANNED.items():
        s = lf.sigma_with_zero_point(n, target, profile)
        assert s == float(np.float32(s)) and lf.zero_point(n, s, profile) == target
        a, b = lf.sigma_interval(n, target, profile)
        assert lf.zero_point(n, a, profile) == target == lf.zero_point(n, b, profile)
        assert a <= lo and hi <= b and a < s < b, (n, target, a, b, s)
        print(f"profile {profile}: {n}-entry LUT, zero point {target}: sigma_color {s!r} in [{a!r}, {b!r}]")
    # the suite's fixed points
    assert lf.zero_point(1536, 30.0, profile) == 433
    assert lf.zero_point(768, 3.0 ** 0.5, profile) == 25
    with pytest.raises(ValueError):
        lf.sigma_with_zero_point(768, 768, profile)


def test_frames_are_deterministic_and_read_only():
    for f in (lf.noise_guide(), lf.blocks(), lf.two_level(), lf.two_level_noisy(), lf.lone_pixel(), lf.flat(254),
              lf.random_source(), lf.gray(lf.two_level()), *lf.blocks_batch()):
        assert f.dtype == np.uint8 and f.shape[:2] == (lf.H, lf.W) and not f.flags.writeable
    assert np.array_equal(lf.noise_guide(), 100 + np.random.default_rng(1).integers(0, 20, (lf.H, lf.W, 3)))
    assert lf.noise_guide().min() == 100 and lf.noise_guide().max() == 119
    assert set(np.unique(lf.two_level())) == {0, 255} and lf.two_level().shape == (65, 129, 3)
    assert lf.two_level_noisy().max() == 255 and lf.two_level_noisy().min() == 0
    src = lf.random_source()
    assert all(src[..., c].min() == 0 and src[..., c].max() == 255 for c in range(3))
    assert lf.two_level(257).shape == (65, 257, 3)


# the joint filter's switches: (zero points either side, the radii that switch there)
@pytest.mark.parametrize("r", [1, 6, 7])
def test_noise_guide_straddles_the_joint_switches(r):
    """Every d in [target - 4, target + 3] at least 100 times for the zero points 25 (the texture
    filter's, and radius 7's case), 26 | 27 and 31 | 32, at the smallest and the largest radius of
    the folded form and at radius 7, which has none."""
    for disc in (False, True):
        hist = lf.joint_distances(lf.noise_guide(), r, disc)
        print(f"noise_guide r={r} {'disc' if disc else 'square'}: d 21..35 -> {hist[21:36].tolist()}, "
              f"d < 8 -> {int(hist[:8].sum())}")
        for target in (25, 26, 27, 31, 32):
            win = hist[target - 4:target + 4]
            assert (win >= 100).all(), (disc, target, win.tolist())
        assert hist[:8].sum() >= 1000  # the distances whose weights show, at the switch's sigma ~ 2


@pytest.mark.parametrize("r", sorted({k // 2 for k in lf.ADAPTIVE_SWITCH_KSIZES}))
def test_blocks_straddle_the_adaptive_switch(r):
    hist, dmin = lf.adaptive_distances(lf.blocks(), r)
    disc, _ = lf.adaptive_distances(lf.blocks(), r, disc=True)
    print(f"blocks(50, 170) r={r} square: d 507..515 -> {hist[507:516].tolist()}, d > 511 -> {int(hist[512:].sum())}; "
          f"disc: {disc[507:516].tolist()}, d > 511 -> {int(disc[512:].sum())}; best tap of the worst pixel {int(dmin.max())}")
    assert (hist[507:516] >= 16).all(), hist[507:516].tolist()
    assert hist[512:].sum() >= 1000
    assert (disc[507:516] >= 1).all() and disc[512:].sum() >= 500, disc[507:516].tolist()
    assert dmin.max() <= 255  # far below the zero points 511 | 512


@pytest.mark.parametrize("w", [129, 257])
def test_two_level_frames_reach_the_last_entries(w):
    for disc in (False, True):
        h3 = lf.joint_distances(lf.two_level(w), 1, disc)
        h1 = lf.joint_distances(lf.gray(lf.two_level(w)), 1, disc)
        n3 = lf.joint_distances(lf.two_level_noisy(w), 1, disc)
        n1 = lf.joint_distances(lf.gray(lf.two_level_noisy(w)), 1, disc)
        print(f"two_level w={w} r=1 {'disc' if disc else 'square'}: d=765 -> {int(h3[765])}, gray d=255 -> {int(h1[255])}; "
              f"two_level_noisy: d >= 735 -> {int(n3[735:].sum())}, largest {int(np.flatnonzero(n3)[-1])}, "
              f"gray d >= 245 -> {int(n1[245:].sum())}, largest {int(np.flatnonzero(n1)[-1])}")
        assert h3[765] >= 1000 and h1[255] >= 1000
        assert set(np.flatnonzero(h3)) == {0, 765} and set(np.flatnonzero(h1)) == {0, 255}
        # the noisy levels spread the same taps over the LUT's last 31 (gray: 11) entries
        assert n3[735:].sum() == h3[765] and n1[245:].sum() == h1[255]
        assert np.flatnonzero(n3)[-1] >= 762 and n1[255] >= 1


@pytest.mark.parametrize("negative", [False, True])
def test_lone_pixel_reaches_the_top_of_the_adaptive_table(negative):
    for k, top3, top1 in ((15, 1526, 508), (31, 1529, 509)):
        h3, _ = lf.adaptive_distances(lf.lone_pixel(negative), k // 2, disc=True)
        h1, _ = lf.adaptive_distances(lf.gray(lf.lone_pixel(negative)), k // 2, disc=True)
        got3, got1 = int(np.flatnonzero(h3)[-1]), int(np.flatnonzero(h1)[-1])
        print(f"lone_pixel negative={negative} k={k}: largest adaptive d {got3} ({int(h3[got3])} taps), gray {got1}")
        assert got3 >= top3 and got1 >= top1
        assert h3[got3] >= k * k // 2  # every tap of the lone pixel's own window but its centre


_dist_cache = {}


def _dmin(frame, r):
    key = (frame.shape, hash(frame.tobytes()), r)
    if key not in _dist_cache:
        # a flat frame needs no loop over its k x k taps: every difference and offset is zero
        flat = (frame == frame.flat[0]).all()
        _dist_cache[key] = 0 if flat else int(lf.adaptive_distances(frame, r, disc=True)[1].max())
    return _dist_cache[key]


@pytest.mark.parametrize("profile", PROFILES)
def test_adaptive_sums_stay_positive(profile):
    """Every adaptive case of the GPU file: each output pixel has a tap of the disc whose LUT entry
    is not zero -- and whose product with the smallest spatial weight is not zero either -- so
    sumk > 0. Where no tap has a weight the reference converts a NaN to an integer, which C leaves
    undefined: such pixels are not to be tested."""
    cases = lf.adaptive_cases(profile)
    assert len(cases) >= 40
    for label, frame, k, sc in cases:
        worst = _dmin(frame, k // 2)
        zp = lf.zero_point(1536, sc, profile)
        assert worst < zp, (label, k, sc, worst, zp)
        ws = o.space_lut(k, 10.0, profile)
        wmin = np.float32(ws[ws > 0].min()) * o.color_lut(1536, sc, profile)[worst]
        assert wmin > np.float32(1e-30), (label, k, sc, worst, float(wmin))
    assert _dmin(lf.flat(255), 31) == 0 == int(lf.adaptive_distances(lf.flat(255), 2, disc=True)[1].max())


def _within_one(got, want, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: {int((d == 0).sum())} of {d.size} channels equal, largest difference {int(d.max())}")
    assert d.max() <= 1, (what, int(d.max()), np.argwhere(d > 1)[:3].tolist())


@pytest.mark.parametrize("profile", PROFILES)
def test_oracle_within_the_reference_tolerance_on_the_new_frames(oracle, profile):
    """oracle.bilateral / joint_bilateral / adaptive against float64 NumPy filters of the same
    definitions (exact exp weights, no float32 LUT) within +-1, the reference tests' tolerance
    (test/bilateral_filter.cu:58-60), on each new 3-channel frame at ksize 5."""
    k, ss = 5, 10.0
    src = lf.random_source()
    s31, s32 = (lf.sigma_with_zero_point(768, t, profile) for t in (31, 32))
    for name, guide, sc in (("noise_guide", lf.noise_guide(), s31), ("two_level_noisy", lf.two_level_noisy(), s32),
                            ("two_level", lf.two_level(), 1000.0), ("two_level_noisy", lf.two_level_noisy(), 200.0)):
        _within_one(oracle.joint_bilateral(src, guide, k, ss, sc, profile), lf.bilateral_f64(src, k, ss, sc, guide),
                    f"joint under {name}, sigma_color {sc:g}, profile {profile}")
    for name, img in (("two_level", lf.two_level()), ("two_level_noisy", lf.two_level_noisy())):
        for sc in (1000.0, 200.0):
            _within_one(oracle.bilateral(img, k, ss, sc, profile), lf.bilateral_f64(img, k, ss, sc),
                        f"bilateral of {name}, sigma_color {sc:g}, profile {profile}")
    s511 = lf.sigma_with_zero_point(1536, 511, profile)
    for name, img, sc in (("blocks", lf.blocks(), s511), ("lone_pixel", lf.lone_pixel(), 1e4),
                          ("lone_pixel negative", lf.lone_pixel(True), 1e4), ("two_level_noisy", lf.two_level_noisy(), 1000.0)):
        _within_one(oracle.adaptive(img, k, ss, sc, profile), lf.adaptive_f64(img, k, ss, sc),
                    f"adaptive of {name}, sigma_color {sc:g}, profile {profile}")
    for v in (0, 1, 254, 255):  # a flat frame comes back, from either filter
        assert np.array_equal(oracle.bilateral(lf.flat(v), k, profile=profile), lf.flat(v))
        assert np.array_equal(oracle.adaptive(lf.flat(v), k, profile=profile), lf.flat(v))
        assert np.array_equal(lf.bilateral_f64(lf.flat(v), k, ss, 30.0), lf.flat(v))
        assert np.array_equal(lf.adaptive_f64(lf.flat(v), k, ss, 30.0), lf.flat(v))
