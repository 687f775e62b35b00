"""CPU checks of tests/c1_sweep.py: the default draw (seed0 = 0, counts()) of the crossing sweep
holds what the sweep exists for, so that tests/test_gpu_c1_sweep.py cannot pass by drawing nothing.
Also here: the cache of the cases' inputs and oracle outputs, which the GPU file shares (one process
pays for each oracle once)."""
import itertools

import numpy as np
import pytest

import c1_sweep as cs
from various_image_processings_amd import _lib

_cache = {}


def case(family, i, seed0=0):
    """c1_sweep.case under the library's ksize caps. The library is loaded at the first call, not when
    this module is imported: a GPU run loads it after torch, as the dev fixture does."""
    if "caps" not in _cache:
        cs.bind_caps(_lib.lib().vip_max_ksize, _lib.lib().vip_joint_f32c_max_ksize)
        _cache["caps"] = True
    return cs.case(family, i, seed0)


def inputs(c):
    key = ("in", c["family"], c["i"], c["seed0"])
    if key not in _cache:
        _cache[key] = cs.arrays(c)
    return _cache[key]


def want(c):
    """c1_sweep.want(c), computed once per process; the arrays are read-only."""
    key = ("out", c["family"], c["i"], c["seed0"])
    if key not in _cache:
        out = cs.want(c, inputs(c))
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _draw(family):
    return [case(family, i, 0) for i in range(cs.counts()[family])]


def test_counts():
    n = cs.counts()
    assert set(n) == set(cs.FAMILIES) and len(cs.FAMILIES) == 8
    assert all(n[f] == 12 for f in cs.FAMILIES if f != "joint_conf") and n["joint_conf"] == 32
    assert 96 <= sum(n.values()) <= 120  # about a hundred
    assert cs.counts(120)["gray"] == 120 and cs.counts(120)["joint_conf"] == 320


def test_caps_come_from_the_library():
    L = _lib.lib()
    case("gray", 0)
    assert cs.cap("gray", gch=0) == L.vip_max_ksize(0) and cs.cap("gray", gch=3) == L.vip_max_ksize(1)
    assert cs.cap("gray_adaptive") == L.vip_max_ksize(2) and cs.cap("gray_texture") == L.vip_max_ksize(3)
    assert cs.cap("joint_f32") == L.vip_max_ksize(1) and cs.cap("joint_conf") == L.vip_max_ksize(5)
    assert cs.cap("upsample") == cs.cap("upsample_f32c") == L.vip_max_ksize(4)
    assert [cs.cap("joint_f32c", ch) for ch in (2, 3, 4)] == [L.vip_joint_f32c_max_ksize(ch) for ch in (2, 3, 4)]
    assert cs.ksizes("gray_texture") == list(range(1, 25)) and cs.ksizes("upsample") == [1, 3, 5, 7, 9]


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_cases_are_deterministic_and_bounded(family):
    draw = _draw(family)
    assert len(draw) == cs.counts()[family]
    for i, c in enumerate(draw):
        assert c == case(family, i, 0) and c["i"] == i and c["family"] == family
        assert 0 < cs.cost(c) <= cs.COST_BOUND, c
        assert c["w"] >= 1 and c["h"] >= 1
        assert c["ksize"] in cs.ksizes(family, c["channels"], c["gch"]), c
        a, b = cs.arrays(c), cs.arrays(c)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype != np.uint8) for k in a)
    assert case(family, 0, 1) != case(family, 0, 0)  # another seed, another draw


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_default_draw_holds_every_class(family):
    draw = _draw(family)
    assert {c["profile"] for c in draw} == {0, 1}
    if family == "gray":
        assert {c["gch"] for c in draw} == {0, 1, 3}
    elif family not in ("gray_adaptive", "gray_texture"):
        assert {c["gch"] for c in draw} == {1, 3}
    if family in cs.HONOURS_PATH:
        assert {c["path"] for c in draw} == {cs.AUTO, cs.RUNTIME}
    else:
        assert {c["path"] for c in draw} == {cs.AUTO}
    ks = {c["ksize"] for c in draw}
    tops = {cs.cap(family, ch, 0) for ch in ((2, 3, 4) if family == "joint_f32c" else (0,))}
    assert 1 in ks and max(tops) in ks, ks
    if family == "gray":  # the joint forms' cap, under a guide
        assert any(c["ksize"] == cs.cap("gray", gch=1) and c["gch"] for c in draw)
    assert cs.classes(family) <= {cs.kernel_class(c) for c in draw}, \
        cs.classes(family) - {cs.kernel_class(c) for c in draw}
    if family in ("joint_f32c", "upsample_f32c"):
        assert {c["channels"] for c in draw} == {2, 3, 4}
    if family in ("upsample", "upsample_f32c"):
        assert {c["scale"] for c in draw} == {2, 4, 8}
        for s, seen in ((2, 2), (4, 4), (8, 6)):  # the residues the draw covers: all, all, six of eight
            for key in ("w", "h"):
                assert len({c[key] % s for c in draw if c["scale"] == s}) >= seen, (s, key)
    # the two sides of every switch
    sides = {q["ksize"] for q in cs.pins(family, np.random.default_rng(0)) if "ksize" in q}
    if family not in ("joint_f32c", "upsample_f32c"):  # theirs are representatives, drawn per run
        assert sides <= ks, sides - ks
    assert max(c["w"] for c in draw) > 128 and max(c["h"] for c in draw) > 64
    assert min(c["w"] for c in draw) < 64 and min(c["h"] for c in draw) < 48
    assert {c["w"] % 4 for c in draw} == {0, 1, 2, 3}
    assert {c["shape"] for c in draw} >= {"wide", "tall", "general"}
    stats = cs.F32_STATS if family in cs.F32 else cs.U8_STATS
    assert {c["stat"] for c in draw} == set(stats)
    if family == "gray_texture":
        assert sum(c["inplace"] for c in draw) == len(draw) // 4
        assert all(c["lay"]["dst"] == c["lay"]["src"] for c in draw if c["inplace"])


@pytest.mark.parametrize("family", cs.F32)
def test_default_draw_holds_every_alignment_combination(family):
    draw = _draw(family)
    if family != "joint_conf":
        seen = {tuple(v for _, v in cs.vec_flags(c)) for c in draw}
        assert seen == set(itertools.product((False, True), repeat=2))
        return
    assert sum(c["weight"] for c in draw) == len(draw) // 2
    with_w = {tuple(v for _, v in cs.vec_flags(c)) for c in draw if c["weight"]}
    without = {tuple(v for _, v in cs.vec_flags(c)) for c in draw if not c["weight"]}
    assert with_w == set(itertools.product((False, True), repeat=4))
    assert without == set(itertools.product((False, True), repeat=3))


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_layouts(family):
    for c in _draw(family):
        for name, (off, pitch, *vec) in c["lay"].items():
            if family in cs.F32 and name in ("src", "dst", "conf", "weight"):
                assert off % 4 == 0 and pitch % 4 == 0
                assert (off % 16 == 0 and pitch % 16 == 0) == vec[0], (c, name)
            else:
                assert 0 <= off <= 5
        rowbytes = {"src": c["w"] * max(1, c["channels"]) * (4 if family in cs.F32 else 1)}
        if family in ("upsample", "upsample_f32c"):
            rowbytes["src"] = -(-c["w"] // c["scale"]) * max(1, c["channels"]) * 4
        assert c["lay"]["src"][1] >= rowbytes["src"]
        assert c["lay"]["dst"][1] >= c["w"] * max(1, c["channels"]) * (4 if family in cs.F32 else 1)
    if family not in cs.F32:  # bytes: any padding 0..67
        pads = [c["lay"]["src"][1] - c["w"] for c in _draw(family)]
        assert min(pads) >= 0 and max(pads) <= 67 and len(set(pads)) > 6


@pytest.mark.parametrize("family", cs.HAS_ROWS)
def test_bands(family):
    draw = _draw(family)
    bands = [c for c in draw if c["band"]]
    assert len(bands) == len(draw) // 2
    for c in bands:
        b = c["band"]
        assert 0 <= b["row_lo"] < b["row_hi"] <= c["h"]
        assert b["row_lo"] <= b["src_row0"] and b["out_rows"] >= 1 and b["src_row0"] + b["out_rows"] <= b["row_hi"]
        assert want(c)["dst"].shape[0] == b["out_rows"]
    assert any(c["band"]["row_lo"] > 0 and c["band"]["row_hi"] < c["h"] for c in bands)
    assert any(c["path"] == cs.RUNTIME for c in bands)  # the runtime-radius kernels on a pitched band
    assert all(c["band"] is None for f in cs.FAMILIES if f not in cs.HAS_ROWS for c in _draw(f))


@pytest.mark.parametrize("family", ["upsample", "upsample_f32c"])
def test_a_case_takes_both_upsample_branches(family):
    both = [c for c in _draw(family) if want(c)["fallback"].any() and not want(c)["fallback"].all()]
    assert both, "no case with sumk == 0 at some pixels and sumk > 0 at others"


@pytest.mark.parametrize("family", cs.F32)
def test_huge_overflows_and_zeros_hold_a_negative_zero(family):
    draw = _draw(family)
    huge = [c for c in draw if c["stat"] == "huge"]
    zeros = [c for c in draw if c["stat"] == "zeros"]
    assert huge and zeros
    for c in huge:
        src = inputs(c)["src"]
        valid = inputs(c)["conf"] > 0 if family == "joint_conf" else np.ones(src.shape, bool)
        assert (np.abs(src[valid]) >= 1e37).all() and np.isfinite(src[valid]).all()
        out = want(c)["dst"]
        assert np.isinf(out).any() and not np.isnan(out).any(), c
    assert any((want(c)["dst"] == np.inf).any() and (want(c)["dst"] == -np.inf).any() for c in huge)
    for c in zeros:
        src = inputs(c)["src"]
        assert (np.signbit(src) & (src == 0)).any(), c
        assert (~np.signbit(src) & (src == 0)).any() or src.size < 4, c


def test_texture_in_place_and_u8_statistics():
    for c in _draw("gray"):
        src = inputs(c)["src"]
        assert src.dtype == np.uint8 and src.shape == (c["h"], c["w"])
        if c["stat"] == "two_level":
            assert set(np.unique(src)) <= {0, 255}
        if c["stat"] == "narrow":
            assert src.min() >= 100 and src.max() < 120
        if c["gch"]:
            assert inputs(c)["guide"].shape == (c["h"], c["w"]) + ((3,) if c["gch"] == 3 else ())
