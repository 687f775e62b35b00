"""CPU checks of tests/round_shapes.py: the tile heights it restates, that tall() and wide() reach
the later rounds of the persistent one-channel kernels on every CU count a gfx9 part has shipped
with, so that tests/test_gpu_c1_rounds.py is not vacuous, and the oracles' row-band entry points
against their whole-frame forms.

The conditions are on the shapes, not measurements.
"""
import math

import numpy as np
import pytest

import conf_oracle as co
import f32_oracle
import gray_adaptive_oracle as gao
import gray_oracle
import round_shapes as rs
from oracle import oracle as o

CUS = [64, 104, 128, 256, 304]
HEIGHTS = [64, 48, 32]  # every tile height of the table below
RADII = range(1, rs.MAX_RADIUS + 1)


def _height(lo, hi, th16=64, th12=48, th8=32):
    """radius -> tile height with the switches 16 | 12 waves at lo | lo + 1 and 12 | 8 at hi | hi + 1."""
    return lambda r: th16 if r <= lo else (th12 if r <= hi else th8)


def test_tile_heights():
    """The table of the kernels' tile heights; where LDS would make pick_waves choose fewer waves
    than the register caps allow, tile_rows follows pick_waves and this table would not hold."""
    for r in RADII:
        for gch in (0, 1, 3):
            assert rs.tile_rows("gray_kernel", r, gch) == 64
        assert rs.tile_rows("gray_adaptive_kernel", r, 0) == 64
        for gch in (1, 3):
            assert rs.tile_rows("upsample_f32_kernel", min(r, 4), gch) == 64
        assert rs.tile_rows("joint_f32_kernel", r, 1) == _height(12, 15)(r)
        assert rs.tile_rows("joint_f32_kernel", r, 3) == _height(9, 15)(r)
        assert rs.tile_rows("joint_conf_f32_kernel", r, 1) == _height(3, 9)(r)
        assert rs.tile_rows("joint_conf_f32_kernel", r, 3) == _height(2, 8)(r)
    assert {rs.tile_rows(k, r, g) for k in rs.KERNELS for r in RADII for g in (1, 3) if k != "upsample_f32_kernel"} \
        == set(HEIGHTS)
    with pytest.raises(ValueError):
        rs.tile_rows("joint_f32_kernel", 16, 1)
    with pytest.raises(ValueError):
        rs.tile_rows("joint_conf_f32_kernel", 3, 0)


def test_lds_arithmetic():
    """The figures the kernel sources quote for their LDS budgets (csrc/vip_joint_f32.hip:24-33,
    csrc/vip_joint_conf.hip:17-21): the restated lds_bytes and pick_waves reproduce them."""
    assert rs.lds_bytes(15, 16, 2, 256 * 32) == 156096
    assert rs.lds_bytes(12, 16, 2, 768 * 16) == 158976
    assert rs.lds_bytes(15, 12, 2, 768 * 16) == 151488
    assert rs.lds_bytes(1, 16, 2, 768 * 32) == 172224 > rs.LDS_BUDGET
    gray = [rs.pick_waves(r, 3, 16, 256 * 32) for r in RADII]
    assert gray == [16] * 4 + [12] * 7 + [8] * 4
    rgb16 = [rs.pick_waves(r, 3, 16, 768 * 16) for r in RADII]
    assert rgb16 == [16] * 2 + [12] * 6 + [8] * 5 + [4] * 2
    rgb8 = [rs.pick_waves(r, 3, 16, 768 * 8) for r in RADII]
    assert rgb8 == [16] * 7 + [12] * 5 + [8] * 3


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("th", HEIGHTS)
def test_tall(cus, th):
    w, h = rs.tall(cus, th)
    tiles, full, last = rs.rounds(w, h, th, cus)
    assert w == 9 and tiles == 2 * cus + 10
    assert full >= 2 and 0 < last < cus
    assert 0 < h % th < th                      # the last tile has fewer rows than th
    assert rs.RPW < h % th < 2 * rs.RPW         # wave 0 runs whole, wave 1 in part, the others skip
    # no vector path is on: dword loads and word stores (gray, 3-channel guide), float4 loads and stores
    assert w % 4 != 0 and (3 * w) % 4 != 0 and (4 * w) % 16 != 0


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("th", HEIGHTS)
def test_wide(cus, th):
    w, h = rs.wide(cus, th)
    cols = rs.columns(cus)
    tiles, full, last = rs.rounds(w, h, th, cus)
    assert cols == -(-w // rs.TW) and tiles == cols * -(-h // th)
    assert full >= 1 and 0 < last < cus
    assert math.gcd(cols, cus) == 1 and cols >= 3
    assert 0 < h % th < th
    assert w % rs.TW == 4                       # the last tile column is 4 pixels wide
    assert w % 4 == 0 and (3 * w) % 4 == 0 and (4 * w) % 16 == 0  # every vector path is on


def test_shapes_at_256_cus():
    """The MI355X's figures, as DESIGN.md quotes them."""
    assert rs.tall(256, 64) == (9, 33349) and rs.rounds(9, 33349, 64, 256) == (522, 2, 10)
    assert rs.tall(256, 48) == (9, 25013) and rs.tall(256, 32) == (9, 16677)
    assert rs.wide(256, 64) == (260, 6021) and rs.rounds(260, 6021, 64, 256) == (285, 1, 29)
    assert rs.wide(256, 48) == (260, 4517) and rs.wide(256, 32) == (260, 3013)
    assert rs.columns(255) == 4 and rs.wide(255, 64)[0] == 388 and rs.columns(96) == 5


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("th", HEIGHTS)
def test_band(cus, th):
    h, row_lo, row_hi, src_row0, out_rows = rs.band(cus, th)
    assert h == rs.tall(cus, th)[1]
    assert 0 < row_lo < src_row0 and src_row0 + out_rows < row_hi < h
    assert src_row0 - 2 < row_lo and src_row0 + out_rows + 2 > row_hi  # radius 2 clamps at both ends
    tiles, full, last = rs.rounds(9, out_rows, th, cus)
    assert full >= 2 and 0 < last < cus and 0 < out_rows % th < th


# ---- the oracles' row-band entry points against their whole-frame forms, 9 x 200 ----
@pytest.mark.parametrize("profile", [o.CUDA, o.CPP])
def test_band_entry_points(profile):
    w, h, k = 9, 200, 5
    rng = np.random.default_rng(9200)
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    gg = rng.integers(0, 256, (h, w), dtype=np.uint8)
    g3 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for row0, rows in ((0, 200), (1, 198), (61, 70), (199, 1)):
        cut = slice(row0, row0 + rows)
        assert np.array_equal(rs.gray_band(g, None, row0, rows, k, profile=profile),
                              gray_oracle.bilateral(g, k, profile=profile)[cut])
        for guide in (gg, g3):
            assert np.array_equal(rs.gray_band(g, guide, row0, rows, k, profile=profile),
                                  gray_oracle.joint_bilateral(g, guide, k, profile=profile)[cut])
        assert np.array_equal(rs.adaptive_band(g, row0, rows, k, profile=profile),
                              gao.adaptive(g, k, profile=profile)[cut])
    # the NumPy oracles in parallel bands: 8 bands of 25 rows, and more bands than some have halo rows
    f = np.ascontiguousarray(rng.uniform(0.5, 10.0, (h, w)), dtype=np.float32)
    c = co.confidence("holes", w, h)
    for guide in (gg, g3):
        for kk, threads in ((5, 8), (31, 8), (5, 64)):
            whole = f32_oracle.joint_bilateral(f, guide, kk, profile=profile)
            banded = rs.in_bands(lambda a, b: f32_oracle.joint_bilateral(a, b, kk, profile=profile), kk // 2, f, guide,
                                 threads=threads)
            assert np.array_equal(banded.view(np.uint32), whole.view(np.uint32))
        whole = co.joint_bilateral_conf(f, c, guide, k, profile=profile, hole_value=-1.0)
        banded = rs.in_bands(lambda a, b, d: co.joint_bilateral_conf(a, b, d, k, profile=profile, hole_value=-1.0),
                             k // 2, f, c, guide)
        assert len(banded) == 2
        for x, y in zip(banded, whole):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
