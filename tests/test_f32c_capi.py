"""CPU tests of the multi-channel f32 joint bilateral filter's surface (include/vip.h
vip_joint_bilateral_run_f32c): the ksize caps the library reports, tests/f32c_oracle.py against a
per-pixel transcription of the definition, and the helper's restatement of the kernels' wave counts
against the committed compiler table. The GPU parity is tests/test_gpu_joint_f32c.py."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest

import f32c_oracle as fo
import various_image_processings_amd as vip
from oracle import oracle as o
from various_image_processings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ksize_caps():
    L = _lib.lib()
    assert vip.VIP_FILTER_JOINT_F32C == 6
    assert [L.vip_joint_f32c_max_ksize(c) for c in range(6)] == [10001, 47, 31, 15, 15, 10001]
    assert L.vip_joint_f32c_max_ksize(-1) == 10001
    assert L.vip_max_ksize(vip.VIP_FILTER_JOINT_F32C) == 31 == vip.max_ksize(6)
    assert L.vip_max_ksize(7) == 10001
    assert fo.MAX_KSIZE == {c: L.vip_joint_f32c_max_ksize(c) for c in (1, 2, 3, 4)}


def _transcription(f, guide, ksize, profile, sigma_space=10.0, sigma_color=30.0):
    """The definition as include/vip.h states it, pixel by pixel, tap by tap, channel by channel,
    with libm's fmaf."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    h, w, ch = f.shape
    r = ksize // 2
    ws = o.space_lut(ksize, sigma_space, profile)
    wc = o.color_lut(768, sigma_color, profile)
    g = guide.reshape(h, w, -1).astype(np.int64)
    out = np.zeros((h, w, ch), np.float32)
    F = np.float32
    for y in range(h):
        for x in range(w):
            s = [F(0)] * ch
            sumk = F(0)
            for ky in range(-r, r + 1):
                for kx in range(-r, r + 1):
                    ny, nx = min(max(y + ky, 0), h - 1), min(max(x + kx, 0), w - 1)
                    d = int(np.abs(g[ny, nx] - g[y, x]).sum())
                    wgt = F(F(ws[ky + r, kx + r]) * F(wc[d]))  # once per tap
                    for c in range(ch):
                        if profile == o.CUDA:
                            s[c] = F(libm.fmaf(float(f[ny, nx, c]), float(wgt), float(s[c])))
                        else:
                            s[c] = F(s[c] + F(f[ny, nx, c] * wgt))
                    sumk = F(sumk + wgt)
            for c in range(ch):
                out[y, x, c] = F(s[c] / sumk)
    return out


@pytest.mark.parametrize("profile", [o.CUDA, o.CPP])
@pytest.mark.parametrize("gch", [1, 3])
def test_oracle_is_the_definition(profile, gch):
    w, h, ch, k = 7, 5, 3, 5
    f = fo.source(w, h, ch)
    assert f.shape == (h, w, ch) and f.dtype == np.float32
    planes = [f[..., c] for c in range(ch)]
    assert not any(np.array_equal(planes[a], planes[b]) for a in range(ch) for b in range(a))
    rng = np.random.default_rng(5 + gch)
    guide = rng.integers(0, 256, (h, w) if gch == 1 else (h, w, 3), dtype=np.uint8)
    with np.errstate(under="ignore"):
        want = _transcription(f, guide, k, profile)
    got = fo.joint_bilateral(f, guide, k, profile=profile)
    assert got.shape == (h, w, ch) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (np.abs(got[..., 2]) < 1e-29).all() and (got[..., 2] != 0).all()  # the tiny channel stays tiny


def test_source_channels_are_seeded_per_channel():
    a, b = fo.plane(9, 4, "depth", 0), fo.plane(9, 4, "depth", 3)
    assert not np.array_equal(a, b)
    f = fo.source(9, 4, 4)
    assert np.array_equal(f[..., 0], a) and np.array_equal(f[..., 3], b)
    t = fo.source(9, 4, 2, "tiny")
    assert (np.abs(t) < 1e-29).all() and not np.array_equal(t[..., 0], t[..., 1])


def test_wave_counts_match_the_compiler_table():
    """profiles/joint_f32c_resources.txt lists every kernel with its workgroup's waves and 0 scratch;
    f32c_oracle.waves() must say the same (the GPU tests size their frames by it)."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "joint_f32c_resources.txt")) as fh:
        for ln in fh:
            m = re.match(r"joint_f32c_kernel<(\d+), (\d+), (\d+), (true|false)>\s+(\d+)\s+\d+\s+\d+\s+\d+\s+(\d+)", ln)
            if m:
                r, c, g = int(m.group(1)), int(m.group(2)), int(m.group(3))
                rows[(r, c, g, m.group(4))] = (int(m.group(5)), int(m.group(6)))
    want = {(r, c, g, fma) for c in (2, 3, 4) for r in range(1, fo.MAX_KSIZE[c] // 2 + 1) for g in (1, 3)
            for fma in ("true", "false")}
    assert set(rows) == want
    for (r, c, g, _), (waves, scratch) in rows.items():
        assert waves == fo.waves(c, r, g), (r, c, g)
        assert scratch == 0, (r, c, g)
    # the budgets the design names: planes and LUT of the largest radius of 3 and 4 channels
    assert fo.form(3, 7, 1) == (8, 32) and rs_lds(3, 7, 1) == 141696
    assert fo.form(4, 7, 1) == (8, 16) and rs_lds(4, 7, 1) == 152544
    assert fo.form(4, 7, 3) == (8, 8) and rs_lds(4, 7, 3) == 160736


def rs_lds(channels, radius, gch):
    import round_shapes as rs
    waves, copies = fo.form(channels, radius, gch)
    return rs.lds_bytes(radius, waves, channels + 1, (768 if gch == 3 else 256) * copies)
