"""CPU tests of multi-channel joint bilateral upsampling's surface (include/vip.h
vip_upsample_run_f32c): the symbol and its binding, the ksize caps the library reports,
tests/upsample_c_oracle.py against a per-pixel transcription of the definition, and the helper's
restatement of the kernels' wave counts and LDS against the committed compiler table. The GPU parity
is tests/test_gpu_upsample_f32c.py."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest

import upsample_c_oracle as uc
import upsample_oracle as uo
import various_image_processings_amd as vip
from oracle import oracle as o
from various_image_processings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_binding():
    L = _lib.lib()
    fn = L.vip_upsample_run_f32c
    c = ctypes
    # h, d_src_lo, src_pitch, channels, d_guide_lo, guide_lo_pitch, d_guide, guide_pitch, guide_channels,
    # d_dst, dst_pitch, stream
    assert fn.restype is c.c_int
    assert list(fn.argtypes) == [c.c_void_p, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p,
                                 c.c_size_t, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p]
    with open(os.path.join(ROOT, "include", "vip.h")) as fh:
        header = " ".join(fh.read().split())
    assert ("int vip_upsample_run_f32c(vip_upsample_t h, const float* d_src_lo, size_t src_pitch, int channels, "
            "const uint8_t* d_guide_lo, size_t guide_lo_pitch, const uint8_t* d_guide, size_t guide_pitch, "
            "int guide_channels, float* d_dst, size_t dst_pitch, void* stream);") in header
    # a null handle is refused before anything touches a device, whatever the channel count
    for ch in (0, 1, 2, 3, 4, 5):
        assert fn(None, None, 0, ch, None, 0, None, 0, 1, None, 0, None) == _lib.VIP_ERR_INVALID_ARGUMENT
    assert hasattr(vip.CudaJointBilateralUpsample, "upsample_f32c")


def test_ksize_caps_are_unchanged():
    L = _lib.lib()
    assert L.vip_max_ksize(vip.VIP_FILTER_UPSAMPLE) == 9 == 2 * uc.MAX_RADIUS + 1
    assert L.vip_max_ksize(7) == 10001  # no new filter id
    assert L.vip_abi_version() == 1


def _transcription(f, g_lo, g_hi, s, ksize, profile, sigma_space=1.0, sigma_color=30.0):
    """The definition as include/vip.h states it, pixel by pixel, tap by tap, channel by channel,
    with libm's fmaf."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    lh, lw, ch = f.shape
    hh, ww = g_hi.shape[:2]
    r = ksize // 2
    ws, m = uo.space_table(s, r, sigma_space, profile)
    wc = o.color_lut(768, sigma_color, profile)
    gl = g_lo.reshape(lh, lw, -1).astype(np.int64)
    gh = g_hi.reshape(hh, ww, -1).astype(np.int64)
    out = np.zeros((hh, ww, ch), np.float32)
    F = np.float32
    for y in range(hh):
        cy, py = y // s, y % s
        for x in range(ww):
            cx, px = x // s, x % s
            acc = [F(0)] * ch
            sumk = F(0)
            for ky in range(-r, r + 1):
                iy = min(max(cy + ky, 0), lh - 1)
                oy = 2 * s * ky + (s - 1) - 2 * py
                for kx in range(-r, r + 1):
                    ix = min(max(cx + kx, 0), lw - 1)
                    ox = 2 * s * kx + (s - 1) - 2 * px
                    d = int(np.abs(gl[iy, ix] - gh[y, x]).sum())
                    wgt = F(F(ws[m + oy, m + ox]) * F(wc[d]))  # once per tap
                    for c in range(ch):
                        if profile == o.CUDA:
                            acc[c] = F(libm.fmaf(float(f[iy, ix, c]), float(wgt), float(acc[c])))
                        else:
                            acc[c] = F(acc[c] + F(f[iy, ix, c] * wgt))
                    sumk = F(sumk + wgt)
            for c in range(ch):
                out[y, x, c] = f[cy, cx, c] if sumk == 0 else F(acc[c] / sumk)
    return out


@pytest.mark.parametrize("profile", [o.CUDA, o.CPP])
@pytest.mark.parametrize("gch", [1, 3])
@pytest.mark.parametrize("s", uc.SCALES)
def test_oracle_is_the_definition(s, gch, profile):
    w, h, ch, k = 11, 7, 3, 3
    lw, lh = uo.low_size(w, h, s)
    f = uc.source(w, h, s, ch)
    assert f.shape == (lh, lw, ch) and f.dtype == np.float32
    if lw * lh > 1:
        assert not any(np.array_equal(f[..., a], f[..., b]) for a in range(ch) for b in range(a))
    rng = np.random.default_rng(11 + gch + s)
    tail = () if gch == 1 else (3,)
    g_lo = rng.integers(0, 256, (lh, lw) + tail, dtype=np.uint8)
    g_hi = rng.integers(0, 256, (h, w) + tail, dtype=np.uint8)
    with np.errstate(under="ignore"):
        want = _transcription(f, g_lo, g_hi, s, k, profile)
    got = uc.upsample(f, g_lo, g_hi, s, k, profile=profile)
    assert got.shape == (h, w, ch) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (np.abs(got[..., 2]) < 1e-29).all() and (got[..., 2] != 0).any()  # the tiny channel stays tiny


def test_oracle_fallback_is_per_channel():
    """Guides 255 apart under sigma_color 1: every weight underflows, every channel returns its own
    nearest sample."""
    w, h, s, ch = 11, 7, 4, 4
    lw, lh = uo.low_size(w, h, s)
    f = uc.source(w, h, s, ch)
    got, zero = uc.upsample(f, np.zeros((lh, lw), np.uint8), np.full((h, w), 255, np.uint8), s, 5, 1.0, 1.0,
                            with_fallback=True)
    assert zero.all()
    assert np.array_equal(got.view(np.uint32), f[(np.arange(h) // s)[:, None], (np.arange(w) // s)[None, :]].view(np.uint32))


def test_geometry_matches_the_compiler_table():
    """profiles/upsample_f32c_resources.txt lists every kernel with its workgroup's waves and 0 scratch;
    upsample_c_oracle.waves() must say the same (the GPU tests size their frames by it)."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "upsample_f32c_resources.txt")) as fh:
        for ln in fh:
            m = re.match(r"upsample_f32c_kernel<(\d+), (\d+), (\d+), (\d+), (true|false)>"
                         r"\s+(\d+)\s+(\d+)\s+\d+\s+\d+\s+(\d+)\s+\d+\s+\d+\s+(\d+)\s*$", ln)
            if m:
                r, s, c, g = (int(m.group(i)) for i in (1, 2, 3, 4))
                rows[(r, s, c, g, m.group(5))] = tuple(int(m.group(i)) for i in (6, 7, 8, 9))
    want = {(r, s, c, g, fma) for r in range(uc.MAX_RADIUS + 1) for s in uc.SCALES for c in uc.CHANNELS
            for g in (1, 3) for fma in ("true", "false")}
    assert len(want) == 180 and set(rows) == want
    for (r, s, c, g, _), (waves, vgprs, scratch, denorm) in rows.items():
        assert waves == uc.waves(c, s, r, g), (r, s, c, g)
        assert scratch == 0 and denorm == 3, (r, s, c, g)
        assert vgprs <= (128 if waves == 16 else 256), (r, s, c, g)
        assert uc.lds_bytes(c, s, r, g) <= uc.LDS_BUDGET, (r, s, c, g)
        assert uc.tile_rows(c, s, r, g) == 4 * waves and uc.tile_rows(c, s, r, g) % s == 0
    # the budgets the design names
    assert uc.waves(4, 2, 4, 3) == 8 and uc.lds_bytes(4, 2, 4, 3) == 159744
    assert uc.waves(2, 2, 4, 3) == 16 and uc.lds_bytes(2, 2, 4, 3) == 159744
    assert uc.waves(3, 2, 1, 3) == 8 and uc.lds_bytes_at(3, 2, 1, 3, 16) == 167936
    assert uc.waves(3, 2, 4, 1) == 16 and uc.lds_bytes(3, 2, 4, 1) == 114688
    assert uc.waves(4, 8, 0, 3) == 16 and uc.waves(4, 2, 1, 1) == 8
    assert uc.waves(4, 4, 2, 3) == 16 and uc.waves(4, 8, 3, 1) == 8
