"""CPU tests of the self-guided f32 bilateral filter's entry points (include/vip.h
vip_bilateral_f32_*): what they refuse before any device work, and their presence in every layer.
No compute call is made here (there is no GPU in the CPU suite)."""
import ctypes
import os

import pytest

from conftest import ROOT

INV, KS = 10001, 10002


def _create(L, *args):
    return L.vip_bilateral_f32_create(ctypes.byref(ctypes.c_void_p()), *args)


def test_max_ksize():
    import various_image_processings_amd as vip
    L = vip.lib()
    assert L.vip_bilateral_f32_max_ksize() == 31
    assert L.vip_max_ksize(7) == 10001  # the cap has its own function: vip_max_ksize knows no filter 7


@pytest.mark.parametrize("value_range", [0.0, -1.0, float("nan"), float("inf"), 1e-45])
def test_create_rejects_value_range(value_range):
    """0, negative, NaN and Inf are no range; 1e-45 (a subnormal) overflows scale = 1024 / value_range."""
    import various_image_processings_amd as vip
    assert _create(vip.lib(), 64, 48, 9, 10.0, 30.0, value_range, vip.VIP_NUMERICS_CUDA) == INV


def test_create_rejects_ksize_and_sizes():
    import various_image_processings_amd as vip
    L = vip.lib()
    for k in (33, 35, 0, -1, 4):
        assert _create(L, 64, 48, k, 10.0, 30.0, 255.0, vip.VIP_NUMERICS_CUDA) == KS, k
    assert _create(L, 0, 48, 9, 10.0, 30.0, 255.0, 0) == INV
    assert _create(L, 64, 0, 9, 10.0, 30.0, 255.0, 0) == INV
    assert L.vip_bilateral_f32_create(None, 64, 48, 9, 10.0, 30.0, 255.0, 0) == INV


def test_null_handle_is_refused():
    import various_image_processings_amd as vip
    L = vip.lib()
    assert L.vip_bilateral_f32_run(None, None, 0, None, 0, None) == INV
    assert L.vip_bilateral_f32_run_rows(None, None, 0, None, 0, 1, 0, 0, 1, None) == INV
    assert L.vip_bilateral_f32_destroy(None) == 0


def test_entry_points():
    import various_image_processings_amd as vip
    from various_image_processings_amd import _lib
    from various_image_processings_amd.filters import _BilateralF32Impl
    handle = ctypes.CDLL(vip.LIB_PATH)
    for name, nargs in (("vip_bilateral_f32_create", 8), ("vip_bilateral_f32_destroy", 1),
                        ("vip_bilateral_f32_run", 6), ("vip_bilateral_f32_run_rows", 10),
                        ("vip_bilateral_f32_max_ksize", 0)):
        assert hasattr(handle, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert callable(_BilateralF32Impl.bilateral_filter) and callable(_BilateralF32Impl.run_rows)
    assert callable(vip.CudaBilateralFilterF32.bilateral_filter) and vip._BilateralF32Impl is _BilateralF32Impl
    text = open(os.path.join(ROOT, "include", "vip.h")).read()
    assert "#define VIP_BILATERAL_F32_BINS 1024" in text
    hdr = open(os.path.join(ROOT, "include", "cuda", "bilateral_filter_f32.hpp")).read()
    assert "void bilateral_filter(const float* const d_src, float* const d_dst) const;" in hdr
