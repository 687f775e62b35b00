"""CPU tests of the entry points of the self-guided f32 bilateral filter on 2 and 3 channels
(include/vip.h vip_bilateral_f32_run_c, _run_rows_c, _max_ksize_c): the header and the ctypes
signatures agree, the caps per channel count, what is refused before any device work, and the
presence of the feature in every layer. No compute call is made here (there is no GPU in the CPU
suite)."""
import ctypes
import os
import re

from conftest import ROOT

INV = 10001
NAMES = ("vip_bilateral_f32_max_ksize_c", "vip_bilateral_f32_run_c", "vip_bilateral_f32_run_rows_c")


def _ctype(param):
    """The ctypes type of one parameter of a prototype in include/vip.h."""
    from various_image_processings_amd import _lib
    param = param.strip()
    if "*" in param or param.split()[0] == "vip_bilateral_f32_t":
        return _lib._c_void_p
    return {"int": _lib._c_int, "size_t": _lib._c_size_t, "float": _lib._c_float}[param.split()[0]]


def test_header_and_signatures_agree():
    from various_image_processings_amd import _lib
    text = open(os.path.join(ROOT, "include", "vip.h")).read()
    for name in NAMES:
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert m, name
        params = [p for p in m.group(1).replace("\n", " ").split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib._c_int and argtypes == [_ctype(p) for p in params], name
    # the run forms are the one-channel prototypes with `int channels` after the source pitch
    for name in ("vip_bilateral_f32_run", "vip_bilateral_f32_run_rows"):
        one, many = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_c"][1]
        assert many == one[:3] + [_lib._c_int] + one[3:], name


def test_caps_per_channel_count():
    import various_image_processings_amd as vip
    L = vip.lib()
    assert [L.vip_bilateral_f32_max_ksize_c(c) for c in (-1, 0, 1, 2, 3, 4, 5)] == [0, 0, 31, 15, 15, 0, 0]
    assert L.vip_bilateral_f32_max_ksize_c(1) == L.vip_bilateral_f32_max_ksize()


def test_refused_before_any_device_work():
    import various_image_processings_amd as vip
    L = vip.lib()
    for c in (-1, 0, 4, 5):  # the channel count is looked at first; 4 channels are deliberately not offered
        assert L.vip_bilateral_f32_run_c(None, None, 0, c, None, 0, None) == INV
        assert L.vip_bilateral_f32_run_rows_c(None, None, 0, c, None, 0, 1, 0, 0, 1, None) == INV
    for c in (1, 2, 3):  # a null handle
        assert L.vip_bilateral_f32_run_c(None, None, 0, c, None, 0, None) == INV
        assert L.vip_bilateral_f32_run_rows_c(None, None, 0, c, None, 0, 1, 0, 0, 1, None) == INV


def test_entry_points():
    import various_image_processings_amd as vip
    from various_image_processings_amd.filters import _BilateralF32Impl
    handle = ctypes.CDLL(vip.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name
    assert callable(_BilateralF32Impl.bilateral_filter_c) and callable(_BilateralF32Impl.run_rows_c)
    assert callable(vip.CudaBilateralFilterF32.bilateral_filter_c)
    hdr = open(os.path.join(ROOT, "include", "cuda", "bilateral_filter_f32.hpp")).read()
    assert "void bilateral_filter(const float* const d_src, const int channels, float* const d_dst) const;" in hdr
    assert "void bilateral_filter(const float* const d_src, float* const d_dst) const;" in hdr  # unchanged
    for build_file in ("CMakeLists.txt", os.path.join("various_image_processings_amd", "csrc", "Makefile")):
        assert "vip_bilateral_f32c_" in open(os.path.join(ROOT, build_file)).read(), build_file
