"""CPU tests of the f32 joint bilateral filter's entry points under an f32 guide (include/vip.h
vip_bilateral_f32_run_joint, _run_rows_joint, _max_ksize_joint): what they refuse before any device
work, and their presence in every layer. No compute call is made here (there is no GPU in the CPU
suite)."""
import ctypes
import os
import re

from conftest import ROOT

INV = 10001

NAMES = {"vip_bilateral_f32_max_ksize_joint": 0, "vip_bilateral_f32_run_joint": 8,
         "vip_bilateral_f32_run_rows_joint": 12}


def _ctype(c_type):
    """The ctypes type _lib.SIGNATURES uses for a C parameter type of include/vip.h."""
    c_type = c_type.strip()
    if "*" in c_type or c_type == "vip_bilateral_f32_t":
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float}[c_type]


def test_header_prototypes_and_signatures_agree():
    from various_image_processings_amd import _lib
    text = open(os.path.join(ROOT, "include", "vip.h")).read()
    for name, nargs in NAMES.items():
        m = re.search(r"\bint %s\(([^)]*)\);" % name, text)
        assert m, name
        params = [p for p in (q.strip() for q in m.group(1).replace("\n", " ").split(",")) if p and p != "void"]
        types = [_ctype(p.rsplit(" ", 1)[0] if not p.endswith("*") else p) for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs == len(types), name
        assert list(args) == types, (name, args, types)


def test_cap():
    import various_image_processings_amd as vip
    L = vip.lib()
    cap = L.vip_bilateral_f32_max_ksize_joint()
    assert 15 <= cap <= 31 and cap % 2 == 1
    assert cap <= L.vip_bilateral_f32_max_ksize()


def test_null_handle_and_null_pointers_are_refused():
    """Before any device work. A handle needs a device (its tables live there), so the null pointers
    under a live handle are tests/test_gpu_bilateral_f32_joint.py's; here every call has a null handle,
    with null and with host pointers behind it, and must come back without touching them."""
    import various_image_processings_amd as vip
    L = vip.lib()
    assert L.vip_bilateral_f32_run_joint(None, None, 0, None, 0, None, 0, None) == INV
    assert L.vip_bilateral_f32_run_rows_joint(None, None, 0, None, 0, None, 0, 1, 0, 0, 1, None) == INV
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert L.vip_bilateral_f32_run_joint(None, p, 32, p, 32, p + 128, 32, None) == INV
    assert L.vip_bilateral_f32_run_rows_joint(None, p, 32, p, 32, p + 128, 32, 1, 0, 0, 1, None) == INV


def test_present_in_every_layer():
    import various_image_processings_amd as vip
    from various_image_processings_amd.filters import _BilateralF32Impl
    handle = ctypes.CDLL(vip.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name
    assert callable(_BilateralF32Impl.joint_bilateral_filter) and callable(_BilateralF32Impl.run_rows_joint)
    assert callable(vip.CudaBilateralFilterF32.joint_bilateral_filter)
    hdr = open(os.path.join(ROOT, "include", "cuda", "bilateral_filter_f32.hpp")).read()
    assert "void joint_bilateral_filter(const float* const d_src, const float* const d_guide, float* const d_dst) const;" in hdr
    assert re.search(r"void joint_bilateral_filter\(const float\* const d_src, const float\* const d_guide, "
                     r"float\* const d_dst,\s+void\* stream\) const;", hdr)
    csrc = os.path.join(ROOT, "various_image_processings_amd", "csrc")
    cmake = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "vip_bilateral_f32j_${unit}.hip" in cmake and "bilateral_f32_joint_test" in cmake
    assert "vip_bilateral_f32j_%.hip" in make and "BF32J_OBJS" in make and "bilateral_f32_joint_test" in make
    for arith in ("fma", "mul"):
        for part in range(4):
            assert os.path.exists(os.path.join(csrc, f"vip_bilateral_f32j_{arith}_p{part}.hip"))
    kernel = open(os.path.join(csrc, "vip_bilateral_f32j.hpp")).read()
    assert "void bilateral_f32_joint_kernel(" in kernel and "static_assert(LDS <= kLdsBudget" in kernel
