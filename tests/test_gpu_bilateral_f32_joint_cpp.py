"""The C++ API's f32 joint bilateral filter under an f32 guide
(CudaBilateralFilterF32::joint_bilateral_filter, include/cuda/bilateral_filter_f32.hpp), reached as
tests/test_gpu_bilateral_f32_cpp.py reaches the C++ layer: a small program built by build()
(tests/cpp/bilateral_f32_joint_test) runs the blocking call, the stream overload and the C ABI's
vip_bilateral_f32_run_joint on files; the C++ outputs must equal the C ABI's bit for bit, and all of
them tests/bilateral_f32_joint_oracle.py (CUDA numerics, the C++ API's profile)."""
import os
import subprocess

import numpy as np
import pytest

import bilateral_f32_joint_oracle as jo
from oracle import oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [1, 9])
def test_cpp_calls_match_the_c_abi_and_the_oracle(tmp_path, k):
    w, h, ss, sc, vr = 67, 33, 4.0, 2.0, 9.5
    rng = np.random.default_rng(79)
    f = rng.uniform(-3.0, 10.0, (h, w)).astype(np.float32)
    g = rng.uniform(0.5, 10.0, (h, w)).astype(np.float32)
    f.tofile(tmp_path / "src.bin")
    g.tofile(tmp_path / "guide.bin")
    exe = os.path.join(ROOT, "tests", "cpp", "bilateral_f32_joint_test")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build() first"
    r = subprocess.run([exe, str(tmp_path), str(w), str(h), str(k), str(ss), str(sc), str(vr)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bilateral_f32_joint_test OK" in r.stdout, r.stdout + r.stderr
    capi = np.fromfile(tmp_path / "dst_capi.bin", np.uint32).reshape(h, w)
    for name in ("dst.bin", "dst_stream.bin"):
        assert np.array_equal(np.fromfile(tmp_path / name, np.uint32).reshape(h, w), capi), name
    assert np.array_equal(capi, jo.joint(f, g, k, ss, sc, vr, o.CUDA).view(np.uint32))
