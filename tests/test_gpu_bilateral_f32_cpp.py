"""The C++ API's self-guided f32 bilateral filter (CudaBilateralFilterF32,
include/cuda/bilateral_filter_f32.hpp), reached as tests/test_gpu_joint_conf_cpp.py reaches the C++
layer: a small program built by build() (tests/cpp/bilateral_f32_test) runs the blocking call and
the stream overload on files; its outputs must equal tests/bilateral_f32_oracle.py bit for bit (CUDA
numerics, the C++ API's profile)."""
import os
import subprocess

import numpy as np
import pytest

import bilateral_f32_oracle as bo
from oracle import oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [1, 9])
def test_cpp_calls_match_the_oracle(tmp_path, k):
    w, h, ss, sc, vr = 67, 33, 4.0, 2.0, 9.5
    f = np.random.default_rng(78).uniform(0.5, 10.0, (h, w)).astype(np.float32)
    f.tofile(tmp_path / "src.bin")
    exe = os.path.join(ROOT, "tests", "cpp", "bilateral_f32_test")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build() first"
    r = subprocess.run([exe, str(tmp_path), str(w), str(h), str(k), str(ss), str(sc), str(vr)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bilateral_f32_test OK" in r.stdout, r.stdout + r.stderr
    want = bo.bilateral(f, k, ss, sc, vr, o.CUDA).view(np.uint32)
    for name in ("dst.bin", "dst_stream.bin"):
        assert np.array_equal(np.fromfile(tmp_path / name, np.uint32).reshape(h, w), want), name
