"""The C++ API's multi-channel f32 joint bilateral filter
(CudaBilateralFilter::joint_bilateral_filter_f32c, include/cuda/bilateral_filter.hpp), reached as
tests/test_gpu_joint_conf_cpp.py reaches its sibling: a small program built by build()
(tests/cpp/joint_f32c_test) runs the dense blocking overload on files; its output must equal
tests/f32c_oracle.py bit for bit (CUDA numerics, the C++ API's profile)."""
import os
import subprocess

import numpy as np
import pytest

import f32c_oracle as fo
from oracle import oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form", ["gray", "rgb"])
def test_cpp_blocking_overload_matches_the_oracle(tmp_path, form):
    w, h, k, ch = 67, 33, 9, 3
    f = fo.source(w, h, ch)
    rng = np.random.default_rng(77)
    guide = rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8)
    f.tofile(tmp_path / "src.bin")
    guide.tofile(tmp_path / "guide.bin")
    exe = os.path.join(ROOT, "tests", "cpp", "joint_f32c_test")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build() first"
    r = subprocess.run([exe, str(tmp_path), str(w), str(h), str(k), str(ch), "1" if form == "gray" else "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "joint_f32c_test OK" in r.stdout, r.stdout + r.stderr
    want = fo.joint_bilateral(f, guide, k, profile=o.CUDA)
    got = np.fromfile(tmp_path / "dst.bin", np.uint32).reshape(h, w, ch)
    assert np.array_equal(got, want.view(np.uint32))
