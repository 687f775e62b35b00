"""The C++ API's confidence-weighted f32 joint bilateral filter
(CudaBilateralFilter::joint_bilateral_filter_conf_f32, include/cuda/bilateral_filter.hpp), reached
as tests/test_gpu_dropin.py reaches the C++ layer: a small program built by build()
(tests/cpp/joint_conf_test) runs the dense blocking overload on files; its outputs must equal
tests/conf_oracle.py bit for bit (CUDA numerics, the C++ API's profile)."""
import os
import subprocess

import numpy as np
import pytest

import conf_oracle as co
from oracle import oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form", ["gray", "rgb"])
def test_cpp_blocking_overload_matches_the_oracle(tmp_path, form):
    w, h, k, hole = 67, 33, 9, -1.0
    rng = np.random.default_rng(77)
    f = rng.uniform(0.5, 10.0, (h, w)).astype(np.float32)
    c = co.confidence("holes", w, h)
    f[c == 0] = np.nan   # a hole's source value is not read
    guide = rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8)
    f.tofile(tmp_path / "src.bin")
    c.tofile(tmp_path / "conf.bin")
    guide.tofile(tmp_path / "guide.bin")
    exe = os.path.join(ROOT, "tests", "cpp", "joint_conf_test")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build() first"
    r = subprocess.run([exe, str(tmp_path), str(w), str(h), str(k), "1" if form == "gray" else "3", str(hole)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "joint_conf_test OK" in r.stdout, r.stdout + r.stderr
    want, want_k = co.joint_bilateral_conf(f, c, guide, k, profile=o.CUDA, hole_value=hole)
    assert (want_k == 0).any() and ((c == 0) & (want_k > 0)).any()

    def load(name):
        return np.fromfile(tmp_path / name, np.uint32).reshape(h, w)

    assert np.array_equal(load("dst.bin"), want.view(np.uint32))
    assert np.array_equal(load("weight.bin"), want_k.view(np.uint32))
    assert np.array_equal(load("dst_alone.bin"), want.view(np.uint32))
