"""The C++ API's multi-channel f32 joint bilateral upsampling
(CudaJointBilateralUpsample::upsample_f32c, include/cuda/joint_bilateral_upsample.hpp), reached as
tests/test_gpu_joint_f32c_cpp.py reaches its sibling: a small program built by build()
(tests/cpp/upsample_f32c_test) runs the dense blocking overload on files; its output must equal
tests/upsample_c_oracle.py bit for bit (CUDA numerics, the C++ API's profile)."""
import os
import subprocess

import numpy as np
import pytest

import upsample_c_oracle as uc
import upsample_oracle as uo
from oracle import oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ch,s,form", [(2, 4, "rgb"), (3, 2, "gray"), (4, 8, "rgb")])
def test_cpp_blocking_overload_matches_the_oracle(tmp_path, ch, s, form):
    w, h, k = 67, 33, 5
    lw, lh = uo.low_size(w, h, s)
    f = uc.source(w, h, s, ch)
    rng = np.random.default_rng(77 + ch)
    tail = () if form == "gray" else (3,)
    g_lo = rng.integers(0, 256, (lh, lw) + tail, dtype=np.uint8)
    g_hi = rng.integers(0, 256, (h, w) + tail, dtype=np.uint8)
    f.tofile(tmp_path / "src_lo.bin")
    g_lo.tofile(tmp_path / "guide_lo.bin")
    g_hi.tofile(tmp_path / "guide.bin")
    exe = os.path.join(ROOT, "tests", "cpp", "upsample_f32c_test")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build() first"
    r = subprocess.run([exe, str(tmp_path), str(w), str(h), str(s), str(k), str(ch), "1" if form == "gray" else "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "upsample_f32c_test OK" in r.stdout, r.stdout + r.stderr
    want = uc.upsample(f, g_lo, g_hi, s, k, profile=o.CUDA)
    got = np.fromfile(tmp_path / "dst.bin", np.uint32).reshape(h, w, ch)
    assert np.array_equal(got, want.view(np.uint32))
