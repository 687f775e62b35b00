"""The C++ API's self-guided f32 bilateral filter on 2 and 3 channels
(CudaBilateralFilterF32::bilateral_filter(d_src, channels, d_dst), include/cuda/bilateral_filter_f32.hpp),
reached as tests/test_gpu_bilateral_f32_cpp.py reaches the one-channel form: a small program built by
build() (tests/cpp/bilateral_f32c_test) runs the blocking call and the stream overload on files;
its outputs must equal tests/bilateral_f32c_oracle.py bit for bit (CUDA numerics, the C++ API's
profile)."""
import os
import subprocess

import numpy as np
import pytest

import bilateral_f32c_oracle as bc
from oracle import oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ch,k", [(2, 1), (3, 9)])
def test_cpp_calls_match_the_oracle(tmp_path, ch, k):
    w, h, ss, sc, vr = 67, 33, 4.0, 2.0, 9.5 * ch
    f = np.random.default_rng(78 + ch).uniform(0.5, 10.0, (h, w, ch)).astype(np.float32)
    f.tofile(tmp_path / "src.bin")
    exe = os.path.join(ROOT, "tests", "cpp", "bilateral_f32c_test")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build() first"
    r = subprocess.run([exe, str(tmp_path), str(w), str(h), str(ch), str(k), str(ss), str(sc), str(vr)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bilateral_f32c_test OK" in r.stdout, r.stdout + r.stderr
    want = bc.bilateral(f, k, ss, sc, vr, o.CUDA).view(np.uint32)
    for name in ("dst.bin", "dst_stream.bin"):
        assert np.array_equal(np.fromfile(tmp_path / name, np.uint32).reshape(h, w, ch), want), name
