"""samples/vip_filter `texture-gray`: gray image file -> the C++ one-channel member
(CudaBilateralTextureFilter::execute_c1) -> gray image file, on lenna's channel 0 at ksize 5,
2 iterations. The output file holds the oracle's bytes (tests/gray_texture_oracle.py); a colour
file is refused."""
import os
import subprocess

import numpy as np
import pytest

import gray_texture_oracle as gto
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "samples", "vip_filter")


def _read_pgm(path):
    magic, dims, maxv, raster = open(path, "rb").read().split(b"\n", 3)
    assert magic == b"P5" and maxv == b"255", (magic, maxv)  # one channel on disk
    w, h = map(int, dims.split())
    return np.frombuffer(raster, np.uint8).reshape(h, w)


def test_vip_filter_texture_gray(tmp_path, lenna, dev):
    g = np.ascontiguousarray(lenna[..., 0])
    (tmp_path / "gray.pgm").write_bytes(b"P5\n%d %d\n255\n" % (g.shape[1], g.shape[0]) + g.tobytes())
    args = [EXE, "texture-gray", str(tmp_path / "gray.pgm"), str(tmp_path / "out.pgm"), "5", "2"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    np.testing.assert_array_equal(_read_pgm(tmp_path / "out.pgm"), gto.texture(g, 5, 2))
    # a 3-channel file is not a gray file
    (tmp_path / "rgb.ppm").write_bytes(b"P6\n512 512\n255\n" + np.ascontiguousarray(lenna).tobytes())
    args[2] = str(tmp_path / "rgb.ppm")
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not a gray" in r.stderr, (r.returncode, r.stderr)
