"""samples/vip_filter `gray` and `joint-gray`: gray image file -> the C++ one-channel members
(CudaBilateralFilter::bilateral_filter_c1 / joint_bilateral_filter_c1) -> gray image file,
on lenna's channel 0 at ksize 9. Every output file holds the oracle's bytes
(tests/gray_oracle.py)."""
import os
import subprocess

import numpy as np
import pytest

import gray_oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "samples", "vip_filter")


def _run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r.stdout


def _read_pgm(path):
    magic, dims, maxv, raster = open(path, "rb").read().split(b"\n", 3)
    assert magic == b"P5" and maxv == b"255", (magic, maxv)  # one channel on disk
    w, h = map(int, dims.split())
    return np.frombuffer(raster, np.uint8).reshape(h, w)


def _pgm(a):
    return b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def files(tmp_path_factory, lenna):
    d = tmp_path_factory.mktemp("vip_filter_gray")
    g = np.ascontiguousarray(lenna[..., 0])
    (d / "gray.pgm").write_bytes(_pgm(g))
    (d / "guide_gray.pgm").write_bytes(_pgm(g[:, ::-1]))  # gray guide: mirrored left-right
    (d / "guide_rgb.ppm").write_bytes(b"P6\n512 512\n255\n" + np.ascontiguousarray(lenna[..., ::-1]).tobytes())
    return d, g


def test_vip_filter_gray(files, dev):
    d, g = files
    _run([EXE, "gray", d / "gray.pgm", d / "out.pgm", 9, 10, 30])
    np.testing.assert_array_equal(_read_pgm(d / "out.pgm"), gray_oracle.bilateral(g, 9, threads=8))
    # PNG in and out: a gray PNG (colour type 0, one sample per pixel) holding the same bytes
    _run([EXE, "gray", d / "out.pgm", d / "id.png", 1])  # ksize 1: output = input
    png = (d / "id.png").read_bytes()
    assert png[24] == 8 and png[25] == 0, "8-bit gray PNG"
    _run([EXE, "gray", d / "id.png", d / "id.pgm", 1])
    np.testing.assert_array_equal(_read_pgm(d / "id.pgm"), _read_pgm(d / "out.pgm"))


@pytest.mark.parametrize("guide", ["guide_gray.pgm", "guide_rgb.ppm"])
def test_vip_filter_joint_gray(files, dev, lenna, guide):
    d, g = files
    out = d / ("joint_" + guide.split(".")[0] + ".pgm")
    _run([EXE, "joint-gray", d / "gray.pgm", d / guide, out, 9, 10, 30])
    gd = g[:, ::-1] if guide.endswith(".pgm") else lenna
    np.testing.assert_array_equal(_read_pgm(out), gray_oracle.joint_bilateral(g, gd, 9, threads=8))
