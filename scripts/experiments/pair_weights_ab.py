"""Interleaved A/B of library builds on the three launches the shared centre-row weights
touch: C2 (bilateral r = 7, 3840 x 2160), one 2048-row slab of C5
(bilateral r = 15, 16384 wide) and the texture filter's joint bilateral (r = 4 with its
sigmas, folded tables) at 3840 x 2160.

usage: python scripts/experiments/pair_weights_ab.py [--out FILE] LIB.so LIB.so [...]

Every library is loaded into this one process through the C ABI. Per case: a 2 s settle, then
PASSES passes of LAUNCHES rounds; a round launches each library's kernel once, one after the
other on the default stream, and each kernel's own duration comes from its library's
kernel-timing recorder (include/vip.h vip_kernel_timing_*). Prints the median per pass and
library. The first library is the base the others are compared with."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from various_image_processings_amd._lib import SIGNATURES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--out", default=None)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--launches", type=int, default=60)
ap.add_argument("--settle", type=float, default=2.0)
opt = ap.parse_args()


def load(path):
    h = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in SIGNATURES.items():
        if hasattr(h, name):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
    return h


def ok(rc):
    assert rc == 0, rc


libs = [load(p) for p in opt.libs]
names = [os.path.splitext(os.path.basename(p))[0] for p in opt.libs]
torch.cuda.set_device(0)
gen = torch.Generator(device="cuda").manual_seed(1)


def frames(w, h):
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(2)] + \
        [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")]


def case(w, h, ksize, sigma_space, sigma_color, joint):
    src, guide, dst = frames(w, h)
    calls = []
    for lib in libs:
        hd = ctypes.c_void_p()
        ok(lib.vip_bilateral_create(ctypes.byref(hd), w, h, ksize, sigma_space, sigma_color, 0))
        p = w * 3
        if joint:
            calls.append(lambda lib=lib, hd=hd: ok(lib.vip_joint_bilateral_run(
                hd, src.data_ptr(), p, guide.data_ptr(), p, dst.data_ptr(), p, None)))
        else:
            calls.append(lambda lib=lib, hd=hd: ok(lib.vip_bilateral_run(hd, src.data_ptr(), p, dst.data_ptr(), p, None)))
    return calls


def medians(calls):
    """[pass][library] median kernel duration in us, and the kernel each library launched."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < opt.settle:
        for c in calls:
            c()
        torch.cuda.synchronize()
    out, kern = [], None
    for _ in range(opt.passes):
        for lib in libs:
            ok(lib.vip_kernel_timing_begin(opt.launches))
        for _ in range(opt.launches):
            for c in calls:
                c()
        torch.cuda.synchronize()
        row, kern = [], []
        for lib in libs:
            n = lib.vip_kernel_timing_end()
            assert n == opt.launches, n
            ms, name, d = ctypes.c_float(), ctypes.create_string_buffer(512), []
            for i in range(n):
                ok(lib.vip_kernel_timing_get(i, ctypes.byref(ms), name, len(name)))
                d.append(ms.value * 1e3)
            row.append(statistics.median(d))
            kern.append(name.value.decode())
        out.append(row)
    return out, kern


CASES = [("C2 bilateral r=7 3840x2160", (3840, 2160, 15, 10.0, 30.0, False)),
         ("C5 slab bilateral r=15 16384x2078", (16384, 2078, 31, 10.0, 30.0, False)),
         ("C4 JBF r=4 texture sigmas 3840x2160", (3840, 2160, 9, 4.0, 1.73205080757, True))]
lines = [f"# kernel-stamped durations (us), {opt.passes} passes of {opt.launches} launches per library, interleaved "
         f"on one stream; median per pass ({torch.cuda.get_device_name(0)})",
         "# libraries: " + ", ".join(names) + f"; differences against {names[0]}"]
for title, args in CASES:
    med, kern = medians(case(*args))
    first = len(lines)
    lines.append(f"{title}: {kern[0]}")
    assert all(k == kern[0] for k in kern), kern
    lines.append(f"{'pass':<8}" + "".join(f"{n:>12}" for n in names) + "".join(f"{n + '-' + names[0]:>18}" for n in names[1:]))
    for i, row in enumerate(med):
        lines.append(f"{i + 1:<8}" + "".join(f"{v:>12.2f}" for v in row) + "".join(f"{v - row[0]:>18.2f}" for v in row[1:]))
    base = [r[0] for r in med]
    lines.append(f"spread of {names[0]}'s medians across passes: {max(base) - min(base):.2f} us")
    for j in range(1, len(names)):
        worst = max(r[j] - r[0] for r in med)
        lines.append(f"{names[j]}: lower in every pass: {all(r[j] < r[0] for r in med)}; smallest gain {-worst:.2f} us "
                     f"({-worst / statistics.median(base) * 100:.2f} %)")
    print("\n".join(lines[first:]), flush=True)
text = "\n".join(lines) + "\n"
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
