"""Gray (one-channel) bilateral filter against the 3-channel filter a gray user had to run
before it existed (widen, filter, take one channel back -- only the filter is timed here).

3840 x 2160 uniform-random frame, CUDA numerics, ksize 5, 15 and 31: after a 2 s settle, 60
launches of the gray filter and 60 of the 3-channel filter of the same width, height and
ksize, interleaved on one stream; each kernel's own duration from the kernel-timing
recorder (include/vip.h vip_kernel_timing_*); the median of each. --passes N repeats that N
times and gives the median of the pass medians and every pass median. Prints a table, and
with --out FILE writes it there (profiles/gray_4k_ab.txt). --forms adds the gray-guide and
RGB-guide joint forms against the 3-channel joint filter; --numerics 1 times the C++ profile's
kernels; --lib FILE loads an alternative library build (scripts/build_*variant.sh)."""
import argparse
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--numerics", type=int, default=0)
ap.add_argument("--launches", type=int, default=60)
ap.add_argument("--passes", type=int, default=1)
ap.add_argument("--settle", type=float, default=2.0)
ap.add_argument("--ksizes", type=int, nargs="+", default=[5, 15, 31])
ap.add_argument("--forms", action="store_true")
opt = ap.parse_args()

sys.path.insert(0, ".")
if opt.lib:
    import various_image_processings_amd._lib as L
    L.LIB_PATH = opt.lib
import various_image_processings_amd as vip  # noqa: E402,F401
from various_image_processings_amd.filters import _BilateralImpl, kernel_timing  # noqa: E402

W, H = 3840, 2160
torch.cuda.set_device(0)
gen = torch.Generator(device="cuda").manual_seed(1)
g = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen)
gg = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen)
rgb = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
rgb2 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
d1 = torch.empty((H, W), dtype=torch.uint8, device="cuda")
d3 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")


def ab(impl, gray_call, rgb_call):
    """Median kernel duration (us) of the two calls, interleaved on the default stream."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < opt.settle:
        gray_call()
        rgb_call()
        torch.cuda.synchronize()
    with kernel_timing(2 * opt.launches) as kt:
        for _ in range(opt.launches):
            gray_call()
            rgb_call()
    rec = kt.records()
    assert len(rec) == 2 * opt.launches, len(rec)
    a, b = rec[0::2], rec[1::2]
    assert all("gray_" in n for n, _ in a) and not any("gray_" in n for n, _ in b), (a[0], b[0])
    return (a[0][0], statistics.median(ms for _, ms in a) * 1e3), (b[0][0], statistics.median(ms for _, ms in b) * 1e3)


def fmt(v):
    return "/".join(f"{x:.2f}" for x in v)


lines = [f"# gray vs 3-channel bilateral, {W} x {H} uniform random, numerics {opt.numerics}; per pass the median kernel "
         f"duration of {opt.launches} launches each, interleaved on one stream; {opt.passes} passes "
         f"({torch.cuda.get_device_name(0)})",
         f"{'form':<12}{'ksize':>6}{'gray us':>10}{'3ch us':>10}{'gray/3ch':>10}  gray passes | 3ch passes | kernels"]
for k in opt.ksizes:
    impl = _BilateralImpl(W, H, k, numerics=opt.numerics)
    cases = [("plain", lambda: impl.bilateral_filter_c1(g, d1), lambda: impl.bilateral_filter(rgb, d3))]
    if opt.forms and k <= 47:
        cases.append(("gray-guide", lambda: impl.joint_bilateral_filter_c1(g, gg, 1, d1),
                      lambda: impl.joint_bilateral_filter(rgb, rgb2, d3)))
        cases.append(("rgb-guide", lambda: impl.joint_bilateral_filter_c1(g, rgb2, 3, d1),
                      lambda: impl.joint_bilateral_filter(rgb, rgb2, d3)))
    for form, fg, f3 in cases:
        pg, p3 = [], []
        for _ in range(opt.passes):
            (ng, ug), (n3, u3) = ab(impl, fg, f3)
            pg.append(ug)
            p3.append(u3)
        ug, u3 = statistics.median(pg), statistics.median(p3)
        lines.append(f"{form:<12}{k:>6}{ug:>10.2f}{u3:>10.2f}{ug / u3:>10.3f}  {fmt(pg)} | {fmt(p3)} | {ng} | {n3}")
        print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
