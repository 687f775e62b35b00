"""Gray (one-channel) bilateral filter against the 3-channel filter a gray user had to run
before it existed (widen, filter, take one channel back -- only the filter is timed here).

3840 x 2160 uniform-random frame, CUDA numerics, ksize 5, 15 and 31: after a 2 s settle, 60
launches of the gray filter and 60 of the 3-channel filter of the same width, height and
ksize, interleaved on one stream; each kernel's own duration from the kernel-timing
recorder (include/vip.h vip_kernel_timing_*); the median of each. Prints a table, and
with --out FILE writes it there (profiles/gray_4k_ab.txt). --forms adds the gray-guide and
RGB-guide joint forms against the 3-channel joint filter."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import various_image_processings_amd as vip  # noqa: E402
from various_image_processings_amd.filters import _BilateralImpl, kernel_timing  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=60)
ap.add_argument("--settle", type=float, default=2.0)
ap.add_argument("--ksizes", type=int, nargs="+", default=[5, 15, 31])
ap.add_argument("--forms", action="store_true")
opt = ap.parse_args()

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


lines = [f"# gray vs 3-channel bilateral, {W} x {H} uniform random, CUDA numerics; median kernel duration of "
         f"{opt.launches} launches each, interleaved on one stream ({torch.cuda.get_device_name(0)})",
         f"{'form':<12}{'ksize':>6}{'gray us':>10}{'3ch us':>10}{'gray/3ch':>10}  kernels"]
for k in opt.ksizes:
    impl = _BilateralImpl(W, H, k)
    cases = [("plain", lambda: impl.bilateral_filter_c1(g, d1), lambda: impl.bilateral_filter(rgb, d3))]
    if opt.forms and k <= 47:
        cases.append(("gray-guide", lambda: impl.joint_bilateral_filter_c1(g, gg, 1, d1),
                      lambda: impl.joint_bilateral_filter(rgb, rgb2, d3)))
        cases.append(("rgb-guide", lambda: impl.joint_bilateral_filter_c1(g, rgb2, 3, d1),
                      lambda: impl.joint_bilateral_filter(rgb, rgb2, d3)))
    for form, fg, f3 in cases:
        (ng, ug), (n3, u3) = ab(impl, fg, f3)
        lines.append(f"{form:<12}{k:>6}{ug:>10.2f}{u3:>10.2f}{ug / u3:>10.3f}  {ng} | {n3}")
        print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
