"""Self-guided f32 bilateral filter (vip_bilateral_f32_run) against the f32 joint bilateral filter
under a gray guide (vip_joint_bilateral_run_f32), the nearest existing kernel.

3840 x 2160 frame, CUDA numerics, ksize 5, 15 and 31, on two sources: uniform random (the f32
source is a uniform-random 8-bit frame as floats, value_range 255: neighbouring lanes read table
entries far apart) and smooth (a ramp plus a little noise: neighbouring lanes read the same or
adjacent entries). After a 2 s settle, 60 launches of each filter, interleaved on one stream; each
kernel's own duration from the kernel-timing recorder (include/vip.h vip_kernel_timing_*); the
median of each. --passes N repeats that N times and gives the median of the pass medians, every
pass median and the spread (max - min) / median of the joint passes: a ratio inside that spread is
no difference. Prints a table, and with --out FILE writes it there
(profiles/bilateral_f32_4k_ab.txt). --numerics 1 times the C++ profile's kernels."""
import argparse
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--numerics", type=int, default=0)
ap.add_argument("--launches", type=int, default=60)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--settle", type=float, default=2.0)
ap.add_argument("--ksizes", type=int, nargs="+", default=[5, 15, 31])
opt = ap.parse_args()

sys.path.insert(0, ".")
import various_image_processings_amd as vip  # noqa: E402,F401
from various_image_processings_amd.filters import _BilateralF32Impl, _BilateralImpl, kernel_timing  # noqa: E402

W, H = 3840, 2160
torch.cuda.set_device(0)
gen = torch.Generator(device="cuda").manual_seed(1)
g = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen)
gg = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen)
yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
sources = {
    "random": g.to(torch.float32),
    "smooth": (0.05 * xx + 0.03 * yy + torch.rand((H, W), device="cuda", generator=gen)).to(torch.float32).contiguous(),
}
df = torch.empty((H, W), dtype=torch.float32, device="cuda")
dj = torch.empty((H, W), dtype=torch.float32, device="cuda")


def ab(self_call, joint_call):
    """Median kernel duration (us) of the two calls, interleaved on the default stream."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < opt.settle:
        self_call()
        joint_call()
        torch.cuda.synchronize()
    with kernel_timing(2 * opt.launches) as kt:
        for _ in range(opt.launches):
            self_call()
            joint_call()
    rec = kt.records()
    assert len(rec) == 2 * opt.launches, len(rec)
    a, b = rec[0::2], rec[1::2]
    assert all("bilateral_f32" in n for n, _ in a) and all("joint_f32" in n for n, _ in b), (a[0], b[0])
    return (a[0][0], statistics.median(ms for _, ms in a) * 1e3), (b[0][0], statistics.median(ms for _, ms in b) * 1e3)


def fmt(v):
    return "/".join(f"{x:.2f}" for x in v)


lines = [f"# self-guided f32 bilateral vs f32 joint bilateral under a gray guide, {W} x {H}, numerics {opt.numerics}; "
         f"per pass the median kernel duration of {opt.launches} launches each, interleaved on one stream; "
         f"{opt.passes} passes ({torch.cuda.get_device_name(0)})",
         f"{'source':<8}{'ksize':>6}{'self us':>10}{'joint us':>10}{'self/joint':>11}{'joint spread':>13}  "
         f"self passes | joint passes | kernels"]
for k in opt.ksizes:
    joint = _BilateralImpl(W, H, k, numerics=opt.numerics)
    impl = _BilateralF32Impl(W, H, k, 10.0, 30.0, 255.0, opt.numerics)
    for name, f in sources.items():
        ps, pj = [], []
        for _ in range(opt.passes):
            (ns, us), (nj, uj) = ab(lambda: impl.bilateral_filter(f, df),
                                    lambda: joint.joint_bilateral_filter_f32(f, gg, 1, dj))
            ps.append(us)
            pj.append(uj)
        us, uj = statistics.median(ps), statistics.median(pj)
        spread = (max(pj) - min(pj)) / uj
        lines.append(f"{name:<8}{k:>6}{us:>10.2f}{uj:>10.2f}{us / uj:>11.3f}{spread:>13.3f}  "
                     f"{fmt(ps)} | {fmt(pj)} | {ns} | {nj}")
        print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as fh:
        fh.write(text)
