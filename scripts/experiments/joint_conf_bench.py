"""Confidence-weighted f32 joint bilateral filter (vip_joint_bilateral_run_conf_f32) against the f32
joint filter (vip_joint_bilateral_run_f32) and against the route a caller had before it: two f32
launches, on f * c and on c, an elementwise product before and an elementwise divide after.

3840 x 2160 frame (uniform-random 8-bit guides, a uniform-random float field, a 0/1 confidence with
40 % holes), CUDA numerics, ksize 5, 15 and 31, gray and 3-channel guide: after a settle, 60 rounds
of five launches interleaved on one stream (conf without and with the weight output, the f32 filter
on f, on f * c and on c); each kernel's own duration from the kernel-timing recorder (include/vip.h
vip_kernel_timing_*); the median of each. --passes N repeats that N times and gives the median of
the pass medians and the spread (max - min) / median of the f32 filter's passes: the yardstick's own
spread, inside which a ratio is no difference. The two elementwise passes are torch kernels, which
the recorder does not see: they are timed with events around 60 back-to-back launches (so with
launch gaps, an upper bound) and shown beside the route, not inside it.
Prints a table, and with --out FILE writes it there (profiles/joint_conf_4k_ab.txt). --lib FILE loads
an alternative library build (scripts/build_object_variant.sh), --forms / --ksizes narrow the run."""
import argparse
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--launches", type=int, default=60)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--settle", type=float, default=1.0)
ap.add_argument("--ksizes", type=int, nargs="+", default=[5, 15, 31])
ap.add_argument("--forms", nargs="+", default=["gray", "rgb"])
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
guides = {"gray": (torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen), 1),
          "rgb": (torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen), 3)}
f = torch.rand((H, W), device="cuda", generator=gen) * 10
c = (torch.rand((H, W), device="cuda", generator=gen) >= 0.4).to(torch.float32)
fc = f * c
dst, wgt, num, den = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(4))
NAMES = ["conf", "conf+w", "f32(f)", "f32(fc)", "f32(c)"]


def one_pass(impl, guide, gch):
    """Median kernel duration (us) of the five launches, interleaved on the default stream, and the kernels' names."""
    calls = [lambda: impl.joint_bilateral_filter_conf_f32(f, c, guide, gch, dst, -1.0),
             lambda: impl.joint_bilateral_filter_conf_f32(f, c, guide, gch, dst, -1.0, wgt),
             lambda: impl.joint_bilateral_filter_f32(f, guide, gch, dst),
             lambda: impl.joint_bilateral_filter_f32(fc, guide, gch, num),
             lambda: impl.joint_bilateral_filter_f32(c, guide, gch, den)]
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < opt.settle:
        for call in calls:
            call()
        torch.cuda.synchronize()
    n = len(calls)
    with kernel_timing(n * opt.launches) as kt:
        for _ in range(opt.launches):
            for call in calls:
                call()
    rec = kt.records()
    assert len(rec) == n * opt.launches, len(rec)
    cols = [rec[i::n] for i in range(n)]
    assert all("joint_conf_f32" in nm for nm, _ in cols[0] + cols[1]) and all("joint_f32" in nm for nm, _ in cols[2])
    return [statistics.median(ms for _, ms in col) * 1e3 for col in cols], (cols[0][0][0], cols[2][0][0])


def elementwise():
    """us per launch of the route's product and divide, events around opt.launches back-to-back launches."""
    out = []
    for fn in (lambda: torch.mul(f, c, out=fc), lambda: torch.where(den == 0, -1.0, num / den)):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(opt.launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / opt.launches)
    return out


def fmt(v):
    return "/".join(f"{x:.1f}" for x in v)


mul_us, div_us = elementwise()
lines = [f"# confidence-weighted f32 joint bilateral against the f32 joint filter and the two-launch route, {W} x {H}, "
         f"CUDA numerics; per pass the median kernel duration of {opt.launches} launches each, five kernels interleaved "
         f"on one stream; {opt.passes} passes ({torch.cuda.get_device_name(0)}; library: {opt.lib or 'the build'})",
         f"# elementwise passes of the route (torch kernels, events around {opt.launches} launches): product "
         f"{mul_us:.1f} us, select + divide {div_us:.1f} us",
         f"{'guide':<6}{'ksize':>6}{'conf':>9}{'conf+w':>9}{'f32(f)':>9}{'route':>9}{'conf/f32':>9}{'conf+w/route':>13}"
         f"{'f32 spread':>11}  passes conf | conf+w | f32(f) | f32(fc) | f32(c) | kernels"]
for k in opt.ksizes:
    impl = _BilateralImpl(W, H, k)
    for form in opt.forms:
        guide, gch = guides[form]
        passes, names = [], None
        for _ in range(opt.passes):
            us, names = one_pass(impl, guide, gch)
            passes.append(us)
        med = [statistics.median(p[i] for p in passes) for i in range(5)]
        route = med[3] + med[4]
        spread = (max(p[2] for p in passes) - min(p[2] for p in passes)) / med[2]
        lines.append(f"{form:<6}{k:>6}{med[0]:>9.1f}{med[1]:>9.1f}{med[2]:>9.1f}{route:>9.1f}{med[0] / med[2]:>9.3f}"
                     f"{med[1] / route:>13.3f}{spread:>11.3f}  "
                     + " | ".join(fmt([p[i] for p in passes]) for i in range(5)) + f" | {names[0]} | {names[1]}")
        print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as fh:
        fh.write(text)
