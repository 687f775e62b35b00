"""Multi-channel f32 joint bilateral filter (vip_joint_bilateral_run_f32c) against the route a caller
of an interleaved H x W x C float field had before it: (a) C launches of vip_joint_bilateral_run_f32
on dense planes, and (b) the same plus a de-interleave pass before and a re-interleave pass after.

3840 x 2160 frame (uniform-random 8-bit guides, a uniform-random float field), CUDA numerics, C = 2, 3
and 4, ksize 5 and 15 (and 31 at C = 2), gray and 3-channel guide: after a settle, 60 rounds of the
1 + C launches interleaved on one stream (the one multi-channel launch, then the f32 filter on each
plane); each kernel's own duration from the kernel-timing recorder (include/vip.h
vip_kernel_timing_*); the median of each. --passes N repeats that N times and gives the median of the
pass medians and the spread (max - min) / median of route (a)'s passes: the yardstick's own spread,
inside which a ratio is no difference. The two layout passes are torch copy kernels, which the
recorder does not see: they are timed with events around 60 back-to-back launches (so with launch
gaps, an upper bound) and added to (a) to give (b).
Prints a table, and with --out FILE writes it there (profiles/joint_f32c_4k_ab.txt). The waves and
LUT copies of each row's kernel are tests/f32c_oracle.py's restatement of the source's choice.
Run from the repository root."""
import argparse
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=60)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--settle", type=float, default=0.5)
ap.add_argument("--channels", type=int, nargs="+", default=[2, 3, 4])
ap.add_argument("--ksizes", type=int, nargs="+", default=[5, 15, 31])
ap.add_argument("--forms", nargs="+", default=["gray", "rgb"])
opt = ap.parse_args()

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import f32c_oracle as fo  # noqa: E402
import various_image_processings_amd as vip  # noqa: E402,F401
from various_image_processings_amd.filters import _BilateralImpl, kernel_timing  # noqa: E402

W, H = 3840, 2160
torch.cuda.set_device(0)
gen = torch.Generator(device="cuda").manual_seed(1)
guides = {"gray": (torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen), 1),
          "rgb": (torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen), 3)}


def one_pass(impl, ch, src, planes, guide, gch, dst, pdst):
    """Median kernel duration (us) of the 1 + ch launches, interleaved on the default stream, and the
    multi-channel kernel's name."""
    calls = [lambda: impl.joint_bilateral_filter_f32c(src, ch, guide, gch, dst)]
    for c in range(ch):
        calls.append(lambda c=c: impl.joint_bilateral_filter_f32(planes[c], guide, gch, pdst[c]))
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
    assert all("joint_f32c_kernel" in nm for nm, _ in cols[0]) and all("joint_f32_kernel" in nm for nm, _ in cols[1])
    return [statistics.median(ms for _, ms in col) * 1e3 for col in cols], cols[0][0][0]


def layout_passes(src, planes, dst, pdst):
    """us per launch of the de-interleave and the re-interleave, events around opt.launches launches."""
    out = []
    for fn in (lambda: planes.copy_(src.permute(2, 0, 1)), lambda: dst.copy_(pdst.permute(1, 2, 0))):
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


lines = [f"# multi-channel f32 joint bilateral (one launch) against (a) C launches of the f32 joint filter on dense "
         f"planes and (b) the same plus de-interleave and re-interleave passes, {W} x {H}, CUDA numerics; per pass the "
         f"median kernel duration of {opt.launches} launches each, 1 + C kernels interleaved on one stream; {opt.passes} "
         f"passes ({torch.cuda.get_device_name(0)}); layout passes: torch copies, events around {opt.launches} launches",
         f"{'C':<3}{'guide':<6}{'ksize':>6}{'waves':>6}{'copies':>7}{'f32c':>9}{'(a)':>9}{'layout':>9}{'(b)':>9}"
         f"{'f32c/(a)':>9}{'f32c/(b)':>9}{'(a) spread':>11}  passes f32c | (a) | de-/re-interleave | kernel"]
for ch in opt.channels:
    src = torch.rand((H, W, ch), device="cuda", generator=gen) * 10
    planes = torch.empty((ch, H, W), dtype=torch.float32, device="cuda")
    planes.copy_(src.permute(2, 0, 1))
    dst = torch.empty_like(src)
    pdst = torch.empty_like(planes)
    de_us, re_us = layout_passes(src, planes, dst, pdst)
    for k in opt.ksizes:
        if k > fo.MAX_KSIZE[ch]:
            continue
        impl = _BilateralImpl(W, H, k)
        for form in opt.forms:
            guide, gch = guides[form]
            passes, name = [], None
            for _ in range(opt.passes):
                us, name = one_pass(impl, ch, src, planes, guide, gch, dst, pdst)
                passes.append((us[0], sum(us[1:])))
            one = statistics.median(p[0] for p in passes)
            a = statistics.median(p[1] for p in passes)
            b = a + de_us + re_us
            spread = (max(p[1] for p in passes) - min(p[1] for p in passes)) / a
            waves, copies = fo.form(ch, k // 2, gch)
            lines.append(f"{ch:<3}{form:<6}{k:>6}{waves:>6}{copies:>7}{one:>9.1f}{a:>9.1f}{de_us + re_us:>9.1f}{b:>9.1f}"
                         f"{one / a:>9.3f}{one / b:>9.3f}{spread:>11.3f}  "
                         + " | ".join(fmt([p[i] for p in passes]) for i in range(2))
                         + f" | {de_us:.1f}/{re_us:.1f} | {name}")
            print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as fh:
        fh.write(text)
