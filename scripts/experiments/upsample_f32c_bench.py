"""Multi-channel joint bilateral upsampling (vip_upsample_run_f32c) against the route a caller of an
interleaved low-resolution h x w x C float field had before it: C launches of vip_upsample_run_f32
on dense planes (the unchanged one-channel kernel is the yardstick). The de-interleave and
re-interleave passes that route also needs are not timed: the ratio is the kernels' alone.

3840 x 2160 output (uniform-random 8-bit guides, the low-resolution guide a subsample of the
full-resolution one, a uniform-random field), CUDA numerics, C = 2, 3 and 4, gray and 3-channel
guides, the cases (s, ksize) = (4, 5), (2, 5), (8, 9): after a settle, 60 rounds of the 1 + C
launches interleaved on one stream (the one multi-channel launch, then the one-channel kernel on
each plane); each kernel's own duration from the kernel-timing recorder (include/vip.h
vip_kernel_timing_*); the median of each. --passes N repeats that N times and gives the median of
the pass medians and the spread (max - min) / median of the C-launch route's passes: the
yardstick's own spread, inside which a ratio is no difference. est: the instruction-count estimate
of the ratio, (W + 1 + C) / (C * (W + 2)) with W = 4 (gray guide) or 5 (3-channel guide) VALU
instructions per tap for the weight.
Prints a table, and with --out FILE writes it there (profiles/upsample_f32c_4k_ab.txt). The waves of
each row's kernel are tests/upsample_c_oracle.py's restatement of the source's choice.
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
ap.add_argument("--cases", type=int, nargs="+", default=[4, 5, 2, 5, 8, 9], help="scale ksize pairs")
ap.add_argument("--forms", nargs="+", default=["gray", "rgb"])
ap.add_argument("--size", type=int, nargs=2, default=[3840, 2160])
opt = ap.parse_args()

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import upsample_c_oracle as uc  # noqa: E402
import various_image_processings_amd as vip  # noqa: E402,F401
from various_image_processings_amd.filters import _UpsampleImpl, kernel_timing  # noqa: E402

W, H = opt.size
torch.cuda.set_device(0)
gen = torch.Generator(device="cuda").manual_seed(1)
guides = {"gray": (torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen), 1),
          "rgb": (torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen), 3)}


def one_pass(impl, ch, src, planes, g_lo, guide, gch, dst, pdst):
    """Median kernel duration (us) of the 1 + ch launches, interleaved on the default stream, and the
    multi-channel kernel's name."""
    calls = [lambda: impl.upsample_f32c(src, ch, g_lo, guide, gch, dst)]
    for c in range(ch):
        calls.append(lambda c=c: impl.upsample_f32(planes[c], g_lo, guide, gch, pdst[c]))
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
    assert all("upsample_f32c_kernel" in nm for nm, _ in cols[0])
    assert all("upsample_f32_kernel" in nm for col in cols[1:] for nm, _ in col)
    return [statistics.median(ms for _, ms in col) * 1e3 for col in cols], cols[0][0][0]


def fmt(v):
    return "/".join(f"{x:.1f}" for x in v)


lines = [f"# multi-channel joint bilateral upsampling (one launch) against C launches of the one-channel kernel on "
         f"dense planes, {W} x {H} output, CUDA numerics; per pass the median kernel duration of {opt.launches} launches "
         f"each, 1 + C kernels interleaved on one stream; {opt.passes} passes ({torch.cuda.get_device_name(0)})",
         f"{'C':<3}{'guide':<6}{'s':>3}{'k':>3}{'waves':>6}{'f32c us':>9}{'C x f32 us':>11}{'ratio':>8}{'est':>7}"
         f"{'spread':>8}  passes f32c | C x f32 | kernel"]
for ch in opt.channels:
    for s, k in zip(opt.cases[0::2], opt.cases[1::2]):
        lw, lh = -(-W // s), -(-H // s)
        src = torch.rand((lh, lw, ch), device="cuda", generator=gen) * 10
        planes = src.permute(2, 0, 1).contiguous()
        dst = torch.empty((H, W, ch), dtype=torch.float32, device="cuda")
        pdst = torch.empty((ch, H, W), dtype=torch.float32, device="cuda")
        impl = _UpsampleImpl(W, H, s, k)
        assert (impl.low_width(), impl.low_height()) == (lw, lh)
        for form in opt.forms:
            guide, gch = guides[form]
            g_lo = guide[::s, ::s].contiguous()
            passes, name = [], None
            for _ in range(opt.passes):
                us, name = one_pass(impl, ch, src, planes, g_lo, guide, gch, dst, pdst)
                passes.append((us[0], sum(us[1:])))
            one = statistics.median(p[0] for p in passes)
            many = statistics.median(p[1] for p in passes)
            spread = (max(p[1] for p in passes) - min(p[1] for p in passes)) / many
            wv = 4 if gch == 1 else 5
            est = (wv + 1 + ch) / (ch * (wv + 2))
            lines.append(f"{ch:<3}{form:<6}{s:>3}{k:>3}{uc.waves(ch, s, k // 2, gch):>6}{one:>9.1f}{many:>11.1f}"
                         f"{one / many:>8.3f}{est:>7.2f}{spread:>8.3f}  "
                         + " | ".join(fmt([p[i] for p in passes]) for i in range(2)) + f" | {name}")
            print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as fh:
        fh.write(text)
