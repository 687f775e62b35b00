"""Joint bilateral upsampling (vip_upsample_run_f32) against two yardsticks from the f32 joint
filter (vip_joint_bilateral_run_f32), measured in the same run:

  same-k   the joint filter at the same ksize on a full-resolution float source: the same taps
           per output, but a full-resolution float plane to read;
  blow-up  the route a caller had before: a nearest-neighbour blow-up of the field to full
           resolution (torch.repeat_interleave, timed with stream events) followed by the joint
           filter at ksize s (k - 1) + 1, where that is <= 47.

3840 x 2160 output (uniform-random 8-bit guides, the low-resolution guide a subsample of the
full-resolution one, a uniform-random field), CUDA numerics, the cases (s, ksize) = (4, 5),
(2, 5), (8, 9), gray and 3-channel guides: after a 2 s settle, 60 launches of each kernel,
interleaved on one stream; each kernel's own duration from the kernel-timing recorder
(include/vip.h vip_kernel_timing_*); the median of each. --passes N repeats that N times and
gives the median of the pass medians, every pass median and the spread (max - min) / median of
the same-k passes: a ratio inside that spread is no difference. The HBM floor of the upsampling
kernel is the bytes it must move (4 B/px out, 1 or 3 B/px of guide, the two low-resolution planes)
over --hbm-gbs (the copy bandwidth to compare against, default 6300 GB/s: what a float4 copy
reaches on an MI355X). Prints a
table, and with --out FILE writes it there (profiles/upsample_4k_ab.txt). --numerics 1 times the
C++ profile's kernels."""
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
ap.add_argument("--hbm-gbs", type=float, default=6300.0)
ap.add_argument("--cases", type=int, nargs="+", default=[4, 5, 2, 5, 8, 9], help="scale ksize pairs")
ap.add_argument("--size", type=int, nargs=2, default=[3840, 2160])
opt = ap.parse_args()

sys.path.insert(0, ".")
import various_image_processings_amd as vip  # noqa: E402,F401
from various_image_processings_amd.filters import _BilateralImpl, _UpsampleImpl, kernel_timing  # noqa: E402

W, H = opt.size
torch.cuda.set_device(0)
gen = torch.Generator(device="cuda").manual_seed(1)
guides = {1: torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen),
          3: torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)}
full = torch.rand((H, W), dtype=torch.float32, device="cuda", generator=gen) * 10
dst = torch.empty((H, W), dtype=torch.float32, device="cuda")


def timed(calls, tags):
    """Median kernel duration (us) of each call, interleaved on the default stream."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < opt.settle:
        for c in calls:
            c()
        torch.cuda.synchronize()
    n = len(calls)
    with kernel_timing(n * opt.launches) as kt:
        for _ in range(opt.launches):
            for c in calls:
                c()
    rec = kt.records()
    assert len(rec) == n * opt.launches, len(rec)
    out = []
    for i, tag in enumerate(tags):
        mine = rec[i::n]
        assert all(tag in name for name, _ in mine), (tag, mine[0])
        out.append((mine[0][0], statistics.median(ms for _, ms in mine) * 1e3))
    return out


def blowup_us(lo, s):
    """Median duration (us) of the nearest-neighbour blow-up in torch, by stream events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(opt.launches)]
    for _ in range(5):
        lo.repeat_interleave(s, 0).repeat_interleave(s, 1)
    for a, b in ev:
        a.record()
        lo.repeat_interleave(s, 0).repeat_interleave(s, 1)
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def fmt(v):
    return "/".join(f"{x:.1f}" for x in v)


lines = [f"# joint bilateral upsampling vs the f32 joint filter, {W} x {H} output, uniform random, numerics "
         f"{opt.numerics}; per pass the median kernel duration of {opt.launches} launches each, interleaved on one "
         f"stream; {opt.passes} passes; HBM floor at {opt.hbm_gbs:.0f} GB/s ({torch.cuda.get_device_name(0)})",
         f"{'guide':<6}{'s':>3}{'k':>3}{'up us':>9}{'same-k us':>11}{'up/same':>9}{'spread':>8}{'blow k':>8}"
         f"{'blow-up us':>12}{'big-k us':>10}{'route/up':>10}{'floor us':>10}{'floor/up':>10}  "
         f"up passes | same-k passes | kernels"]
for s, k in zip(opt.cases[0::2], opt.cases[1::2]):
    lw, lh = -(-W // s), -(-H // s)
    lo = full[::s, ::s].contiguous()
    assert lo.shape == (lh, lw)
    big_k = s * (k - 1) + 1
    up = _UpsampleImpl(W, H, s, k, 1.0, 30.0, opt.numerics)
    same = _BilateralImpl(W, H, k, float(s), 30.0, numerics=opt.numerics)
    big = _BilateralImpl(W, H, big_k, float(s), 30.0, numerics=opt.numerics) if big_k <= 47 else None
    t_blow = blowup_us(lo, s)
    for gch, form in ((1, "gray"), (3, "rgb")):
        g = guides[gch]
        g_lo = g[::s, ::s].contiguous()
        calls = [lambda: up.upsample_f32(lo, g_lo, g, gch, dst),
                 lambda: same.joint_bilateral_filter_f32(full, g, gch, dst)]
        tags = ["upsample_f32_kernel", "joint_f32"]
        if big:
            calls.append(lambda: big.joint_bilateral_filter_f32(full, g, gch, dst))
            tags.append("joint_f32")
        passes = [timed(calls, tags) for _ in range(opt.passes)]
        col = [[p[i][1] for p in passes] for i in range(len(calls))]
        u_up, u_same = statistics.median(col[0]), statistics.median(col[1])
        spread = (max(col[1]) - min(col[1])) / u_same
        u_big = statistics.median(col[2]) if big else float("nan")
        floor = (W * H * (4 + gch) + lw * lh * (4 + gch)) / (opt.hbm_gbs * 1e3)
        names = " | ".join(p[0] for p in passes[0])
        lines.append(f"{form:<6}{s:>3}{k:>3}{u_up:>9.1f}{u_same:>11.1f}{u_up / u_same:>9.3f}{spread:>8.3f}"
                     f"{big_k if big else '-':>8}{t_blow:>12.1f}{u_big:>10.1f}{(t_blow + u_big) / u_up:>10.2f}"
                     f"{floor:>10.1f}{floor / u_up:>10.3f}  {fmt(col[0])} | {fmt(col[1])} | {names}")
        print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as fh:
        fh.write(text)
