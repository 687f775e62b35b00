"""Gray (one-channel) bilateral texture filter against the 3-channel texture filter a gray user
had to run before it existed (widen to (g, g, g), filter, take one channel back -- only the
filter is timed here).

3840 x 2160 uniform-random gray frame, CUDA numerics; ksize 5 with 5 iterations (C4's parameters)
and ksize 9 with 3 (the reference's defaults). One pass: after a 2 s settle, 30 frames of the
gray filter and 30 of the 3-channel filter of the same handle on the frame (g, g, g), interleaved
on one stream; each kernel's own duration from the kernel-timing recorder (include/vip.h
vip_kernel_timing_*). Per frame the guide stage is the sum of its nitr guide kernels, the joint
stage the sum of its nitr joint bilaterals, the whole frame the sum of both; the pass figure is
the median over the frames. Three passes; the table gives the median of the three pass medians,
every pass median, and the spread (max - min) of the pass medians. Nothing is accepted or
refused here: the table is the result. Prints it, and with --out FILE writes it there
(profiles/gray_texture_4k_ab.txt)."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import various_image_processings_amd as vip  # noqa: E402,F401
from various_image_processings_amd.filters import _TextureImpl, kernel_timing  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--frames", type=int, default=30)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--settle", type=float, default=2.0)
ap.add_argument("--cases", type=int, nargs="+", default=[5, 5, 9, 3], help="ksize nitr pairs")
opt = ap.parse_args()

W, H = 3840, 2160
torch.cuda.set_device(0)
gen = torch.Generator(device="cuda").manual_seed(1)
g = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen)
rgb = g[..., None].expand(H, W, 3).contiguous()
d1 = torch.empty((H, W), dtype=torch.uint8, device="cuda")
d3 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")


def stages(rec, nitr):
    """Per frame (2 * nitr records: guide, joint, guide, joint, ...) -> [(guide us, joint us, frame us)]."""
    out = []
    for f in range(0, len(rec), 2 * nitr):
        fr = rec[f:f + 2 * nitr]
        assert all("guide" in n for n, _ in fr[0::2]) and not any("guide" in n for n, _ in fr[1::2]), fr
        gu, jo = sum(ms for _, ms in fr[0::2]) * 1e3, sum(ms for _, ms in fr[1::2]) * 1e3
        out.append((gu, jo, gu + jo))
    return out


def one_pass(impl, nitr):
    """Median per-frame stage durations (us) of the gray and the 3-channel filter, interleaved."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < opt.settle:
        impl.execute_c1(g, d1)
        impl.execute(rgb, d3)
        torch.cuda.synchronize()
    per = 2 * nitr
    with kernel_timing(2 * per * opt.frames) as kt:
        for _ in range(opt.frames):
            impl.execute_c1(g, d1)
            impl.execute(rgb, d3)
    rec = kt.records()
    assert len(rec) == 2 * per * opt.frames, len(rec)
    a = [r for f in range(0, len(rec), 2 * per) for r in rec[f:f + per]]
    b = [r for f in range(0, len(rec), 2 * per) for r in rec[f + per:f + 2 * per]]
    assert all("gray_" in n for n, _ in a) and not any("gray_" in n for n, _ in b), (a[0], b[0])
    med = lambda rows: tuple(statistics.median(r[i] for r in rows) for i in range(3))  # noqa: E731
    return med(stages(a, nitr)), med(stages(b, nitr)), f"{a[0][0]}, {a[1][0]} | {b[0][0]}, {b[1][0]}"


def fmt(v):
    return "/".join(f"{x:.1f}" for x in v)


lines = [f"# gray vs 3-channel bilateral texture filter, {W} x {H} uniform random, CUDA numerics; per pass the median "
         f"over {opt.frames} frames each of the summed kernel durations, interleaved on one stream; {opt.passes} "
         f"passes ({torch.cuda.get_device_name(0)})",
         f"{'ksize':>5}{'nitr':>5}  {'stage':<6}{'gray us':>10}{'3ch us':>10}{'gray/3ch':>10}{'gray spread':>12}"
         f"{'3ch spread':>12}  gray passes | 3ch passes"]
for k, nitr in zip(opt.cases[0::2], opt.cases[1::2]):
    impl = _TextureImpl(W, H, k, nitr)
    ug, u3, names = [], [], None
    for _ in range(opt.passes):
        a, b, names = one_pass(impl, nitr)
        ug.append(a)
        u3.append(b)
    for i, stage in enumerate(("guide", "joint", "frame")):
        pg, p3 = [u[i] for u in ug], [u[i] for u in u3]
        mg, m3 = statistics.median(pg), statistics.median(p3)
        lines.append(f"{k:>5}{nitr:>5}  {stage:<6}{mg:>10.1f}{m3:>10.1f}{mg / m3:>10.3f}{max(pg) - min(pg):>12.1f}"
                     f"{max(p3) - min(p3):>12.1f}  {fmt(pg)} | {fmt(p3)}")
        print(lines[-1], flush=True)
    lines.append(f"#     kernels: {names}")
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
