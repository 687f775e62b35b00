"""f32 joint bilateral filter (vip_joint_bilateral_run_f32) against the one-channel 8-bit joint
filter (vip_joint_bilateral_run_c1), the nearest existing kernel.

3840 x 2160 frame (uniform-random 8-bit source and guides; the f32 source is the 8-bit one as
floats, so both filters weigh the same taps), CUDA numerics, ksize 5, 15 and 31, gray and
3-channel guide: after a 2 s settle, 60 launches of each filter, interleaved on one stream;
each kernel's own duration from the kernel-timing recorder (include/vip.h vip_kernel_timing_*);
the median of each. --passes N repeats that N times and gives the median of the pass medians,
every pass median and the spread (max - min) / median of the c1 passes: a ratio inside that
spread is no difference. Prints a table, and with --out FILE writes it there
(profiles/joint_f32_4k_ab.txt). --numerics 1 times the C++ profile's kernels; --lib FILE loads
an alternative library build (scripts/build_*variant.sh)."""
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
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--settle", type=float, default=2.0)
ap.add_argument("--ksizes", type=int, nargs="+", default=[5, 15, 31])
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
f = g.to(torch.float32)
d1 = torch.empty((H, W), dtype=torch.uint8, device="cuda")
df = torch.empty((H, W), dtype=torch.float32, device="cuda")


def ab(f32_call, c1_call):
    """Median kernel duration (us) of the two calls, interleaved on the default stream."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < opt.settle:
        f32_call()
        c1_call()
        torch.cuda.synchronize()
    with kernel_timing(2 * opt.launches) as kt:
        for _ in range(opt.launches):
            f32_call()
            c1_call()
    rec = kt.records()
    assert len(rec) == 2 * opt.launches, len(rec)
    a, b = rec[0::2], rec[1::2]
    assert all("joint_f32" in n for n, _ in a) and all("gray_" in n for n, _ in b), (a[0], b[0])
    return (a[0][0], statistics.median(ms for _, ms in a) * 1e3), (b[0][0], statistics.median(ms for _, ms in b) * 1e3)


def fmt(v):
    return "/".join(f"{x:.2f}" for x in v)


lines = [f"# f32 vs one-channel 8-bit joint bilateral, {W} x {H} uniform random, numerics {opt.numerics}; per pass the "
         f"median kernel duration of {opt.launches} launches each, interleaved on one stream; {opt.passes} passes "
         f"({torch.cuda.get_device_name(0)})",
         f"{'guide':<8}{'ksize':>6}{'f32 us':>10}{'c1 us':>10}{'f32/c1':>8}{'c1 spread':>10}  "
         f"f32 passes | c1 passes | kernels"]
for k in opt.ksizes:
    impl = _BilateralImpl(W, H, k, numerics=opt.numerics)
    for form, guide, gch in (("gray", gg, 1), ("rgb", rgb, 3)):
        pf, pc = [], []
        for _ in range(opt.passes):
            (nf, uf), (nc, uc) = ab(lambda: impl.joint_bilateral_filter_f32(f, guide, gch, df),
                                    lambda: impl.joint_bilateral_filter_c1(g, guide, gch, d1))
            pf.append(uf)
            pc.append(uc)
        uf, uc = statistics.median(pf), statistics.median(pc)
        spread = (max(pc) - min(pc)) / uc
        lines.append(f"{form:<8}{k:>6}{uf:>10.2f}{uc:>10.2f}{uf / uc:>8.3f}{spread:>10.3f}  "
                     f"{fmt(pf)} | {fmt(pc)} | {nf} | {nc}")
        print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if opt.out:
    with open(opt.out, "w") as fh:
        fh.write(text)
