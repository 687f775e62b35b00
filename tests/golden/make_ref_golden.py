"""Regenerate tests/golden/ref_oracles.npz and tests/golden/ref_cpp_filters.npz (run in the
dev container, where the reference is present).

ref_oracles.npz: outputs of the reference tests' OWN CPU oracles, compiled where they lie
(oracle/ref_test_oracles.cpp + oracle/Makefile -> oracle/_ref/libref_test_oracles.so):

  RefAdaptiveBilateralFilterImpl   test/adaptive_bilateral_filter.cu:7-119
  RefBilateralTextureFilterImpl    test/bilateral_texture_filter.cu:8-113 (blur/rtv, guide)
  ref_gradient<T>                  test/gradient.cu:9-34
  internal::pre_compute_kernels    include/cpp/bilateral_filter.hpp:10-39 (the include/cpp LUTs)

on the reference tests' own inputs (test/random_array.hpp, seed 42, 50x50: the inputs every
gtest case of those files builds) at ksize 9 (their default) and 15, plus one 640x360 frame
through the whole texture-stage chain (gradient -> blur/rtv -> guide) and the adaptive filter,
and the adaptive filter on lenna. Small outputs are stored whole; the 640x360 and lenna ones
as sha256 digests (the oracle's REF profile regenerates them bit for bit, which is what the
CPU tests check, and the GPU tests then compare the HIP outputs with those at the
reference's own tolerances). The fixture holds data only, no reference source text.

ref_cpp_filters.npz: outputs of the reference's include/cpp CPU filters -- bilateral_filter,
joint_bilateral_filter (include/cpp/bilateral_filter.hpp), adaptive_bilateral_filter
(include/cpp/adaptive_bilateral_filter.hpp) -- compiled whole and unmodified where they lie,
over our own stand-in for OpenCV's containers (oracle/ref_cpp_filters.cpp +
oracle/cv_standin/ -> oracle/_ref/libref_cpp_filters.so): the reference's arithmetic text is
what ran, OpenCV's containers are not. They define the CPP numerics profile, so this pins
bilateral, joint bilateral (under a guide distinct from the source) and adaptive in that
profile to reference execution on whole frames, borders included: the seed-42 50x50 image
(stored whole), a 259x70 frame that crosses every tile of the 3-channel kernels, 640x360 and
lenna (sha256 digests). The joint guides are the generator's next draw after the image.
It also holds the "box-harmonic" frames (HARMONIC: made here, committed as data) with the
compiled RefAdaptiveBilateralFilterImpl's outputs on them: where that filter's offset is
exactly zero its second loop is the float-LUT bilateral loop, which pins the REF profile of
the plain bilateral filter on those pixels (offset_zero_mask).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SMALL_K = (9, 15)
# include/cpp LUT sets (ksize, sigma_space, sigma_color, colour LUT length): the bilateral
# defaults, BASELINE C2/C5, the largest ksize, a narrow sigma, and the adaptive filter's 1536
LUT_CASES = ((9, 10.0, 30.0, 768), (15, 10.0, 30.0, 768), (31, 20.0, 60.0, 768), (65, 10.0, 30.0, 768),
             (9, 4.0, 1.73205080757, 768), (15, 10.0, 30.0, 1536), (63, 10.0, 30.0, 1536))
CHAIN_K = (5, 9)
OUT = os.path.join(HERE, "ref_oracles.npz")

# ---- include/cpp filters (ref_cpp_filters.npz) ----
CPP_OUT = os.path.join(HERE, "ref_cpp_filters.npz")
SQRT3 = 1.73205080757
CPP_BILATERAL = ((9, 10.0, 30.0), (15, 10.0, 30.0), (9, 4.0, SQRT3), (31, 20.0, 60.0), (65, 10.0, 30.0))
CPP_JOINT_K = (9, 15, 47)
CPP_ADAPTIVE_K = (9, 15, 63)
# wider and taller than every tile of the 3-channel kernels (vip_stencil.hpp Geom: 64, 128 or
# 256 pixels wide, at most 16 waves x 4 = 64 rows), with a 3-pixel and a 6-row remainder
TILE_FRAME = (259, 70)
FILTERS = ("bilateral", "joint", "adaptive")
# box-harmonic frames (name, ksize, side, amplitude, seed) and the sigmas RefAdaptive ran at
HARMONIC = (("k9", 9, 40, 25, 2), ("k15", 15, 52, 25, 3), ("k31", 31, 80, 25, 2), ("k9low", 9, 52, 4, 5))
HARMONIC_SIGMAS = ((10.0, 30.0), (4.0, SQRT3))


def inputs(o):
    """The reference tests' inputs, from the oracle's generator (pinned to
    test/random_array.hpp by tests/golden/random_array_*.bin)."""
    return dict(
        img50=o.random_image(50, 50),                        # every filter test's image
        mag50=o.random_f32(2500).reshape(50, 50),            # CudaComputeBlurAndRTV magnitude
        blur50=o.random_f32(7500).reshape(50, 50, 3),        # CudaComputeGuide blurred
        rtv50=o.random_f32(2500, 1.0).reshape(50, 50),       # CudaComputeGuide rtv (max 1)
        u8c1=o.random_u8(2500).reshape(50, 50, 1), u8c3=o.random_u8(7500).reshape(50, 50, 3),
        f32c1=o.random_f32(2500).reshape(50, 50, 1), f32c3=o.random_f32(7500).reshape(50, 50, 3),
        img640=o.random_image(640, 360),
    )


def sha(a: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def compute(ref, x, lenna):
    """Every fixture entry from `ref` (the compiled reference oracles, or the oracle's REF
    profile behind the same five functions)."""
    out = {}
    for k in SMALL_K:
        out[f"adaptive_k{k}"] = ref.adaptive(x["img50"], k)
        out[f"blurred_k{k}"], out[f"rtv_k{k}"] = ref.blur_rtv(x["img50"], x["mag50"], k)
        out[f"guide_k{k}"] = ref.guide(x["blur50"], x["rtv50"], k)
    for name in ("u8c1", "u8c3", "f32c1", "f32c3"):
        out[f"gradient_{name}"] = ref.gradient(x[name])
    out["adaptive640_k9_sha256"] = sha(ref.adaptive(x["img640"], 9))
    out["adaptive_lenna_k15_sha256"] = sha(ref.adaptive(lenna, 15))
    mag = ref.gradient(x["img640"])
    out["chain640_magnitude_sha256"] = sha(mag)
    for k in CHAIN_K:
        b, r = ref.blur_rtv(x["img640"], mag, k)
        out[f"chain640_k{k}_blurred_sha256"] = sha(b)
        out[f"chain640_k{k}_rtv_sha256"] = sha(r)
        out[f"chain640_k{k}_guide_sha256"] = sha(ref.guide(b, r, k))
    return out


def bil_key(k, ss, sc):
    return f"cpp_bilateral_k{k}_s{ss:g}_c{sc:g}"


def cpp_inputs(o, lenna):
    """(image, joint guide) per frame: the guide is the second half of a draw of twice the
    length (the generator's next draw after the image), so it is distinct from the source."""
    def pair(w, h):
        both = o.random_u8(2 * w * h * 3)
        return both[:w * h * 3].reshape(h, w, 3), both[w * h * 3:].reshape(h, w, 3)
    return dict(f50=pair(50, 50), tile=pair(*TILE_FRAME), f640=pair(640, 360), lenna=(lenna, None))


def compute_cpp(f, x):
    """Every include/cpp entry from `f`: f["bilateral"](img, k, ss, sc), f["joint"](img, guide,
    k), f["adaptive"](img, k) -- the compiled include/cpp filters, or the oracle in a profile."""
    out = {}
    img, guide = x["f50"]
    for k, ss, sc in CPP_BILATERAL:
        out[bil_key(k, ss, sc)] = f["bilateral"](img, k, ss, sc)
    for k in CPP_JOINT_K:
        out[f"cpp_joint_k{k}"] = f["joint"](img, guide, k)
    for k in CPP_ADAPTIVE_K:
        out[f"cpp_adaptive_k{k}"] = f["adaptive"](img, k)
    for name, k in (("tile", 9), ("f640", 15)):
        for flt, res in cpp_frame(f, x, name, k).items():
            out[f"cpp_{flt}_{name}_k{k}_sha256"] = sha(res)
    out["cpp_bilateral_lenna_k11_sha256"] = sha(f["bilateral"](x["lenna"][0], 11, 10.0, 30.0))
    return out


def cpp_frame(f, x, name, k):
    """The three filters on the frame x[name] at ksize k, whole outputs."""
    img, guide = x[name]
    return dict(bilateral=f["bilateral"](img, k, 10.0, 30.0), joint=f["joint"](img, guide, k),
                adaptive=f["adaptive"](img, k))


def oracle_filters(o, profile, threads=8):
    """The oracle in one numerics profile behind compute_cpp's three functions."""
    def th(img):
        return threads if img.shape[0] > 100 else 1
    return dict(bilateral=lambda img, k, ss, sc: o.bilateral(img, k, ss, sc, profile=profile, threads=th(img)),
                joint=lambda img, g, k: o.joint_bilateral(img, g, k, profile=profile, threads=th(img)),
                adaptive=lambda img, k: o.adaptive(img, k, profile=profile, threads=th(img)))


def ref_filters(ref):
    """The compiled include/cpp filters (oracle/ref_test_oracles.py) behind the same functions."""
    return dict(bilateral=ref.cpp_bilateral, joint=ref.cpp_joint, adaptive=ref.cpp_adaptive)


# ---- box-harmonic frames: RefAdaptive's offset is exactly 0 on many pixels ----
def harmonic_frame(k, side, amp, seed):
    """Per channel: a constant + a small integer ramp + u[x mod k] + v[y mod k], u and v
    integer, zero-sum, non-zero at about k/3 positions shared by the three channels. Away from
    the border the k x k box sum is k^2 * (constant + ramp), so wherever u[x] = v[y] = 0 the
    box sum equals k^2 times the centre. Only main() calls this: the frames are committed."""
    rng = np.random.default_rng(seed)
    n = max(2, round(k / 3))

    def wave(pos):
        while True:
            val = rng.integers(-amp, amp + 1, n)
            val[-1] = -val[:-1].sum()
            if (val != 0).all() and abs(val[-1]) <= amp:
                out = np.zeros(k, np.int64)
                out[pos] = val
                return out

    px, py = rng.choice(k, n, replace=False), rng.choice(k, n, replace=False)
    yy, xx = np.mgrid[:side, :side]
    ramps = ((1, 0), (0, -1), (1, 1)) if side <= 52 else ((1, 0), (0, -1), (-1, 0))
    chans = []
    for a, b in ramps:
        c = a * xx + b * yy + wave(px)[xx % k] + wave(py)[yy % k]
        c += 128 - (int(c.min()) + int(c.max())) // 2
        assert c.min() >= 0 and c.max() <= 255
        chans.append(c)
    return np.stack(chans, axis=2).astype(np.uint8)


def offset_zero_mask(img, k):
    """Pixels where RefAdaptive's offset is 0.0f in all three channels: the replicate-clamped
    k x k box sum equals k^2 times the centre, in integers (the float sum is exact, < 2^24,
    and centre - sum / k^2 is 0.0f exactly when the quotient is the centre)."""
    r = k // 2
    h, w, _ = img.shape
    p = np.pad(img.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="edge")
    box = np.zeros((h, w, 3), np.int64)
    for ky in range(k):
        for kx in range(k):
            box += p[ky:ky + h, kx:kx + w]
    return (box == k * k * img.astype(np.int64)).all(axis=2)


def harm_key(name, ss, sc):
    return f"harmonic_{name}_refadaptive_s{ss:g}_c{sc:g}"


def compute_harmonic(adaptive, frames):
    """RefAdaptive outputs and offset-zero masks of the committed frames ({name: frame})."""
    out = {}
    for name, k, _, _, _ in HARMONIC:
        out[f"harmonic_{name}_mask"] = offset_zero_mask(frames[name], k)
        for ss, sc in HARMONIC_SIGMAS:
            out[harm_key(name, ss, sc)] = adaptive(frames[name], k, ss, sc)
    return out


def compute_luts(luts):
    """luts(ksize, sigma_space, sigma_color, color_len) -> (space, colour), per LUT_CASES."""
    out = {}
    for k, ss, sc, n in LUT_CASES:
        sp, co = luts(k, ss, sc, n)
        out[f"cpp_lut_space_k{k}_s{ss:g}_c{sc:g}_n{n}"] = np.asarray(sp, np.float32).reshape(k, k)
        out[f"cpp_lut_color_k{k}_s{ss:g}_c{sc:g}_n{n}"] = np.asarray(co, np.float32)
    return out


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    from oracle import oracle as o
    from oracle import ref_test_oracles as ref
    if not ref.available():
        raise SystemExit("oracle/_ref/libref_test_oracles.so missing: /root/reference not mounted?")
    lenna = np.load(os.path.join(HERE, "lenna_bgr.npz"))["bgr"]
    out = compute(ref, inputs(o), lenna)
    out.update(compute_luts(ref.cpp_luts))
    np.savez_compressed(OUT, **out)
    print("wrote", len(out), "entries to", os.path.relpath(OUT, ROOT))
    cpp = compute_cpp(ref_filters(ref), cpp_inputs(o, lenna))
    frames = {name: harmonic_frame(k, side, amp, seed) for name, k, side, amp, seed in HARMONIC}
    cpp.update({f"harmonic_{name}_frame": fr for name, fr in frames.items()})
    cpp.update(compute_harmonic(ref.adaptive, frames))
    np.savez_compressed(CPP_OUT, **cpp)
    print("wrote", len(cpp), "entries to", os.path.relpath(CPP_OUT, ROOT))


if __name__ == "__main__":
    main()
