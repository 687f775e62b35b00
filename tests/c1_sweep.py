"""Case generator of the crossing sweep over the one-channel and f32 kernel families. A plain helper
module (not a conftest): CPU only, it imports neither torch nor the library.

tests/test_gpu_fuzz.py crosses shape, ksize, sigmas, profile, statistics and row padding for the four
3-channel filters. This module draws the same kind of case for the eight families that came after
them, and adds what their kernels select on: the stencil path, the guide form, the channel count, the
upsampling scale, row bands, and a base offset and a pitch of its own for every array, so that each
array's "base and pitch are multiples of 16" decision is true or false independently of the others.

    case(family, i, seed0)  -> a dict of plain values, fully determined by its arguments
    arrays(c)               -> the host inputs of the case (NumPy, read-only)
    want(c)                 -> the oracle's outputs: {"dst": ..., "weight": ..., "fallback": ...}

The largest ksizes come from the library (vip_max_ksize, vip_joint_f32c_max_ksize): a test module
hands them over once with bind_caps(), so that this module need not load the library itself.

The draw is stratified, not independent: a parameter with a small set of values (profile, guide form,
path, w % 4, shape class, source statistic, the alignment combination) takes each value once in
every run of len(values) consecutive cases, in an order shuffled per run, and the first cases of a
family carry its pins() -- ksize 1, the largest ksize, the two sides of every kernel switch -- at
shuffled positions. The pairings between parameters are random. tests/test_c1_sweep.py holds the
default draw (seed0 = 0, counts()) to what it must contain.

Counts: 12 cases per family, except joint_conf: its four float arrays give 16 alignment combinations,
all of which must occur with d_weight present, and d_weight is present in half the cases: 32.
Upsampling scales are drawn 8 : 4 : 2 as 6 : 4 : 2 in twelve, and the j-th case of a scale takes the
j-th of that scale's shuffled residues for W % s and for H % s: the default draw covers every residue
at scales 2 and 4 and six of the eight at scale 8; ten times the cases cover all of them.

Cost: every case obeys cost(c) <= COST_BOUND, cost = w * h * ksize^2 * channels (output pixels for the
upsamplers; the guide stage and the 2k - 1 joint filter per iteration for the texture filter), so the
large ksizes come with thin or small frames: a large apron on a frame smaller than a tile is where
the clamps go wrong. Measured on the CPU these tests were written on (one thread): the NumPy f32
oracle runs about 23 M tap-pixels per second (87 x 76 x 2 channels at ksize 27: 0.39 s) and the
confidence oracle, with its two accumulators, about 13 M (149 x 56 at ksize 31: 0.61 s), so
COST_BOUND = 10 M keeps the dearest case under a second. The default draw's oracles take 3.6 s in
all (gray 0.20, gray_adaptive 0.04, gray_texture 0.26, joint_f32 0.19, joint_conf 2.12, joint_f32c
0.62, upsample 0.04, upsample_f32c 0.17); the C oracles of the u8 families cost next to nothing.
"""
import math
import zlib

import numpy as np

import conf_oracle
import f32_oracle
import f32c_oracle as fo
import gray_adaptive_oracle as gao
import gray_oracle
import gray_texture_oracle as gto
import round_shapes as rs
import upsample_c_oracle as uc
import upsample_oracle as uo

FAMILIES = ("gray", "gray_adaptive", "gray_texture", "joint_f32", "joint_conf", "joint_f32c", "upsample",
            "upsample_f32c")
DEFAULT_N = 12
COST_BOUND = 10_000_000  # tap-pixels per case: see the module docstring for the measurement
# include/vip.h VIP_FILTER_*
F_BILATERAL, F_JOINT, F_ADAPTIVE, F_TEXTURE, F_UPSAMPLE, F_JOINT_CONF = 0, 1, 2, 3, 4, 5
AUTO, RUNTIME = 0, 1             # VIP_PATH_*
SPECIALISED_MAX_R = rs.MAX_RADIUS  # radius-specialised kernels up to here, runtime-radius above
SAT_MAX_R = 6                    # csrc/vip_launch.hpp kSatMaxR
HONOURS_PATH = ("gray", "gray_adaptive", "gray_texture", "joint_f32")
HAS_ROWS = ("gray", "gray_adaptive", "joint_f32")
F32 = ("joint_f32", "joint_conf", "joint_f32c", "upsample", "upsample_f32c")
U8_STATS = ("uniform", "narrow", "ramp", "two_level")
F32_STATS = ("depth", "signed", "tiny", "zeros", "huge")
CONF_KINDS = ("ones", "holes", "real")
SHAPES = ("tiny", "wide", "tall", "general")

_caps = None


def bind_caps(max_ksize, f32c_max_ksize):
    """max_ksize(filter) and f32c_max_ksize(channels): the library's vip_max_ksize and
    vip_joint_f32c_max_ksize (or anything that answers as they do)."""
    global _caps
    _caps = {"gray": max_ksize(F_BILATERAL), "gray_joint": max_ksize(F_JOINT), "gray_adaptive": max_ksize(F_ADAPTIVE),
             "gray_texture": max_ksize(F_TEXTURE), "joint_f32": max_ksize(F_JOINT),
             "joint_conf": max_ksize(F_JOINT_CONF), "upsample": max_ksize(F_UPSAMPLE),
             "upsample_f32c": max_ksize(F_UPSAMPLE), **{("joint_f32c", ch): f32c_max_ksize(ch) for ch in (2, 3, 4)}}


def cap(family, channels=0, gch=1):
    """The largest ksize the family's entry point takes (by channel count for joint_f32c; the gray
    bilateral's joint forms stop below its plain form)."""
    if _caps is None:
        raise RuntimeError("c1_sweep.bind_caps() has not been called")
    if family == "joint_f32c":
        return _caps[family, channels]
    if family == "gray" and gch:
        return _caps["gray_joint"]
    return _caps[family]


def counts(n=DEFAULT_N):
    """Cases per family for a base count n (the default draw: n = 12)."""
    return {f: (n * 8 + 2) // 3 if f == "joint_conf" else n for f in FAMILIES}


def ksizes(family, channels=0, gch=1):
    """Every ksize the family accepts."""
    top = cap(family, channels, gch)
    return list(range(1, top + 1, 1 if family == "gray_texture" else 2))


# ---- the kernel classes, restated through the helper modules ----
def kernel_class(c):
    """What the launch picks for the case, as far as the helper modules restate it: a tuple that
    differs wherever another kernel, wave count or LUT form runs."""
    f, r, gch = c["family"], c["ksize"] // 2, c["gch"]
    if f in ("gray", "gray_adaptive"):
        return ("rt",) if r == 0 or r > SPECIALISED_MAX_R or c["path"] == RUNTIME else ("specialised",)
    if f == "gray_texture":  # the embedded joint filter has ksize 2k - 1: radius k - 1
        r = c["ksize"] - 1
        return ("rt",) if r == 0 or r > SPECIALISED_MAX_R or c["path"] == RUNTIME else ("specialised",)
    if f == "joint_f32":
        if r == 0 or r > SPECIALISED_MAX_R or c["path"] == RUNTIME:
            return ("rt", gch)
        return ("specialised", gch, rs.waves("joint_f32_kernel", r, gch))
    if f == "joint_conf":
        return ("k1",) if r == 0 else ("specialised", gch, rs.waves("joint_conf_f32_kernel", r, gch))
    if f == "joint_f32c":
        return ("k1",) if r == 0 else ("specialised",) + fo.form(c["channels"], r, gch)
    if f == "upsample":
        return ("scale", c["scale"])
    return ("waves", uc.waves(c["channels"], c["scale"], r, gch))


def classes(family):
    """Every kernel_class the family has (for joint_f32c: every distinct (waves, LUT copies) form)."""
    if family in ("gray", "gray_adaptive", "gray_texture"):
        return {("rt",), ("specialised",)}
    radii = range(1, SPECIALISED_MAX_R + 1)
    if family == "joint_f32":
        return {("rt", g) for g in (1, 3)} | {("specialised", g, rs.waves("joint_f32_kernel", r, g))
                                               for g in (1, 3) for r in radii}
    if family == "joint_conf":
        return {("k1",)} | {("specialised", g, rs.waves("joint_conf_f32_kernel", r, g)) for g in (1, 3) for r in radii}
    if family == "joint_f32c":
        return {("k1",)} | {("specialised",) + fo.form(ch, r, g) for ch in (2, 3, 4) for g in (1, 3)
                            for r in range(1, cap(family, ch) // 2 + 1)}
    if family == "upsample":
        return {("scale", s) for s in uo.SCALES}
    return {("waves", uc.waves(ch, s, r, g)) for ch in uc.CHANNELS for s in uc.SCALES for g in (1, 3)
            for r in range(uc.MAX_RADIUS + 1)}


def _sides(values):
    """[(r, r + 1)] wherever values[r] != values[r + 1] (values: {radius: class})."""
    rr = sorted(values)
    return [(a, b) for a, b in zip(rr, rr[1:]) if values[a] != values[b]]


def pins(family, r):
    """The cases a draw must hold whatever else it draws: a list of partial cases. r: a Generator,
    for the pins that choose a representative."""
    top_r = SPECIALISED_MAX_R
    if family == "gray":
        g = lambda: int(r.choice([1, 3]))  # noqa: E731
        return [dict(ksize=1), dict(ksize=cap(family, gch=0), gch=0), dict(ksize=cap(family, gch=1), gch=g()),
                dict(ksize=2 * top_r + 1, path=AUTO), dict(ksize=2 * top_r + 3),
                dict(ksize=2 * SAT_MAX_R + 1, gch=g(), path=AUTO), dict(ksize=2 * SAT_MAX_R + 3, gch=g(), path=AUTO)]
    if family == "gray_adaptive":
        return [dict(ksize=1), dict(ksize=cap(family)), dict(ksize=2 * top_r + 1, path=AUTO), dict(ksize=2 * top_r + 3)]
    if family == "gray_texture":  # joint radius k - 1: specialised up to k = 16
        return [dict(ksize=1), dict(ksize=cap(family)), dict(ksize=top_r + 1, path=AUTO), dict(ksize=top_r + 2)]
    if family in ("joint_f32", "joint_conf"):
        kernel = "joint_f32_kernel" if family == "joint_f32" else "joint_conf_f32_kernel"
        out = [dict(ksize=1), dict(ksize=cap(family))]
        if family == "joint_f32":
            out += [dict(ksize=2 * top_r + 1, path=AUTO), dict(ksize=2 * top_r + 3)]
        for g in (1, 3):
            for a, b in _sides({q: rs.waves(kernel, q, g) for q in range(1, top_r + 1)}):
                out += [dict(ksize=2 * a + 1, gch=g, path=AUTO), dict(ksize=2 * b + 1, gch=g, path=AUTO)]
        return out
    if family == "joint_f32c":
        reps = {}
        for ch in (2, 3, 4):
            for g in (1, 3):
                for q in range(1, cap(family, ch) // 2 + 1):
                    reps.setdefault(fo.form(ch, q, g), []).append(dict(ksize=2 * q + 1, channels=ch, gch=g))
        g = int(r.choice([1, 3]))
        out = [dict(ksize=1), dict(ksize=cap(family, 2), channels=2, gch=g)]
        done = {fo.form(2, cap(family, 2) // 2, g)}
        for form in sorted(reps):
            if form not in done:  # one representative of every (waves, copies) form, preferring a switch's side
                side = [p for p in reps[form] if p["ksize"] in fo.switch_ksizes(p["channels"], p["gch"])]
                pool = side or reps[form]
                out.append(pool[int(r.integers(len(pool)))])
        return out
    if family == "upsample":
        return [dict(ksize=1), dict(ksize=cap(family)), dict(fallback=True)]
    out = [dict(ksize=1), dict(ksize=cap(family)), dict(fallback=True)]
    combos = [(ch, q, g) for ch in uc.CHANNELS for q in range(1, uc.MAX_RADIUS + 1) for g in (1, 3)]
    for waves in (8, 16):  # at every scale, so that the pin leaves the scale to the draw
        pool = [(ch, q, g) for ch, q, g in combos if all(uc.waves(ch, s, q, g) == waves for s in uc.SCALES)]
        ch, q, g = pool[int(r.integers(len(pool)))]
        out.append(dict(ksize=2 * q + 1, channels=ch, gch=g))
    return out


# ---- the draw ----
def _fam(family):
    return FAMILIES.index(family)


def _strat(values, family, name, i, seed0):
    """values[...] so that every run of len(values) consecutive i takes each value once."""
    block, j = divmod(i, len(values))
    r = np.random.default_rng([seed0, _fam(family), zlib.crc32(name.encode()), block])
    return values[int(r.permutation(len(values))[j])]


def _pin(family, i, seed0):
    n = counts()[family]
    block, j = divmod(i, n)
    r = np.random.default_rng([seed0, _fam(family), 77, block])
    todo = pins(family, r)
    assert len(todo) <= n, (family, len(todo))
    slot = [int(x) for x in r.permutation(n)]
    return dict(todo[slot.index(j)]) if slot.index(j) < len(todo) else {}


def _float_layout(r, rowbytes, vec):
    """(offset, pitch) in bytes, multiples of 4; both multiples of 16 exactly when vec."""
    up = -(-rowbytes // 16) * 16
    odd = lambda: 4 * int(r.integers(1, 4))  # noqa: E731  4, 8 or 12
    if vec:
        return 16 * int(r.integers(0, 3)), up + 16 * int(r.integers(0, 3))
    which = int(r.integers(0, 3))  # the base, the pitch, or both break the 16-byte rule
    off = 16 * int(r.integers(0, 3)) + (odd() if which != 1 else 0)
    pitch = up + 16 * int(r.integers(0, 3)) + (odd() if which != 0 else 0)
    return off, pitch


def _byte_layout(r, rowbytes):
    return int(r.integers(0, 6)), rowbytes + int(r.integers(0, 68))


def _log_uniform(r, lo, hi):
    return float(np.float32(10.0 ** r.uniform(lo, hi)))


def cost(c):
    k = c["ksize"]
    if c["family"] == "gray_texture":
        return c["w"] * c["h"] * (2 * k * k + (2 * k - 1) ** 2) * c["nitr"]
    return c["w"] * c["h"] * k * k * max(1, c["channels"])


def _shape(r, cls, res4, per_pixel, min_pixels):
    """(w, h) of the class with w % 4 == res4 and w * h * per_pixel <= COST_BOUND."""
    room = max(1, COST_BOUND // per_pixel)
    if cls == "tiny":
        w, h = int(r.integers(1, 9)), int(r.integers(1, 9))
    elif cls == "wide":
        w = int(r.integers(129, 301)) if r.random() < 0.7 else int(r.integers(40, 129))
        h = int(r.integers(1, 13))
    elif cls == "tall":
        w = int(r.integers(1, 13))
        h = int(r.integers(65, 161)) if r.random() < 0.7 else int(r.integers(30, 65))
    else:
        w, h = int(r.integers(20, 201)), int(r.integers(20, 101))
    if min_pixels:  # the statistic needs neighbours of both signs in reach
        w, h = max(w, 5), max(h, 3)
    if cls == "wide":
        h = max(1, min(h, room // w))
        w = min(w, room // h)
    elif cls == "tall":
        w = max(1, min(w, room // h))
        h = min(h, room // w)
    elif w * h > room:
        f = math.sqrt(room / (w * h))
        w, h = max(1, int(w * f)), max(1, int(h * f))
    w -= (w - res4) % 4
    if w < 1:
        w += 4
    while w * h > room and h > 1:
        h -= 1
    while w * h > room:
        w -= 4
    return w, h


def case(family, i, seed0=0):
    """Case i of the family under seed0: a dict of ints, floats, strings, bools and small dicts."""
    assert family in FAMILIES and i >= 0
    r = np.random.default_rng([seed0, _fam(family), i, 1])
    p = _pin(family, i, seed0)
    S = lambda values, name: _strat(values, family, name, i, seed0)  # noqa: E731
    c = dict(family=family, i=i, seed0=seed0)
    f32 = family in F32
    c["profile"] = S((0, 1), "profile")
    c["path"] = p.get("path", S((AUTO, RUNTIME), "path")) if family in HONOURS_PATH else AUTO
    if family == "gray":
        c["gch"] = p.get("gch", S((0, 1, 3), "gch"))
    elif family in ("gray_adaptive", "gray_texture"):
        c["gch"] = 0
    else:
        c["gch"] = p.get("gch", S((1, 3), "gch"))
    c["channels"] = p.get("channels", S((2, 3, 4), "channels")) if family in ("joint_f32c", "upsample_f32c") else 0
    up = family in ("upsample", "upsample_f32c")
    c["scale"] = p.get("scale", S((8, 8, 8, 8, 8, 8, 4, 4, 4, 4, 2, 2), "scale")) if up else 0
    c["nitr"] = int(r.integers(1, 4)) if family == "gray_texture" else 0
    c["stat"] = S(F32_STATS if f32 else U8_STATS, "stat")
    c["gstat"] = U8_STATS[int(r.integers(len(U8_STATS)))] if c["gch"] else ""
    huge = c["stat"] == "huge"
    fallback = bool(p.get("fallback"))
    # ksize: pinned, or half the time one beside a switch, else any the family takes
    allowed = ksizes(family, c["channels"], c["gch"])
    if "ksize" in p:
        k = p["ksize"]
    else:
        hot = sorted({q["ksize"] for q in pins(family, np.random.default_rng(0)) if "ksize" in q} & set(allowed))
        k = int(r.choice(hot)) if r.random() < 0.5 else int(r.choice(allowed))
    if huge and k < 5:  # a sum needs taps to overflow
        k = [q for q in allowed if q >= 5][int(r.integers(0, 3))]
    if fallback:  # few taps, so that all of them can weigh nothing
        k = int(r.choice([1, 3]))
    c["ksize"] = k
    # sigmas: log-uniform over tests/test_gpu_fuzz.py's decades; the upsamplers' sigma_color from 0.1
    c["ss"] = _log_uniform(r, -0.5, 2.5)
    c["sc"] = _log_uniform(r, -1.0 if up else -0.3, 2.3)
    if huge:  # weights near 1 under a narrow guide, so that the sums do overflow
        c["ss"], c["sc"], c["gstat"] = _log_uniform(r, 0.5, 2.5), _log_uniform(r, 2.7, 3.3), "narrow"
    if fallback:
        c["sc"], c["gstat"], c["stat"] = _log_uniform(r, -1.0, -0.5), "uniform", ("depth" if huge else c["stat"])
    if family == "gray_texture":
        c["ss"] = c["sc"] = 0.0  # the filter derives both from ksize
    c["fallback_pin"] = fallback
    cls = S(SHAPES, "shape")
    if (huge or fallback) and cls == "tiny":
        cls = "general"
    c["shape"] = cls
    per_pixel = cost(dict(c, w=1, h=1))
    c["w"], c["h"] = _shape(r, cls, S((0, 1, 2, 3), "w % 4"), per_pixel, huge or fallback)
    if up:  # the j-th case of this scale takes the scale's j-th residues
        s = c["scale"]
        j = sum(1 for q in range(i) if case_scale(family, q, seed0) == s)
        for key, name in (("w", "W % s"), ("h", "H % s")):
            res = _strat(tuple(range(s)), family, f"{name} {s}", j, seed0)
            v = c[key] - (c[key] - res) % s
            c[key] = v if v >= 1 else v + s
        while cost(c) > COST_BOUND:
            c["h"] -= s
    c["inplace"] = family == "gray_texture" and S((False, False, True, False), "inplace")
    # bands
    c["band"] = None
    if family in HAS_ROWS and S((False, True), "band"):
        h = c["h"]
        if h >= 3 and r.random() < 0.75:
            lo = int(r.integers(1, h - 1))
            hi = int(r.integers(lo + 1, h))
        else:
            lo = int(r.integers(0, h))
            hi = int(r.integers(lo + 1, h + 1))
        row0 = int(r.integers(lo, hi))
        c["band"] = dict(row_lo=lo, row_hi=hi, src_row0=row0, out_rows=int(r.integers(1, hi - row0 + 1)))
    # joint_conf's extras
    if family == "joint_conf":
        c["weight"] = S((True, False), "weight")
        c["conf"] = "holes" if huge and S(CONF_KINDS, "conf") == "real" else S(CONF_KINDS, "conf")
        c["poison"] = bool(r.random() < 0.5)  # NaN and Inf in f under the holes: the output ignores them
        c["hole_value"] = float(r.choice([0.0, -1.0, 12345.5]))
    # memory layout: every array its own base offset and pitch
    lay = {}
    w, h, ch = c["w"], c["h"], max(1, c["channels"])
    lw, lh = uo.low_size(w, h, c["scale"]) if up else (w, h)
    if f32:
        names = ["src", "dst"] + (["conf", "weight"] if family == "joint_conf" else [])
        if family == "joint_conf":  # 16 combinations with the weight plane, 8 without
            j = i // 2
            bits = _strat(tuple(range(16 if c["weight"] else 8)), family, f"vec {c['weight']}", j, seed0)
        else:
            bits = S((0, 1, 2, 3), "vec")
        for n, name in enumerate(names):
            rowbytes = 4 * ch * (lw if name == "src" else w)
            vec = bool(bits >> n & 1)
            lay[name] = _float_layout(r, rowbytes, vec) + (vec,)
        lay["guide"] = _byte_layout(r, c["gch"] * w)
        if up:
            lay["guide_lo"] = _byte_layout(r, c["gch"] * lw)
    else:
        lay["src"] = _byte_layout(r, w)
        lay["dst"] = lay["src"] if c["inplace"] else _byte_layout(r, w)
        if c["gch"]:
            lay["guide"] = _byte_layout(r, c["gch"] * w)
    c["lay"] = lay
    assert cost(c) <= COST_BOUND, c
    return c


def case_scale(family, i, seed0):
    """The scale of case i without drawing the rest (the residues count the cases of each scale)."""
    return _pin(family, i, seed0).get("scale", _strat((8, 8, 8, 8, 8, 8, 4, 4, 4, 4, 2, 2), family, "scale", i, seed0))


def vec_flags(c):
    """The per-array 16-byte decisions of the case, as the entry point will take them."""
    return tuple((name, off % 16 == 0 and pitch % 16 == 0) for name, (off, pitch, *_) in sorted(c["lay"].items())
                 if name in ("src", "dst", "conf", "weight") and (name != "weight" or c.get("weight")))


# ---- inputs ----
def _rng(c, salt):
    return np.random.default_rng([c["seed0"], _fam(c["family"]), c["i"], 100 + salt])


def _u8(r, h, w, stat, ch=0, salt=0):
    shape = (h, w, ch) if ch else (h, w)
    if stat == "uniform":
        a = r.integers(0, 256, shape)
    elif stat == "narrow":
        a = r.integers(100, 120, shape)
    elif stat == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        base = (x * 3 + y * 5 + salt * 17) % 256
        a = np.stack([base, (base + 85) % 256, 255 - base][:ch], axis=-1) if ch else base
    else:  # two_level: 5 x 3 cells of 0 | 255
        assert stat == "two_level"
        cells = r.integers(0, 2, (-(-h // 3), -(-w // 5)) + ((ch,) if ch else ())) * 255
        a = np.repeat(np.repeat(cells, 3, axis=0), 5, axis=1)[:h, :w]
    return np.ascontiguousarray(a, dtype=np.uint8)


def _f32(r, shape, stat):
    if stat == "depth":
        f = r.uniform(0.5, 10.0, shape)
    elif stat == "signed":
        f = r.standard_normal(shape) * 1000
    elif stat == "tiny":  # products with the weights go subnormal
        f = r.choice([-1.0, 1.0], shape) * 10.0 ** r.uniform(-36, -30, shape)
    elif stat == "zeros":  # 60 % of the pixels are +-0
        f = np.where(r.random(shape) < 0.6, r.choice([-0.0, 0.0], shape), r.standard_normal(shape))
        f = np.ascontiguousarray(f, dtype=np.float32)
        if not (np.signbit(f) & (f == 0)).any():
            f.flat[0] = -0.0
    else:  # huge: sums overflow
        assert stat == "huge"
        f = r.choice([-1.0, 1.0], shape) * 10.0 ** r.uniform(37, 38.5, shape)
    return np.ascontiguousarray(f, dtype=np.float32)


def arrays(c):
    """The host inputs: src always; guide, guide_lo, conf where the family has them. Whole frames:
    a band case reads rows [row_lo, row_hi) of them."""
    f, w, h, gch, ch = c["family"], c["w"], c["h"], c["gch"], c["channels"]
    out = {}
    up = f in ("upsample", "upsample_f32c")
    lw, lh = uo.low_size(w, h, c["scale"]) if up else (w, h)
    if f in F32:
        out["src"] = _f32(_rng(c, 0), (lh, lw, ch) if ch else (lh, lw), c["stat"])
    else:
        out["src"] = _u8(_rng(c, 0), h, w, c["stat"])
    if gch:
        out["guide"] = _u8(_rng(c, 1), h, w, c["gstat"], 0 if gch == 1 else 3, salt=1)
    if up:  # the low-resolution guide: the subsample of the guide, or (the fallback pin) unrelated to it
        s = c["scale"]
        if c["fallback_pin"] or c["i"] % 2:
            out["guide_lo"] = _u8(_rng(c, 2), lh, lw, c["gstat"], 0 if gch == 1 else 3, salt=2)
        else:
            out["guide_lo"] = np.ascontiguousarray(out["guide"][::s, ::s])
    if f == "joint_conf":
        r = _rng(c, 3)
        if c["conf"] == "ones":
            conf = np.ones((h, w))
        elif c["conf"] == "holes":
            conf = (r.random((h, w)) >= 0.4).astype(np.float64)
        else:  # [0, 1] with 20 % exact zeros
            conf = np.where(r.random((h, w)) < 0.2, 0.0, r.uniform(0.0, 1.0, (h, w)))
        out["conf"] = np.ascontiguousarray(conf, dtype=np.float32)
        if c["poison"]:
            src = out["src"]
            src[out["conf"] == 0] = r.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int((out["conf"] == 0).sum()))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the oracle ----
def want(c, a=None):
    """{"dst": ...} and, where the family has them, "weight" (joint_conf's sumk) and "fallback" (the
    upsamplers' map of the sumk == 0 pixels). A band case gives the band's out_rows rows: the filter
    of rows [row_lo, row_hi) alone, cut to them."""
    a = a or arrays(c)
    f, k, ss, sc, prof = c["family"], c["ksize"], c["ss"], c["sc"], c["profile"]
    src, guide = a["src"], a.get("guide")
    lo, hi, row0, rows = 0, c["h"], 0, c["h"]
    if c["band"]:
        b = c["band"]
        lo, hi, row0, rows = b["row_lo"], b["row_hi"], b["src_row0"] - b["row_lo"], b["out_rows"]
        src = np.ascontiguousarray(src[lo:hi])
        guide = None if guide is None else np.ascontiguousarray(guide[lo:hi])
    if f == "gray":
        if c["band"]:
            return {"dst": rs.gray_band(src, guide, row0, rows, k, ss, sc, prof)}
        fn = gray_oracle.bilateral if guide is None else (lambda g, *x: gray_oracle.joint_bilateral(g, guide, *x))
        return {"dst": fn(src, k, ss, sc, prof)}
    if f == "gray_adaptive":
        if c["band"]:
            return {"dst": gao.adaptive_rows(src, row0, rows, k, ss, sc, prof)}
        return {"dst": gao.adaptive(src, k, ss, sc, prof)}
    if f == "gray_texture":
        return {"dst": gto.texture(src, k, c["nitr"], prof)}
    if f == "joint_f32":
        return {"dst": np.ascontiguousarray(f32_oracle.joint_bilateral(src, guide, k, ss, sc, prof)[row0:row0 + rows])}
    if f == "joint_conf":
        dst, sumk = conf_oracle.joint_bilateral_conf(src, a["conf"], guide, k, ss, sc, prof, c["hole_value"])
        return {"dst": dst, "weight": sumk}
    if f == "joint_f32c":
        return {"dst": fo.joint_bilateral(src, guide, k, ss, sc, prof)}
    mod = uo if f == "upsample" else uc
    dst, zero = mod.upsample(src, a["guide_lo"], guide, c["scale"], k, ss, sc, prof, with_fallback=True)
    return {"dst": dst, "fallback": zero}
