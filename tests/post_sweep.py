"""Case lists of the bloom-launch sweep, and the index arithmetic of the fused kernels restated for the CPU.

Nothing here loads the kernel library or needs a GPU: tests/test_post_sweep_cpu.py asserts that the lists cover what they claim (template
combinations, last-tile remainders, patch fills) and tests/test_gpu_post_sweep.py runs them.

A "case" is a dict of level sizes by name ((width, height) each: hdr, threshold, d0, d1, d2, d3, u2, u1, u0 -- whichever the launch reads or
writes), made either from a frame size as the render graph makes them (frame_levels) or directly from a pair of levels ("off-pyramid": the
entry points take any levels within their ratio rules).

Restated from granite_amd/csrc/post.hip (the names are the file's):
  is_half_of, down_patch_fits, up_patch_fits, the size limits of the gr_bloom_*_supported queries  -> the *_offered functions
  tap_span                                                                                        -> tap_span
  down_pair_block (px0 .. py1), k_bloom_up_tail (px0 .. py1), up_all_block (ax0 .. by1)           -> *_extent
"""
import importlib.util
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# post.hip: constexpr int ...
TAIL_TILE, TAIL_PATCH = 8, 24
UP_TILE, UP_PATCH = 32, 24
UPALL_TILE, UPALL_P1, UPALL_P2 = 32, 20, 18

SCALES = dict(threshold=0.5, d0=0.25, d1=0.125, d2=0.0625, d3=0.03125, u2=0.0625, u1=0.125, u0=0.25)


def level_size(w, h, scale):
    """InputRelative size: ceil(dimension * scale), at least 1 (the scales are powers of two: exact in any float format)."""
    return max(math.ceil(w * scale), 1), max(math.ceil(h * scale), 1)


def frame_levels(w, h):
    levels = {"hdr": (w, h)}
    levels.update({name: level_size(w, h, s) for name, s in SCALES.items()})
    return levels


# ---- the launch rules, restated ------------------------------------------------------------------------------------------------------------
def is_half_of(out, inp):
    return inp[0] == 2 * out[0] and inp[1] == 2 * out[1]


def down_patch_fits(fine, coarse):
    """float(fine) <= 2.3f * float(coarse) per axis, in fp32 as the library evaluates it."""
    f32 = np.float32
    return bool(f32(fine[0]) <= f32(2.3) * f32(coarse[0]) and f32(fine[1]) <= f32(2.3) * f32(coarse[1]))


def up_patch_fits(fine, coarse):
    return all(f <= 2 * c and 2 * c <= f + 1 for f, c in zip(fine, coarse))


def area(size):
    return size[0] * size[1]


def mid_fits(l):
    return down_patch_fits(l["d0"], l["d1"])


def mid_offered(l):
    """gr_bloom_down_mid_supported: the patch rule, and downsample-1 up to 65536 texels (a 1440p frame's)."""
    return mid_fits(l) and area(l["d1"]) <= 65536


def head_fits(l):
    return is_half_of(l["threshold"], l["hdr"]) and is_half_of(l["d0"], l["threshold"]) and is_half_of(l["d1"], l["d0"])


def head_offered(l):
    """gr_bloom_down_head_supported: where the fused middle is offered and every level is exactly half of its input (tight rows of such a frame
    are 16-byte aligned in both HDR formats: its width is a multiple of 8)."""
    return mid_offered(l) and head_fits(l)


def down_tail_fits(l):
    return down_patch_fits(l["d2"], l["d3"])


def up_tail_fits(l):
    return up_patch_fits(l["u1"], l["u2"])


def tail_offered(l):
    """gr_bloom_tail_supported: both launches fit and upsample-2 has the size of downsample-2."""
    return down_tail_fits(l) and up_tail_fits(l) and l["u2"] == l["d2"]


def up_all_fits(l):
    return up_tail_fits(l) and is_half_of(l["u1"], l["u0"])


def up_all_offered(l):
    """gr_bloom_up_all_supported: what the upsample tail takes, upsample-0 exactly twice upsample-1 and at most 960 x 540 (a 4K frame's)."""
    return up_all_fits(l) and area(l["u0"]) <= 960 * 540


def pyramid_fits(l):
    return head_fits(l) and down_tail_fits(l) and up_all_fits(l) and l["u2"] == l["d2"]


def pyramid_offered(l):
    """gr_bloom_pyramid_supported: where the three launches it stands for are offered, up to a 640 x 384 frame."""
    return head_offered(l) and tail_offered(l) and up_all_offered(l) and area(l["hdr"]) <= 640 * 384


OFFERED = {"down_mid": mid_offered, "down_head": head_offered, "tail": tail_offered, "up_all": up_all_offered, "pyramid": pyramid_offered}


# ---- template flags a launch gets, from the level sizes alone (downsample_is_exact / upsample_is_exact on tight, aligned levels) ---------------
def mid_flags(l):
    return is_half_of(l["d0"], l["threshold"]), is_half_of(l["d1"], l["d0"])           # A_EXACT, B_EXACT


def down_tail_flags(l):
    return is_half_of(l["d2"], l["d1"]), is_half_of(l["d3"], l["d2"])                  # A_EXACT, B_EXACT (D2_EXACT, D3_EXACT)


def up_flags(l):
    return is_half_of(l["d3"], l["u2"]), is_half_of(l["u2"], l["u1"])                  # U2_EXACT, U1_EXACT


def pyramid_flags(l):
    return down_tail_flags(l) + up_flags(l)                                            # D2_EXACT, D3_EXACT, U2_EXACT, U1_EXACT


# ---- patch extents ---------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fp32 fma through fp64 (the product of two fp32 is exact there)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def tap_span(lo, hi, out_n, in_n, reach):
    """post.hip tap_span(): first and last input index under outputs [lo, hi], in fp32 (scalars or arrays that broadcast).  The function is
    compiled with contraction allowed, so a multiply-subtract may or may not be one fma: every form is evaluated and the widest span returned
    (they differ only where a tap lies within an ulp of a texel boundary)."""
    f32 = np.float32
    lo, hi, out_n, in_n = (np.asarray(v, np.int64) for v in (lo, hi, out_n, in_n))
    scale = in_n.astype(f32) / out_n.astype(f32)
    half, reach = f32(0.5), f32(reach)
    lo_c, hi_c = lo.astype(f32) + half, hi.astype(f32) + half
    firsts = [lo_c * scale - half - reach, _fma32(lo_c, scale, -(half + reach)), _fma32(lo_c, scale, -half) - reach]
    lasts = [hi_c * scale - half + reach, _fma32(hi_c, scale, reach - half), _fma32(hi_c, scale, -half) + reach]
    first = np.minimum.reduce([np.floor(v).astype(np.int64) for v in firsts]) - 1
    last = np.maximum.reduce([np.floor(v).astype(np.int64) for v in lasts]) + 2
    return np.clip(first, 0, in_n - 1), np.clip(last, 0, in_n - 1)


def _tiles(n, tile):
    return [(t, min(t + tile, n) - 1) for t in range(0, n, tile)]


def _clamp(v, n):
    return min(max(v, 0), n - 1)


def down_axis_extent(fine, coarse, exact):
    """Widest patch of `fine` (rows or columns) staged under one 8-texel tile of `coarse` by down_pair_block; (extent, tile start)."""
    best = (0, 0)
    for lo, hi in _tiles(coarse, TAIL_TILE):
        if exact:
            p0, p1 = _clamp(2 * lo - 2, fine), _clamp(2 * hi + 3, fine)
        else:
            p0, p1 = (int(v) for v in tap_span(lo, hi, coarse, fine, 1.75))
        best = max(best, (p1 - p0 + 1, lo))
    return best


def down_extent(fine, coarse):
    """down_pair_block over both axes (B_EXACT is one flag for both); (largest extent, (axis, tile start))."""
    exact = is_half_of(coarse, fine)
    ex = [down_axis_extent(fine[a], coarse[a], exact) for a in (0, 1)]
    return max((ex[0][0], ("x", ex[0][1])), (ex[1][0], ("y", ex[1][1])))


def up_axis_extent(fine, coarse, exact):
    """Widest patch of `coarse` (upsample-2) under one 32-texel tile of `fine` (upsample-1) in k_bloom_up_tail."""
    best = 0
    for lo, hi in _tiles(fine, UP_TILE):
        if exact:
            p0, p1 = _clamp((lo >> 1) - 2, coarse), _clamp((hi >> 1) + 2, coarse)
        else:
            p0, p1 = (int(v) for v in tap_span(lo, hi, fine, coarse, 0.875))
        best = max(best, p1 - p0 + 1)
    return best


def up_tail_extent(u1, u2):
    exact = is_half_of(u2, u1)
    return max(up_axis_extent(u1[a], u2[a], exact) for a in (0, 1))


def up_all_axis_extents(u0, u1, u2, u1_exact):
    """up_all_block: (widest patch of upsample-1, widest patch of upsample-2) under one 32-texel tile of upsample-0."""
    best1 = best2 = 0
    for lo, hi in _tiles(u0, UPALL_TILE):
        a0, a1 = _clamp((lo >> 1) - 2, u1), _clamp((hi >> 1) + 2, u1)
        if u1_exact:
            b0, b1 = _clamp((a0 >> 1) - 2, u2), _clamp((a1 >> 1) + 2, u2)
        else:
            b0, b1 = (int(v) for v in tap_span(a0, a1, u1, u2, 0.875))
        best1, best2 = max(best1, a1 - a0 + 1), max(best2, b1 - b0 + 1)
    return best1, best2


def up_all_extents(u0, u1, u2):
    exact = is_half_of(u2, u1)
    ex = [up_all_axis_extents(u0[a], u1[a], u2[a], exact) for a in (0, 1)]
    return max(ex[0][0], ex[1][0]), max(ex[0][1], ex[1][1])


# ---- the lists -------------------------------------------------------------------------------------------------------------------------------
# Parity sweep: three periods of 32 in one dimension, the other once a multiple of 64 (every level of that axis an exact half) and once odd
# (every level a ceil).  ceil(65 / 32) = 3: downsample-3 has at least 3 texels, its luminance grid at least one.
PARITY_RANGE = range(65, 161)
PARITY_FIXED = (128, 97)
PARITY_SWEEP = sorted({(v, f) for v in PARITY_RANGE for f in PARITY_FIXED} | {(f, v) for v in PARITY_RANGE for f in PARITY_FIXED})

# Off-pyramid pairs, per axis (fine, coarse).  Down rule (fine <= 2.3 coarse): its boundary fine = floor(2.3 coarse), the two pyramid ratios
# and equal sizes.  Up rule (fine <= 2 coarse <= fine + 1): both of its cases.
DOWN_AXIS_TAKEN = [(23, 10), (43, 19), (46, 20), (230, 100), (37, 19), (38, 19), (19, 19), (23, 12), (24, 12)]
DOWN_AXIS_DECLINED = [(24, 10), (44, 19), (47, 20), (231, 100)]          # one more texel than the rule allows
UP_AXIS_TAKEN = [(24, 12), (23, 12), (38, 19), (37, 19), (66, 33), (65, 33), (200, 100), (199, 100)]
UP_AXIS_DECLINED = [(25, 12), (22, 12), (19, 19), (67, 33)]
# ... and for the remainder of the last tile: every width of the coarse (down) / fine (up) level modulo the tile
DOWN_AXIS_REMAINDERS = [(2 * c - (c & 1), c) for c in range(9, 17)]
UP_AXIS_REMAINDERS = [(f, (f + 1) // 2) for f in range(33, 65)]
UP_ALL_AXIS_REMAINDERS = [(u1, (u1 + 1) // 2) for u1 in range(17, 33)]  # upsample-0 = 2 x upsample-1: 34 .. 64


def _both_axes(axis_cases):
    """Each axis case on both axes, then the axes taking different cases (x: case i, y: case i + 1)."""
    n = len(axis_cases)
    return [(axis_cases[i], axis_cases[i]) for i in range(n)] + [(axis_cases[i], axis_cases[(i + 1) % n]) for i in range(n)]


def _down_pair_levels(names, x, y, k):
    """Levels (src, fine, coarse) of a down_pair launch: the input level alternately exactly twice the fine one and one texel short of it."""
    src_name, fine_name, coarse_name = names
    fine, coarse = (x[0], y[0]), (x[1], y[1])
    src = (2 * fine[0], 2 * fine[1]) if k % 2 == 0 else (2 * fine[0] - 1, 2 * fine[1] - 1)
    return {src_name: src, fine_name: fine, coarse_name: coarse}


def down_pair_cases(names):
    """(levels, taken) for gr_bloom_down_mid (threshold, d0, d1) or gr_bloom_down_tail (d1, d2, d3)."""
    out = []
    for k, (x, y) in enumerate(_both_axes(DOWN_AXIS_TAKEN) + [(c, c) for c in DOWN_AXIS_REMAINDERS]):
        out.append((_down_pair_levels(names, x, y, k), True))
    for k, d in enumerate(DOWN_AXIS_DECLINED):
        ok = DOWN_AXIS_TAKEN[k]
        out.append((_down_pair_levels(names, d, ok, k), False))       # the rule broken in x only,
        out.append((_down_pair_levels(names, ok, d, k + 1), False))   # in y only
    return out


def _up_levels(x, y, k):
    """Levels (d3, u2, u1) of an upsample-tail launch: downsample-3 alternately exactly half of upsample-2 and the ceil of it."""
    u1, u2 = (x[0], y[0]), (x[1], y[1])
    d3 = ((u2[0] + 1) // 2, (u2[1] + 1) // 2) if k % 2 else (max(u2[0] // 2, 1), max(u2[1] // 2, 1))
    return {"d3": d3, "u2": u2, "u1": u1}


def up_tail_cases():
    out = [(_up_levels(x, y, k), True) for k, (x, y) in enumerate(_both_axes(UP_AXIS_TAKEN) + [(c, c) for c in UP_AXIS_REMAINDERS])]
    for k, d in enumerate(UP_AXIS_DECLINED):
        ok = UP_AXIS_TAKEN[k]
        out += [(_up_levels(d, ok, k), False), (_up_levels(ok, d, k + 1), False)]
    return out


def up_all_cases():
    """up_tail's levels with upsample-0 exactly twice upsample-1 on top; and one texel off that (declined: upsample-0 runs on the 1:2 stencil only)."""
    out = []
    for levels, taken in [(_up_levels(x, y, k), True) for k, (x, y) in enumerate(_both_axes(UP_AXIS_TAKEN) + [(c, c) for c in UP_ALL_AXIS_REMAINDERS])]:
        out.append((dict(levels, u0=(2 * levels["u1"][0], 2 * levels["u1"][1])), taken))
    for k, d in enumerate(UP_AXIS_DECLINED):
        levels = _up_levels(d, UP_AXIS_TAKEN[k], k)
        out.append((dict(levels, u0=(2 * levels["u1"][0], 2 * levels["u1"][1])), False))
    levels = _up_levels(UP_AXIS_TAKEN[0], UP_AXIS_TAKEN[2], 0)
    out.append((dict(levels, u0=(2 * levels["u1"][0] - 1, 2 * levels["u1"][1])), False))
    return out


def pyramid_offpyramid_cases():
    """gr_bloom_pyramid on levels a frame never has: upsample-1 (and with it upsample-0) one texel off downsample-1's size, so that D2_EXACT and
    U1_EXACT differ -- the combinations of the four size flags that no frame reaches.  (D3_EXACT = U2_EXACT always: upsample-2 must have
    downsample-2's size.)  The launcher is asked directly; the query offers these too (every rule holds)."""
    out = []
    for d3 in ((4, 3), (5, 4)):
        for d2_exact_half in (True, False):     # downsample-3 exactly half of downsample-2, or its ceil
            d2 = (2 * d3[0], 2 * d3[1]) if d2_exact_half else (2 * d3[0] - 1, 2 * d3[1] - 1)
            for d2_exact in (True, False):      # D2_EXACT and not U1_EXACT, or the other way round
                even, odd = (2 * d2[0], 2 * d2[1]), (2 * d2[0] - 1, 2 * d2[1] - 1)
                d1, u1 = (even, odd) if d2_exact else (odd, even)
                out.append({"hdr": (8 * d1[0], 8 * d1[1]), "threshold": (4 * d1[0], 4 * d1[1]), "d0": (2 * d1[0], 2 * d1[1]), "d1": d1, "d2": d2,
                            "d3": d3, "u2": d2, "u1": u1, "u0": (2 * u1[0], 2 * u1[1])})
    return out


# ---- the committed table's 1s ----------------------------------------------------------------------------------------------------------------
def golden_generator():
    spec = importlib.util.spec_from_file_location("make_bloom_supported_golden", os.path.join(GOLDEN, "make_bloom_supported_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


_committed = None


def committed_answers():
    """{(w, h): {"f16 lum": "11110", ...}} for the un-varied frames of tests/golden/bloom_supported.json (ids "WxH fmt lum", no variant suffix), and
    the function names in the table's order."""
    global _committed
    if _committed is None:
        doc = json.load(open(os.path.join(GOLDEN, "bloom_supported.json")))
        frames = {}
        for name, answer in doc["answers"].items():
            parts = name.split(" ")
            if len(parts) != 3:
                continue
            w, h = (int(v) for v in parts[0].split("x"))
            frames.setdefault((w, h), {})[parts[1] + " " + parts[2]] = answer
        _committed = (frames, tuple(doc["functions"]))
    return _committed


def committed_ones(function):
    """Frame sizes whose committed answer for `function` is 1 (in every format / exposure form the table holds), sorted."""
    frames, functions = committed_answers()
    i = functions.index(function)
    return sorted(size for size, forms in frames.items() if all(a[i] == "1" for a in forms.values()))


def frame_cases(function, cross):
    """What the GPU test of `function` launches on frames: (list name, (w, h), levels, option) over the parity sweep where the rules offer the launch
    (every option 0 .. cross - 1: HDR format / exposure form) and over the committed 1s (one option, picked by a hash of the size)."""
    out = []
    for w, h in PARITY_SWEEP:
        levels = frame_levels(w, h)
        if OFFERED[function](levels):
            out += [("parity", (w, h), levels, option) for option in range(cross)]
    for w, h in committed_ones(function):
        out.append(("committed 1s", (w, h), frame_levels(w, h), size_hash(w, h) % cross))
    return out


CROSS = {"down_mid": 1, "down_head": 4, "tail": 2, "up_all": 2, "pyramid": 4}  # options the GPU tests cross the parity sweep with


def size_hash(w, h):
    """A fixed hash of a frame size: picks the HDR format (bit 0) and the exposure form (bit 1) on the limit grid."""
    return (w * 2654435761 + h * 40503) >> 7


# ---- descriptors for the context-free queries ----------------------------------------------------------------------------------------------
def fake_images(levels, b10=False):
    """Image descriptors of the levels (fake, aligned, distinct device pointers: the queries never dereference them), history the size of d3."""
    from granite_amd import capi
    images = {}
    for i, (name, (w, h)) in enumerate(sorted(levels.items()) + [("history", levels.get("d3", (1, 1)))]):
        fmt = capi.FORMAT_B10G11R11_UFLOAT_PACK32 if (b10 and name == "hdr") else capi.FORMAT_R16G16B16A16_SFLOAT
        images[name] = capi.Image(0x100000000 + i * 0x40000000, w, h, w * capi.FORMAT_BPP[fmt], fmt)
    return images


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
SPECIAL_HALVES = (0x0000, 0x0001, 0x7bff, 0x7c00)  # +0, the smallest denormal, 65504, +inf


def special_positions(w, h, k):
    """Where special value k (0 .. 3) goes in a w x h image (at least 38 x 25): an image corner, the last column (a partial tile's), a corner of
    an 8 x 8 tile, the interior."""
    corner = ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))[k]
    return [corner, (w - 1, h * (k + 1) // 5), (8 * (1 + k % 2) + 16 * (k // 2), 8 * (1 + k // 2)), (5 + 7 * k, 3 + 5 * k)]


def plant_specials(bits):
    """The four special values, whole texels, at their positions in an H x W x 4 array of half bits (in place; returns the (x, y) list)."""
    h, w = bits.shape[:2]
    assert w >= 38 and h >= 25
    planted = []
    for k, value in enumerate(SPECIAL_HALVES):
        for x, y in special_positions(w, h, k):
            bits[y, x, :] = value
            planted.append((x, y))
    assert len(set(planted)) == 16
    return planted


def random_level(size, seed, lo=-8, hi=6):
    """Positive finite fp16 texels, exp2(uniform(lo, hi)), as half bits."""
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(lo, hi, (size[1], size[0], 4))).astype(np.float16).view(np.uint16)
