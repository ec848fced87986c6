"""Numerical reference for gr_video_scale: a numpy restatement of VideoScaler::rescale / update_weights (video/scaler.cpp) and
assets/shaders/util/scaler.comp.

The planning half (weights, flags, transfer functions, matrices) is restated in float32, the way the C++ computes it.  The pixel half
evaluates in float64 with the shader's fp16 weights, its fixed-point sample positions and the fp16 staging of the filter's input and of
its vertical result (the two LDS tiles); the kernel evaluates in fp32 around the same fp16 points.  Out-of-frame input texels read as
zero on the same-size path and are clamped to the edge when rescaling (CLAMP_COORD, or the LinearClamp sampler of the prefilter).
"""
import ctypes as C
import os

import numpy as np

PHASES, TAPS = 256, 8

SRGB, SCRGB, HDR10 = 0, 1000104002, 1000104008
SKIP, DOWN, SAMPLED, CLAMP, CHROMA, PRIMARY, DITHER = 1, 2, 4, 8, 16, 32, 64
T_ID, T_SRGB, T_PQ = 0, 1, 2

R8, R8G8, RGBA8, BGRA8, RGBA8_SRGB, BGRA8_SRGB = 9, 16, 37, 44, 43, 50
A2B10G10R10, R16, R16G16, RGBA16F = 64, 70, 77, 97

GAMMA_BT709 = np.array([[0.5, -0.454153, -0.0458471, 0.5], [0.2126, 0.7152, 0.0722, 0.0], [-0.114572, -0.385428, 0.5, 0.5]], np.float32)
GAMMA_BT2020 = np.array([[0.5, -0.459786, -0.0402143, 0.5], [0.2627, 0.678, 0.0593, 0.0], [-0.13963, -0.36037, 0.5, 0.5]], np.float32)
PRIMARIES_709 = ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060), (0.3127, 0.3290))
PRIMARIES_2020 = ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046), (0.3127, 0.3290))


# ---- planning ------------------------------------------------------------------------------------------------------------------
def float_to_half_away(v):
    """muglm::floatToHalf: float32 -> fp16 bits, round to nearest with ties away from zero (not numpy's ties to even)."""
    v = np.asarray(v, np.float32)
    h = v.astype(np.float16)
    up = np.nextafter(h, np.copysign(np.float16(np.inf), h))
    # numpy rounded a tie toward zero when |v| lies exactly halfway between h and the next value away from zero
    tie_low = (np.abs(v.astype(np.float64) - h.astype(np.float64)) == np.abs(up.astype(np.float64) - v.astype(np.float64))) & \
              (np.abs(h.astype(np.float64)) < np.abs(v.astype(np.float64)))
    h = np.where(tie_low, up, h)
    return h.view(np.uint16)


def scaler_weights(in_w, in_h, out_w, out_h):
    """update_weights in float32: (2, 256, 8) fp16 bits, horizontal then vertical."""
    f = np.float32
    pi = f(np.pi)
    bw = f(min(max(f(out_w) / f(in_w), f(0.5)), f(1.0)))
    bh = f(min(max(f(out_h) / f(in_h), f(0.5)), f(1.0)))
    phase = np.arange(PHASES, dtype=np.float32)[:, None]
    tap = np.arange(TAPS, dtype=np.float32)[None, :]
    l = (tap - f(TAPS // 2 - 1)) - phase / f(PHASES)
    hv = np.cos(f(0.5) * (l / f(TAPS // 2)) * pi).astype(np.float32)
    hann = (hv * hv).astype(np.float32)

    def sinc(x):
        x = (x * pi).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (np.sin(x) / x).astype(np.float32)
        return np.where(np.abs(x) < f(0.0001), f(1.0), s).astype(np.float32)

    out = []
    for b in (bw, bh):
        w = (hann * sinc((b * l).astype(np.float32))).astype(np.float32)
        total = np.zeros(PHASES, np.float32)
        for t in range(TAPS):  # summed in tap order, as the C++ loop
            total = (total + w[:, t]).astype(np.float32)
        out.append(float_to_half_away((w / total[:, None]).astype(np.float32)))
    return np.stack(out)


def _xyz_matrix(prims):
    f = np.float32
    cols = [np.array([f(x) / f(y), 1.0, (f(1.0) - f(x) - f(y)) / f(y)], np.float64) for x, y in prims]
    p = np.stack(cols[:3], axis=1)
    scale = np.linalg.inv(p) @ cols[3]
    return p * scale[None, :]


def plan(in_size, in_format, planes, in_space, out_space):
    """VideoScaler::rescale's decisions; planes = [(w, h, format), ...].  None where it refuses."""
    spaces = (SRGB, SCRGB, HDR10)
    if in_space not in spaces or out_space not in spaces or not 1 <= len(planes) <= 3:
        return None
    if len(planes) > 1 and out_space == SCRGB:
        return None
    f = np.float32
    ow, oh = planes[0][0], planes[0][1]
    s = [f(in_size[0]) / f(ow), f(in_size[1]) / f(oh)]
    sampled = s[0] > 2 or s[1] > 2
    s = [min(f(2.0), v) for v in s]
    inv = [f(1.0) / (f(ow) * s[0]), f(1.0) / (f(oh) * s[1])]
    eotf = T_SRGB if in_space == SRGB and in_format != RGBA8_SRGB else T_PQ if in_space == HDR10 else T_ID
    oetf = T_SRGB if out_space == SRGB else T_PQ if out_space == HDR10 else T_ID
    flags = CLAMP
    if tuple(in_size) == (ow, oh):
        flags |= SKIP
    if s[0] > 1 or s[1] > 1:
        flags |= DOWN
    if sampled:
        flags |= SAMPLED
    if in_space != out_space:
        flags |= PRIMARY
    if len(planes) > 1 and ow > planes[1][0]:
        flags |= CHROMA
    dither = planes[0][2] in (RGBA8, RGBA8_SRGB, BGRA8, BGRA8_SRGB)
    if dither:
        flags |= DITHER
    if eotf == oetf and flags & SKIP:
        eotf = oetf = T_ID
    prim = np.eye(3)
    if in_space != out_space:
        to_out = np.linalg.inv(_xyz_matrix(PRIMARIES_2020 if out_space == HDR10 else PRIMARIES_709))
        conv = to_out @ _xyz_matrix(PRIMARIES_2020 if in_space == HDR10 else PRIMARIES_709)
        sdr = {SRGB: 200.0, SCRGB: 80.0}.get(in_space, 1.0)
        if out_space == SCRGB:
            sdr /= 80.0
        prim = sdr * conv
    return {"flags": flags, "eotf": eotf, "oetf": oetf, "num_planes": len(planes), "resolution": tuple(in_size),
            "scaling_to_input": tuple(s), "inv_input_resolution": tuple(inv), "dither_strength": f(1.0 / 255.0) if dither else f(0.0),
            "gamma_space_transform": GAMMA_BT2020 if out_space == HDR10 else GAMMA_BT709, "primary_transform": prim}


# ---- pixels --------------------------------------------------------------------------------------------------------------------
def decode_input(data, fmt):
    """Stored texels -> float32 RGBA as the kernel's fetch returns them (an *_SRGB view decodes)."""
    if fmt in (RGBA8, RGBA8_SRGB):
        v = data.astype(np.float32) / np.float32(255.0)
        if fmt == RGBA8_SRGB:
            v[..., :3] = decode_srgb(v[..., :3])
        return v
    if fmt == A2B10G10R10:
        u = data.astype(np.uint32)
        return np.stack([(u & 1023) / 1023.0, ((u >> 10) & 1023) / 1023.0, ((u >> 20) & 1023) / 1023.0, (u >> 30) / 3.0],
                        axis=-1).astype(np.float32)
    if fmt == RGBA16F:
        return data.view(np.float16).astype(np.float32)
    raise ValueError(fmt)


def decode_srgb(c):
    return np.clip(np.where(c <= 0.0404482362771082, c / 12.92, ((c + 0.055) / 1.055) ** 2.4), 0.0, 1.0)


def encode_srgb(c):
    c = np.maximum(c, 0.0)
    return np.clip(np.where(c <= 0.0031308, c * 12.92, 1.055 * c ** (1.0 / 2.4) - 0.055), 0.0, 1.0)


def pq_eotf(v):
    m1, m2, c2, c3 = 0.1593017578125, 78.84375, 18.8515625, 18.6875
    c1 = c3 - c2 + 1.0
    e = np.maximum(v, 0.0) ** (1.0 / m2)
    return (np.maximum(e - c1, 0.0) / (c2 - c3 * e)) ** (1.0 / m1) * 10000.0


def pq_oetf(v):
    c1, c2, c3, m1, m2 = 0.8359375, 18.8515625, 18.6875, 0.1593017578125, 78.84375
    p = np.clip(v / 10000.0, 0.0, 1.0) ** m1
    return ((c1 + c2 * p) / (1.0 + c3 * p)) ** m2


def _transfer(kind, decode, rgb):
    if kind == T_SRGB:
        return decode_srgb(rgb) if decode else encode_srgb(rgb)
    if kind == T_PQ:
        return pq_eotf(rgb) if decode else pq_oetf(rgb)
    return rgb


def _eotf(p, v):
    v = v.copy()
    v[..., :3] = _transfer(p["eotf"], True, v[..., :3])
    return v


def _finish(p, v):
    v = v.copy()
    if p["flags"] & PRIMARY:
        v[..., :3] = v[..., :3] @ np.asarray(p["primary_transform"], np.float64).T
    v[..., :3] = _transfer(p["oetf"], False, v[..., :3])
    return v


def _f16(v):
    return v.astype(np.float16).astype(np.float64)


def _sample_pos(o, s):
    """scaler.comp's 8.8 fixed-point position of output o (int array), every operation rounded to float32, int() truncating."""
    f = np.float32
    s = f(s)
    base = (o & ~7).astype(np.float32)
    base_input = ((base + f(0.5)) * s) - f(0.5)
    v = f(PHASES) * (base_input + s * (o.astype(np.int64) - (o & ~7)).astype(np.float32)) + f(0.5)
    return np.trunc(v.astype(np.float32)).astype(np.int64)


def _linear_clamp(img, u, v):
    """LinearClamp at normalised (u, v) (float32 grids), the project's sampler model (device_common.hpp: sample_linear_with)."""
    h, w = img.shape[:2]
    snap = np.float32(1.0 / 256.0)

    def axis(c, n):
        f = (c * np.float32(n) - np.float32(0.5)).astype(np.float32)
        fl = np.floor(f + snap)
        a = (f - fl).astype(np.float32)
        a[a < snap] = 0.0
        i0 = fl.astype(np.int64)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), a

    x0, x1, a = axis(u, w)
    y0, y1, b = axis(v, h)
    a = a[None, :, None]
    b = b[:, None, None]
    t00, t10 = img[y0][:, x0], img[y0][:, x1]
    t01, t11 = img[y1][:, x0], img[y1][:, x1]
    one = np.float32(1.0)
    return t00 * ((one - a) * (one - b)) + t10 * (a * (one - b)) + t01 * ((one - a) * b) + t11 * (a * b)


def _rescaled(rgba, p, out_w, out_h, weights):
    """Linear-light rescaled frame at every output of the padded (even) extent, before primary conversion and OETF."""
    in_h, in_w = rgba.shape[:2]
    sx, sy = p["scaling_to_input"]
    ox = np.arange(out_w + (out_w & 1))
    oy = np.arange(out_h + (out_h & 1))
    px, py = _sample_pos(ox, sx), _sample_pos(oy, sy)
    cols = np.arange((px >> 8).min() - 3, (px >> 8).max() + 5)
    rows = np.arange((py >> 8).min() - 3, (py >> 8).max() + 5)
    if p["flags"] & SAMPLED:
        u = ((cols.astype(np.float32) + np.float32(0.5)) * np.float32(p["inv_input_resolution"][0])).astype(np.float32)
        v = ((rows.astype(np.float32) + np.float32(0.5)) * np.float32(p["inv_input_resolution"][1])).astype(np.float32)
        stage = _linear_clamp(rgba, u, v)
    else:
        stage = rgba[np.clip(rows, 0, in_h - 1)][:, np.clip(cols, 0, in_w - 1)]
    stage = _f16(_eotf(p, stage)).astype(np.float32)
    wt = weights.view(np.float16).astype(np.float64)
    wv = wt[1][py & 255]  # (out rows, 8)
    mid = np.zeros((len(oy), len(cols), 4))
    for k in range(TAPS):
        mid += wv[:, k, None, None] * stage[(py >> 8) - 3 + k - rows[0]]
    mid = _f16(mid)
    wh = wt[0][px & 255]
    out = np.zeros((len(oy), len(ox), 4))
    for k in range(TAPS):
        out += wh[None, :, k, None] * mid[:, (px >> 8) - 3 + k - cols[0]]
    return out


DITHER_TABLE = (np.array([[1, 9, 3, 11], [13, 5, 15, 7], [4, 12, 2, 10], [16, 8, 14, 6]]) / 16.0) - 0.5


def _dither(x, y):
    return DITHER_TABLE[y[:, None] & 3, x[None, :] & 3]


def dither_probe():
    """64 x 16 RGBA16F frame (scRGB, same size: no transfer, no conversion) whose every channel in column block j = x / 4 and row
    block k = y / 4 holds (10 + k + (j + 0.5) / 16) / 255.  The one-plane store adds (n / 16 - 0.5) / 255, n the table entry at
    (x & 3, y & 3), so the code is 10 + k + 1 exactly when n + j >= 16: 1/32 of a code from any midpoint, far beyond the fp16
    input (2^-16 * 255 here) and every rounding after it.  Returns (data, expected codes (h, w, 4))."""
    h, w = 16, 64
    y, x = np.mgrid[0:h, 0:w]
    j, k = x // 4, y // 4
    v = (10 + k + (j + 0.5) / 16) / 255
    data = np.repeat(v[..., None], 4, axis=-1).astype(np.float16).view(np.uint16)
    codes = 10 + k + ((DITHER_TABLE[y & 3, x & 3] + 0.5) * 16 + j >= 16)
    return data, np.repeat(codes[..., None], 4, axis=-1)


def _codes(v, bits):
    scale = 255.0 if bits == 8 else 65535.0
    return np.floor(np.clip(v, 0.0, 1.0) * scale + 0.5).astype(np.int64)


def video_scale(data, in_format, planes, in_space, out_space, weights=None):
    """Expected output planes (integer codes) of gr_video_scale.  data: stored input texels (h, w, 4) uint8 / (h, w) uint32 /
    (h, w, 4) fp16 bits; planes: [(w, h, format), ...]; weights: the filter's (2, 256, 8) fp16 table, by default
    scaler_weights' for these sizes.  Returns a list of arrays: (h, w) for Y / Cb / Cr, (h, w, 2) for interleaved chroma, (h, w, 4)
    for RGBA/BGRA."""
    rgba = decode_input(data, in_format)
    in_h, in_w = rgba.shape[:2]
    p = plan((in_w, in_h), in_format, planes, in_space, out_space)
    assert p is not None
    out_w, out_h, fmt0 = planes[0]
    if p["flags"] & SKIP:
        pad = np.zeros((out_h + (out_h & 1), out_w + (out_w & 1), 4))
        pad[:out_h, :out_w] = rgba
        px = _finish(p, _eotf(p, pad))
    else:
        weights = scaler_weights(in_w, in_h, out_w, out_h) if weights is None else weights
        px = _finish(p, _rescaled(rgba, p, out_w, out_h, weights))
    ys, xs = np.arange(px.shape[0]), np.arange(px.shape[1])
    d = _dither(xs, ys) * float(p["dither_strength"])
    if len(planes) == 1:
        v = px + d[..., None]
        c = _codes(v, 8)[:out_h, :out_w]
        if fmt0 in (BGRA8, BGRA8_SRGB):
            c = c[..., [2, 1, 0, 3]]
        return [c]
    bits = 16 if fmt0 == R16 else 8
    g = np.asarray(p["gamma_space_transform"], np.float64)
    rgb = np.clip(px[..., :3], 0.0, 1.0)
    ycc = rgb @ g[:, :3].T + g[:, 3]  # Cr, Y, Cb
    y = _codes(ycc[..., 1] + d, bits)[:out_h, :out_w]
    cb, cr = ycc[..., 2], ycc[..., 0]
    cw, ch = planes[1][0], planes[1][1]
    if p["flags"] & CHROMA:
        cb = 0.25 * (cb[0::2, 0::2] + cb[0::2, 1::2] + cb[1::2, 0::2] + cb[1::2, 1::2])
        cr = 0.25 * (cr[0::2, 0::2] + cr[0::2, 1::2] + cr[1::2, 0::2] + cr[1::2, 1::2])
        dc = _dither(np.arange(cb.shape[1]), np.arange(cb.shape[0])) * float(p["dither_strength"])
    else:
        dc = d
    cb = _codes(cb + dc, bits)[:ch, :cw]
    cr = _codes(cr + dc, bits)[:ch, :cw]
    if len(planes) == 2:
        return [y, np.stack([cb, cr], axis=-1)]
    return [y, cb, cr]


# ---- the reference's own shader, executed on the CPU -----------------------------------------------------------------------------
REF_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_video.so")
_ref_lib = None


def shader_lib():
    """oracle/_ref/libref_video.so (oracle/ref_build: scaler.comp run on the CPU by ref_video.cpp); skips the calling test when
    it was not built, which needs the reference's sources."""
    global _ref_lib
    if _ref_lib is None:
        if not os.path.exists(REF_LIB):
            import pytest
            pytest.skip("oracle/_ref/libref_video.so not built (needs the reference's sources)")
        lib = C.CDLL(REF_LIB)
        P = C.c_void_p
        lib.ref_video_scale.restype = C.c_int
        lib.ref_video_scale.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, C.c_int, C.c_int, C.c_int, P, P, P, P, P,
                                        C.c_float, P]
        _ref_lib = lib
    return _ref_lib


def shader_scale(data, in_format, planes, p, weights):
    """Output planes of scaler.comp, executed, in video_scale's layout.  p: a plan (gr_video_scale_plan's, or plan() above);
    weights: the (2, 256, 8) fp16 bits of the table the launch would use."""
    lib = shader_lib()
    data = np.ascontiguousarray(data)
    in_h, in_w = data.shape[:2]
    outs = []
    for w, h, fmt in planes:
        ch = 4 if fmt in (RGBA8, BGRA8, RGBA8_SRGB, BGRA8_SRGB) else 2 if fmt in (R8G8, R16G16) else 1
        outs.append(np.zeros((h, w, ch) if ch > 1 else (h, w), np.uint16 if fmt in (R16, R16G16) else np.uint8))
    n = len(planes)
    ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    floats = lambda v: np.ascontiguousarray(v, np.float32)
    pw, ph, pf = ints([q[0] for q in planes]), ints([q[1] for q in planes]), ints([q[2] for q in planes])
    gst = floats(np.asarray(p["gamma_space_transform"], np.float32).reshape(3, 4))
    prim = floats(np.asarray(p["primary_transform"], np.float32).T)  # column major
    res, sti, inv = ints(p["resolution"]), floats(p["scaling_to_input"]), floats(p["inv_input_resolution"])
    table = np.ascontiguousarray(weights, np.uint16)
    ptr = lambda a: a.ctypes.data
    rc = lib.ref_video_scale(ptr(data), in_w, in_h, in_format, n, C.cast(ptrs, C.c_void_p), ptr(pw), ptr(ph), ptr(pf), int(p["flags"]),
                             int(p["eotf"]), int(p["oetf"]), ptr(gst), ptr(prim), ptr(res), ptr(sti), ptr(inv),
                             float(p["dither_strength"]), ptr(table))
    assert rc == 0, f"scaler.comp not built for CONTROL {p['flags']}, EOTF {p['eotf']}, OETF {p['oetf']}, {n} planes (VIDEO_VARIANTS)"
    return [o.astype(np.int64) for o in outs]
