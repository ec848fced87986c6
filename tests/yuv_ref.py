"""Numerical reference for gr_video_yuv_to_rgb: a numpy restatement of VideoDecoder::Impl::init_yuv_to_rgb / dispatch_conversion
(video/ffmpeg_decode.cpp) and assets/shaders/util/yuv_to_rgb.comp, written from the shader and the host code, not from the kernel.

The planning half (the UBO and the three specialization constants) is restated in float32, operation by operation, the way the C++
computes it.  The pixel half evaluates in float64 by default; `dtype=np.float32` evaluates the same arithmetic with every operation
rounded to float32 and pow(x, y) as exp2(y * log2(x)), which is how GLSL defines its precision.  The chroma fetch is the project's
sampler model (oracle/oracle_common.h linear_axis: float32 coordinates and weights, 2^-8 texel snap, clamp to edge); the 16-bit
fetch is v / 65535.
"""
import numpy as np

R8, R8G8, RGBA8, RGBA8_SRGB, A2B10G10R10, R16, R16G16, RGBA16F = 9, 16, 37, 43, 64, 70, 77, 97
M_UNSPECIFIED, M_BT601_525, M_BT601_625, M_BT709, M_BT2020, M_SMPTE240M = range(6)
C_CENTER, C_LEFT, C_TOPLEFT, C_TOP, C_BOTTOMLEFT, C_BOTTOM = range(6)
SITING = {C_CENTER: (0.5, 0.5), C_LEFT: (1.0, 0.5), C_TOPLEFT: (1.0, 1.0), C_TOP: (0.5, 1.0), C_BOTTOMLEFT: (1.0, 0.0), C_BOTTOM: (0.5, 0.0)}

PRIMARIES_709 = ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060), (0.3127, 0.3290))
PRIMARIES_601_625 = ((0.640, 0.330), (0.290, 0.600), (0.150, 0.060), (0.3127, 0.3290))
PRIMARIES_601_525 = ((0.630, 0.340), (0.310, 0.595), (0.155, 0.070), (0.3127, 0.3290))
PRIMARIES_2020 = ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046), (0.3127, 0.3290))

# yuv_to_rgb.comp's sixteen values k: the term is (k - 0.5) / 255
DITHER_TABLE = np.array([[0.0625, 0.5625, 0.1875, 0.6875], [0.8125, 0.3125, 0.9375, 0.4375], [0.25, 0.75, 0.125, 0.625], [1.00, 0.5, 0.875, 0.375]])

F = np.float32


def info(bit_depth=8, msb_aligned=0, full_range=0, matrix=M_BT709, chroma_location=C_CENTER, pq=0, nv21=0):
    return dict(bit_depth=bit_depth, msb_aligned=msb_aligned, full_range=full_range, matrix=matrix, chroma_location=chroma_location, pq=pq, nv21=nv21)


# ---- planning ------------------------------------------------------------------------------------------------------------------
def _inverse3(a):
    """Adjugate / determinant of a column-major 3 x 3 (a[col][row]) in float32, the form muglm::inverse(mat3) has."""
    r = [[F(0)] * 3 for _ in range(3)]
    r[0][0] = a[1][1] * a[2][2] - a[2][1] * a[1][2]
    r[0][1] = a[2][1] * a[0][2] - a[0][1] * a[2][2]
    r[0][2] = a[0][1] * a[1][2] - a[1][1] * a[0][2]
    r[1][0] = a[2][0] * a[1][2] - a[1][0] * a[2][2]
    r[1][1] = a[0][0] * a[2][2] - a[2][0] * a[0][2]
    r[1][2] = a[1][0] * a[0][2] - a[0][0] * a[1][2]
    r[2][0] = a[1][0] * a[2][1] - a[2][0] * a[1][1]
    r[2][1] = a[2][0] * a[0][1] - a[0][0] * a[2][1]
    r[2][2] = a[0][0] * a[1][1] - a[1][0] * a[0][1]
    det = a[0][0] * r[0][0] + a[1][0] * r[0][1] + a[2][0] * r[0][2]
    return [[e / det for e in col] for col in r]


def _xyz_matrix(prims):
    """compute_xyz_matrix in float32: RGB -> XYZ for CIE xy chromaticities of the primaries and the white point; column major.  Not
    video_ref's: that one inverts in float64 (numpy), this one rounds every operation to float32 in the product's order."""
    cols = [[F(x) / F(y), F(1.0), (F(1.0) - F(x) - F(y)) / F(y)] for x, y in prims]
    p, white = cols[:3], cols[3]
    inv = _inverse3(p)
    out = []
    for c in range(3):
        scale = inv[0][c] * white[0] + inv[1][c] * white[1] + inv[2][c] * white[2]
        out.append([p[c][r] * scale for r in range(3)])
    return out


def _mul(a, b, n):
    """Column-major n x n product, each element summed in column order (muglm's mat * vec)."""
    out = []
    for c in range(n):
        col = []
        for r in range(n):
            acc = a[0][r] * b[c][0]
            for k in range(1, n):
                acc = acc + a[k][r] * b[c][k]
            col.append(acc)
        out.append(col)
    return out


def _mat4(m3=None):
    m = [[F(1.0) if r == c else F(0.0) for r in range(4)] for c in range(4)]
    if m3 is not None:
        for c in range(3):
            for r in range(3):
                m[c][r] = F(m3[c][r])
    return m


def plan(planes, out, inf):
    """init_yuv_to_rgb + dispatch_conversion: planes = [(w, h, format), ...], out = (w, h, format), inf = info(...).  Returns the
    UBO's members as float32 (matrices column major, shape (4, 4) indexed [col][row]) and the specialization constants, or None
    where the conversion is refused."""
    n = len(planes)
    if not 1 <= n <= 3:
        return None
    w, h, yfmt = planes[0]
    if yfmt not in (R8, R16) or w < 1 or h < 1 or w > 65535 or h > 65535:
        return None
    wide = yfmt == R16
    depth = inf["bit_depth"]
    if depth not in (8, 10, 16) or (depth == 8) == wide:
        return None
    if inf["matrix"] not in range(6) or inf["chroma_location"] not in SITING or (inf["nv21"] and n != 2):
        return None
    sub = False
    if n > 1:
        cw, ch = planes[1][0], planes[1][1]
        sub = cw < w or ch < h
        if (cw, ch) != (((w + 1) // 2, (h + 1) // 2) if sub else (w, h)):
            return None
        want = (R16G16 if wide else R8G8) if n == 2 else yfmt
        if any(tuple(q) != (cw, ch, want) for q in planes[1:]):
            return None
    rgba8 = out[2] in (RGBA8, RGBA8_SRGB)
    if out[2] not in (RGBA8, RGBA8_SRGB, A2B10G10R10, RGBA16F) or rgba8 == bool(inf["pq"]) or tuple(out[:2]) != (w, h):
        return None

    inv_res = (F(1.0) / F(w), F(1.0) / F(h))
    half = F(0.5) * F(2 if sub else 1)
    clamp = ((F(w) - half) * inv_res[0], (F(h) - half) * inv_res[1])
    rescale = F(1.0)
    if depth == 10:
        rescale = F(0xffff) / F(1023 << 6) if inf["msb_aligned"] else F(0xffff) / F(1023)

    full = bool(inf["full_range"])
    luma_offset = (0 if full else 16) << (depth - 8)
    luma_narrow, chroma_narrow = 219 << (depth - 8), 224 << (depth - 8)
    midpoint, unorm_range = F(1 << (depth - 1)), F((1 << depth) - 1)
    divider = F(1.0) / unorm_range
    shift = -midpoint * divider
    bias = (F(-luma_offset) * divider, shift, shift)
    scale = (F(1.0),) * 3 if full else (unorm_range / F(luma_narrow), unorm_range / F(chroma_narrow), unorm_range / F(chroma_narrow))

    matrix = inf["matrix"]
    if matrix == M_UNSPECIFIED:
        matrix = M_BT601_525 if h < 625 else M_BT601_625 if h < 720 else M_BT709 if h < 2160 else M_BT2020
    coeff = {M_BT709: (F(-0.13397432) / F(0.7152), F(1.8556), F(1.5748), F(-0.33480248) / F(0.7152), None),
             M_BT2020: (F(-0.11156702) / F(0.6780), F(1.8814), F(1.4746), F(-0.38737742) / F(0.6780), PRIMARIES_2020),
             M_BT601_525: (F(-0.202008) / F(0.587), F(1.772), F(1.402), F(-0.419198) / F(0.587), PRIMARIES_601_525),
             M_BT601_625: (F(-0.202008) / F(0.587), F(1.772), F(1.402), F(-0.419198) / F(0.587), PRIMARIES_601_625),
             M_SMPTE240M: (F(-0.58862) / F(0.701), F(1.826), F(1.576), F(-0.334112) / F(0.701), PRIMARIES_601_525)}[matrix]
    g_cb, b_cb, r_cr, g_cr, source = coeff
    m = _mat4([[1.0, 1.0, 1.0], [0.0, g_cb, b_cb], [r_cr, g_cr, 0.0]])
    s = _mat4()
    t = _mat4()
    for i in range(3):
        s[i][i] = scale[i]
        t[3][i] = bias[i]
    to_rgb = _mul(_mul(m, s, 4), t, 4)
    conv = _mat4(_mul(_inverse3(_xyz_matrix(PRIMARIES_709)), _xyz_matrix(source), 3)) if source else _mat4()
    return {"yuv_to_rgb": np.array(to_rgb, np.float32), "primary_conversion": np.array(conv, np.float32), "resolution": (w, h),
            "inv_resolution": inv_res, "chroma_siting": tuple(F(v) for v in SITING[inf["chroma_location"]]), "chroma_clamp": clamp,
            "unorm_rescale": rescale, "spec_pq": int(out[2] == RGBA16F), "spec_num_planes": n, "spec_nv21": int(bool(inf["nv21"])),
            "matrix": matrix}


# ---- pixels --------------------------------------------------------------------------------------------------------------------
def _linear_axis(c, n):
    """linear_axis at normalised float32 coordinates c over n texels: clamped tap indices and the second tap's weight."""
    snap = F(1.0 / 256.0)
    f = (c * F(n) - F(0.5)).astype(np.float32)
    fl = np.floor(f + snap)
    a = (f - fl).astype(np.float32)
    a[a < snap] = 0.0
    i0 = fl.astype(np.int64)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), a


def chroma_taps(p, cw, ch):
    """The taps the shader's chroma fetch resolves to: (x0, x1, a) per output column and (y0, y1, b) per output row."""
    w, h = p["resolution"]
    u = np.minimum((np.arange(w, dtype=np.float32) + p["chroma_siting"][0]) * p["inv_resolution"][0], p["chroma_clamp"][0]).astype(np.float32)
    v = np.minimum((np.arange(h, dtype=np.float32) + p["chroma_siting"][1]) * p["inv_resolution"][1], p["chroma_clamp"][1]).astype(np.float32)
    return _linear_axis(u, cw), _linear_axis(v, ch)


def _sample_chroma(img, p, dtype):
    """LinearClamp fetch of img (ch, cw, channels), decoded, at every output pixel."""
    ch, cw = img.shape[:2]
    (x0, x1, a), (y0, y1, b) = chroma_taps(p, cw, ch)
    a = a[None, :, None].astype(dtype)
    b = b[:, None, None].astype(dtype)
    one = dtype(1.0)
    t00, t10 = img[y0][:, x0], img[y0][:, x1]
    t01, t11 = img[y1][:, x0], img[y1][:, x1]
    return t00 * ((one - a) * (one - b)) + t10 * (a * (one - b)) + t01 * ((one - a) * b) + t11 * (a * b)


def _pow(x, e, dtype):
    if dtype is np.float64:
        return np.power(x, e)
    with np.errstate(divide="ignore"):
        return np.exp2((dtype(e) * np.log2(x).astype(dtype)).astype(dtype)).astype(dtype)


def shade(planes, p, dtype=np.float64):
    """yuv_to_rgb.comp at every pixel: planes are the stored integer texels ((h, w), chroma (ch, cw) or (ch, cw, 2)); p a plan.
    Returns the (h, w, 3) value handed to imageStore, before the store's own conversion, in `dtype`."""
    w, h = p["resolution"]
    unorm = dtype(65535.0 if planes[0].dtype == np.uint16 else 255.0)
    y = planes[0].astype(dtype) / unorm
    assert y.shape == (h, w)
    n = p["spec_num_planes"]
    if n == 3:
        c = _sample_chroma(np.stack([planes[1], planes[2]], axis=-1).astype(dtype) / unorm, p, dtype)
    elif n == 2:
        c = _sample_chroma(planes[1].astype(dtype) / unorm, p, dtype)
        if p["spec_nv21"]:
            c = c[..., ::-1]
    else:
        c = np.full((h, w, 2), dtype(128.0) / dtype(255.0), dtype)
    yuv = np.concatenate([y[..., None], c], axis=-1).astype(dtype) * dtype(p["unorm_rescale"])
    m = p["yuv_to_rgb"].astype(dtype)  # [col][row]
    rgb = yuv[..., 0:1] * m[0][:3] + yuv[..., 1:2] * m[1][:3] + yuv[..., 2:3] * m[2][:3] + m[3][:3]
    rgb = np.clip(rgb.astype(dtype), dtype(0.0), dtype(1.0))
    if p["spec_pq"]:
        m1, m2, c2, c3 = 0.1593017578125, 78.84375, 18.8515625, 18.6875
        c1 = c3 - c2 + 1.0
        e = _pow(rgb, 1.0 / m2, dtype)
        num = np.maximum(e - dtype(c1), dtype(0.0))
        den = dtype(c2) - dtype(c3) * e
        rgb = (_pow((num / den).astype(dtype), 1.0 / m1, dtype) * dtype(10000.0 / 80.0)).astype(dtype)
        pc = p["primary_conversion"].astype(dtype)
        rgb = rgb[..., 0:1] * pc[0][:3] + rgb[..., 1:2] * pc[1][:3] + rgb[..., 2:3] * pc[2][:3]
    else:
        ys, xs = np.arange(h), np.arange(w)
        d = ((DITHER_TABLE[ys[:, None] & 3, xs[None, :] & 3] - 0.5) / 255.0).astype(dtype)
        rgb = rgb + d[..., None]
    return rgb.astype(dtype)


def pq_fp32_allowance(planes, p):
    """First-order bound on what an fp32 evaluation of the PQ branch may differ from the exact value, per output channel (h, w, 3).
    d = 2^-23 is one fp32 ulp: the precision of a hardware exp2 / log2 and twice that of a correctly rounded operation.  With x the
    clamped non-linear channel, e = x^(1/m2) carries a relative error of d (2 + |ln x| / m2); num = e - c1 and den = c2 - c3 e carry
    that as an absolute error (e <= 1), so q = num / den is off by e_err (1 / num + c3 / den) + 2 d relatively -- the cancellation in
    num is what makes dark channels ill-conditioned; the second pow multiplies by 1 / m1 = 6.28 and adds d (2 + |ln q| / m1).  The
    primary conversion then sums |coefficient| x absolute error: where its terms cancel (saturated colours outside the BT.709 gamut)
    the result is small and the error is not."""
    d = 2.0 ** -23
    m1, m2, c2, c3 = 0.1593017578125, 78.84375, 18.8515625, 18.6875
    c1 = c3 - c2 + 1.0
    q = dict(p)
    q["spec_pq"] = 0
    x = np.clip(shade(planes, q) - ((DITHER_TABLE[np.arange(p["resolution"][1])[:, None] & 3, np.arange(p["resolution"][0])[None, :] & 3] - 0.5) / 255.0)[..., None], 0.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = x ** (1.0 / m2)
        e_err = d * (2.0 + np.abs(np.log(np.maximum(x, 1e-30))) / m2)
        num, den = np.maximum(e - c1, 0.0), c2 - c3 * e
        ratio = num / den
        q_rel = e_err * (1.0 / num + c3 / den) + 2.0 * d
        lin = ratio ** (1.0 / m1) * 125.0
        lin_rel = q_rel / m1 + d * (2.0 + np.abs(np.log(np.maximum(ratio, 1e-30))) / m1)
        dlin = np.where(num > 0.0, lin * lin_rel, 0.0)
    dlin = np.nan_to_num(dlin, nan=0.0, posinf=0.0) + d * lin
    pc = np.abs(p["primary_conversion"].astype(np.float64))
    return dlin[..., 0:1] * pc[0][:3] + dlin[..., 1:2] * pc[1][:3] + dlin[..., 2:3] * pc[2][:3]


def store(rgb, out_format):
    """imageStore of vec4(rgb, 1): (h, w, 4) integer codes for the UNORM formats (A2B10G10R10: r, g, b of 1023 and alpha 3),
    fp16 bits for RGBA16F."""
    h, w = rgb.shape[:2]
    if out_format == RGBA16F:
        out = np.ones((h, w, 4), np.float16)
        out[..., :3] = rgb.astype(np.float16)
        return out.view(np.uint16)
    scale, alpha = (1023.0, 3) if out_format == A2B10G10R10 else (255.0, 255)
    out = np.full((h, w, 4), alpha, np.int64)
    out[..., :3] = np.floor(np.clip(rgb.astype(np.float64), 0.0, 1.0) * scale + 0.5)
    return out


def yuv_to_rgb(planes, out_format, inf, dtype=np.float64):
    """Expected output of gr_video_yuv_to_rgb for stored planes (numpy arrays) and info(...)."""
    dims = [(q.shape[1], q.shape[0], {(1, 2): R8, (2, 2): R16, (1, 3): R8G8, (2, 3): R16G16}[(q.dtype.itemsize, q.ndim)]) for q in planes]
    p = plan(dims, (dims[0][0], dims[0][1], out_format), inf)
    assert p is not None, "refused"
    return store(shade(planes, p, dtype), out_format)


def unpack_a2b10g10r10(words):
    u = np.asarray(words, np.uint32)
    return np.stack([u & 1023, (u >> 10) & 1023, (u >> 20) & 1023, u >> 30], axis=-1).astype(np.int64)


# ---- probes with exact answers ---------------------------------------------------------------------------------------------------
def dither_probe():
    """A 64 x 16 gray frame whose stored codes are decided by the dither term alone: one R8 plane (no chroma: the constant 128 / 255
    cancels against the 8-bit chroma bias up to ~1e-8), limited range, BT.709, so r = g = b = (Y - 16) / 219.  Each 4 x 4 block holds
    one luma code Y, taken in ascending order from those for which the stored value stays at least 0.02 code away from a rounding
    midpoint under all sixteen dither terms (n / 16 - 0.5) / 255, n = 1 .. 16, both as an 8-bit and as a 10-bit code: 0.02 code of
    1023 is 2e-5 of the value, a hundred fp32 roundings.  Expected codes are computed in exact rational arithmetic.  Returns (plane,
    RGBA8 codes (h, w, 4), A2B10G10R10 codes (h, w, 4) as r, g, b, alpha 3)."""
    from fractions import Fraction as Q
    import math
    h, w = 16, 64
    terms = [Q(n, 16) - Q(1, 2) for n in range(1, 17)]

    def codes(t, n16, scale):
        v = (Q(t, 219) + (Q(n16).limit_denominator(16) - Q(1, 2)) / 255) * scale + Q(1, 2)
        return math.floor(v), abs(v - round(v))

    def margin(t, scale):
        return min(abs((Q(t, 219) + d / 255) * scale + Q(1, 2) - round((Q(t, 219) + d / 255) * scale + Q(1, 2))) for d in terms)

    good = [t for t in range(1, 219) if margin(t, 255) >= Q(1, 50) and margin(t, 1023) >= Q(1, 50)]
    assert len(good) >= 64, len(good)
    plane = np.zeros((h, w), np.uint8)
    c8 = np.zeros((h, w), np.int64)
    c10 = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            t = good[(y // 4) * 16 + x // 4]
            plane[y, x] = 16 + t
            c8[y, x] = codes(t, DITHER_TABLE[y & 3, x & 3], 255)[0]
            c10[y, x] = codes(t, DITHER_TABLE[y & 3, x & 3], 1023)[0]
    rep = lambda c, a: np.concatenate([np.repeat(c[..., None], 3, axis=-1), np.full((h, w, 1), a)], axis=-1)
    return plane, rep(c8, 255), rep(c10, 3)


PROBE_STEP = 3


def coordinate_probe(w, h, sub, location):
    """Chroma planes whose texels encode their own coordinates (Cb = PROBE_STEP * column, Cr = PROBE_STEP * row, up to 85 x 85 chroma texels), a
    flat luma plane, and what the bilinear fetch must return at every output pixel, computed from first principles in exact rational
    arithmetic: the tap position is min((x + siting) / w, (w - 0.5 * s) / w) * cw - 0.5 with s = 2 for 4:2:0, clamped to the plane;
    sitings and sizes make it a multiple of 1/4 except where chroma_clamp bites on an odd 4:2:0 size, where it is compared with a
    tolerance of 2^-8 texel (the sampler's stated resolution).  Returns (planes [Y, Cb, Cr], expected Cb position, expected Cr
    position) with positions in texels."""
    from fractions import Fraction as Q
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub else (w, h)
    assert cw <= 85 and ch <= 85
    y = np.full((h, w), 128, np.uint8)
    cb = np.tile((PROBE_STEP * np.arange(cw)).astype(np.uint8), (ch, 1))
    cr = np.tile((PROBE_STEP * np.arange(ch)).astype(np.uint8)[:, None], (1, cw))
    sx, sy = SITING[location]
    s = 2 if sub else 1

    def axis(n, cn, siting):
        out = []
        for i in range(n):
            u = min((Q(i) + Q(siting)) / n, (Q(n) - Q(s) / 2) / n)
            out.append(float(min(max(u * cn - Q(1, 2), Q(0)), Q(cn - 1))))
        return np.array(out)

    return [y, cb, cr], axis(w, cw, sx), axis(h, ch, sy)
