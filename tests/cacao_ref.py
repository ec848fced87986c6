"""Reference for the SSAO stages (granite_amd/csrc/cacao_core.hpp): a numpy restatement of ffx_cacao.hlsl in the shader's operation order,
with a dtype switch.  float32 evaluates every operation in fp32 (numpy's are correctly rounded, sqrt and divide included) and rounds to
fp16 at the pack points; float64 evaluates the same formulae without the fp32 roundings.  Each stage takes the previous stage's STORED
bytes.  Nothing here reads the code under test.

Rules that the text of the shader does not settle (stated once more in cacao_core.hpp):
  - samplers are what ffx_cacao_impl.cpp:513-562 creates: g_PointClampSampler and g_PointMirrorSampler filter linearly with the nearest mip,
    g_LinearClampSampler is linear, g_ViewspaceDepthTapSampler is nearest / nearest mip / clamp;
  - linear filtering: per axis linear_axis(u * size - 0.5), exact weights, a coordinate within 2^-8 of a texel centre reads that texel
    alone; two lerps along x, t (1 - a) + t' a, then one along y; a weight of exactly 0 does not read its texel;
  - a gather ignores the filter and returns texels (i0, j0 + 1), (i0 + 1, j0 + 1), (i0 + 1, j0), (i0, j0) with i0, j0 from linear_axis;
  - nearest texel floor(u size) clamped, nearest mip ceil(lod + 0.5) - 1 clamped to [0, 3]; mirrored repeat reflects about the edge;
  - a load outside the image is zero, a store outside it is dropped; mip k of an extent n is max(1, n >> k);
  - min16float is fp32 with fp16 rounding where the shader packs with f32tof16;
  - normalize(v) = v / sqrt(dot(v, v)), dot and mul sum left to right, round() is to nearest even, max / min / saturate drop a NaN;
  - UNORM8 loads v / 255, SNORM8 loads max(v / 127, -1), UNORM10 loads v / 1023; UNORM8 stores uint(saturate(c) 255 + 0.5), SNORM8 stores
    floor(clamp(c, -1, 1) 127 + 0.5).
"""
import numpy as np

QUALITY_HIGH, QUALITY_HIGHEST = 3, 4
PASSES, DEPTH_MIPS = 4, 4
MAX_TAPS, BASE_TAPS, Q2_TAPS = 32, 5, 12
FLEXIBLE_TAPS = MAX_TAPS - BASE_TAPS
SNAP = 1.0 / 256.0
LOD_FLAG_DISTANCE = 2.0 ** -10

CONSTANTS_DTYPE = np.dtype([
    ("DepthUnpackConsts", "<f4", 2), ("CameraTanHalfFOV", "<f4", 2), ("NDCToViewMul", "<f4", 2), ("NDCToViewAdd", "<f4", 2),
    ("DepthBufferUVToViewMul", "<f4", 2), ("DepthBufferUVToViewAdd", "<f4", 2),
    ("EffectRadius", "<f4"), ("EffectShadowStrength", "<f4"), ("EffectShadowPow", "<f4"), ("EffectShadowClamp", "<f4"),
    ("EffectFadeOutMul", "<f4"), ("EffectFadeOutAdd", "<f4"), ("EffectHorizonAngleThreshold", "<f4"), ("EffectSamplingRadiusNearLimitRec", "<f4"),
    ("DepthPrecisionOffsetMod", "<f4"), ("NegRecEffectRadius", "<f4"), ("LoadCounterAvgDiv", "<f4"), ("AdaptiveSampleCountLimit", "<f4"),
    ("InvSharpness", "<f4"), ("PassIndex", "<i4"), ("BilateralSigmaSquared", "<f4"), ("BilateralSimilarityDistanceSigma", "<f4"),
    ("PatternRotScaleMatrices", "<f4", (5, 4)),
    ("NormalsUnpackMul", "<f4"), ("NormalsUnpackAdd", "<f4"), ("DetailAOStrength", "<f4"), ("Dummy0", "<f4"),
    ("SSAOBufferDimensions", "<f4", 2), ("SSAOBufferInverseDimensions", "<f4", 2),
    ("DepthBufferDimensions", "<f4", 2), ("DepthBufferInverseDimensions", "<f4", 2),
    ("DepthBufferOffset", "<i4", 2), ("PerPassFullResUVOffset", "<f4", 2),
    ("InputOutputBufferDimensions", "<f4", 2), ("InputOutputBufferInverseDimensions", "<f4", 2),
    ("ImportanceMapDimensions", "<f4", 2), ("ImportanceMapInverseDimensions", "<f4", 2),
    ("DeinterleavedDepthBufferDimensions", "<f4", 2), ("DeinterleavedDepthBufferInverseDimensions", "<f4", 2),
    ("DeinterleavedDepthBufferOffset", "<f4", 2), ("DeinterleavedDepthBufferNormalisedOffset", "<f4", 2),
    ("NormalsWorldToViewspaceMatrix", "<f4", (4, 4)),
])
assert CONSTANTS_DTYPE.itemsize == 384
BUFFER_SIZES_FIELDS = ("inputOutputBufferWidth", "inputOutputBufferHeight", "ssaoBufferWidth", "ssaoBufferHeight", "depthBufferXOffset",
                       "depthBufferYOffset", "depthBufferWidth", "depthBufferHeight", "deinterleavedDepthBufferXOffset",
                       "deinterleavedDepthBufferYOffset", "deinterleavedDepthBufferWidth", "deinterleavedDepthBufferHeight", "importanceMapWidth",
                       "importanceMapHeight", "downsampledSsaoBufferWidth", "downsampledSsaoBufferHeight")

# g_FFX_CACAO_samplePatternMain, ffx_cacao.hlsl:25-35
PATTERN = np.array([np.float32(t) for t in """
 0.78488064  0.56661671  1.500000 -0.126083     0.26022232 -0.29575172  1.500000 -1.064030     0.10459357  0.08372527  1.110000 -2.730563    -0.68286800  0.04963045  1.090000 -0.498827
-0.13570161 -0.64190155  1.250000 -0.532765    -0.26193795 -0.08205118  0.670000 -1.783245    -0.61177456  0.66664219  0.710000 -0.044234     0.43675563  0.25119025  0.610000 -1.167283
 0.07884444  0.86618668  0.640000 -0.459002    -0.12790935 -0.29869005  0.600000 -1.729424    -0.04031125  0.02413622  0.600000 -4.792042     0.16201244 -0.52851415  0.790000 -1.067055
-0.70991218  0.47301072  0.640000 -0.335236     0.03277707 -0.22349690  0.600000 -1.982384     0.68921727  0.36800742  0.630000 -0.266718     0.29251814  0.37775412  0.610000 -1.422520
-0.12224089  0.96582592  0.600000 -0.426142     0.11071457 -0.16131058  0.600000 -2.165947     0.46562141 -0.59747696  0.600000 -0.189760    -0.51548797  0.11804193  0.600000 -1.246800
 0.89141309 -0.42090443  0.600000  0.028192    -0.32402530 -0.01591529  0.600000 -1.543018     0.60771245  0.41635221  0.600000 -0.605411     0.02379565 -0.08239821  0.600000 -3.809046
 0.48951152 -0.23657045  0.600000 -1.189011    -0.17611565 -0.81696892  0.600000 -0.513724    -0.33930185 -0.20732205  0.600000 -1.698047    -0.91974425  0.05403209  0.600000  0.062246
-0.15064627 -0.14949332  0.600000 -1.896062     0.53180975 -0.35210401  0.600000 -0.758838     0.41487166  0.81442589  0.600000 -0.505648    -0.24106961 -0.32721516  0.600000 -1.665244
""".split()], np.float32).reshape(32, 4)


class Consts:
    """One gr_cacao_constants record with every field as `dt` (the values are the float32 ones either way)."""

    def __init__(self, record, dt):
        record = np.asarray(record).view(CONSTANTS_DTYPE).reshape(-1)[0]
        self.dt = dt
        for name in CONSTANTS_DTYPE.names:
            value = record[name]
            setattr(self, name, value.astype(dt) if CONSTANTS_DTYPE[name].base.kind == "f" else value)


def half_size(width, height):
    return (width + 1) // 2, (height + 1) // 2


def mip_extent(n, k):
    return max(1, n >> k)


# ---- small arithmetic ------------------------------------------------------------------------------------------------------------------
def sat(x):
    return np.fmin(np.fmax(x, 0), 1)


def unorm8(b, dt):
    return b.astype(dt) / dt(255.0)


def snorm8(b, dt):
    return np.fmax(b.view(np.int8).astype(dt) / dt(127.0), dt(-1.0))


def to_unorm8(c, dt):
    return (sat(c) * dt(255.0) + dt(0.5)).astype(np.uint32).astype(np.uint8)


def to_snorm8(c, dt):
    return np.floor(np.fmin(np.fmax(c, dt(-1.0)), dt(1.0)) * dt(127.0) + dt(0.5)).astype(np.int32).astype(np.int8).view(np.uint8)


def f16(x, dt):
    """f32tof16 then f16tof32: round to nearest even"""
    return np.asarray(x).astype(np.float16).astype(dt)


def half_bits(x):
    return np.asarray(x).astype(np.float16).view(np.uint16)


def linear_axis(f, dt):
    fl = np.floor(f + dt(SNAP))
    a = f - fl
    a = np.where(a < dt(SNAP), dt(0.0), a)
    return fl.astype(np.int64), a


def mirror(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def clamp_index(i, n):
    return np.clip(i, 0, n - 1)


def dot4(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]


def sample_linear(fetch, w, h, u, v, dt, mirrored=False):
    """fetch(x, y) takes wrapped index arrays"""
    ix, a = linear_axis(u * dt(w) - dt(0.5), dt)
    iy, b = linear_axis(v * dt(h) - dt(0.5), dt)
    wrap = mirror if mirrored else clamp_index
    x0, x1, y0, y1 = wrap(ix, w), wrap(ix + 1, w), wrap(iy, h), wrap(iy + 1, h)
    one = dt(1.0)
    t0 = fetch(x0, y0)
    t0 = np.where(a != 0, t0 * (one - a) + fetch(x1, y0) * a, t0)
    t1 = fetch(x0, y1)
    t1 = np.where(a != 0, t1 * (one - a) + fetch(x1, y1) * a, t1)
    return np.where(b != 0, t0 * (one - b) + t1 * b, t0)


# ---- prepare --------------------------------------------------------------------------------------------------------------------------
def view_depth(c, d):
    return c.DepthUnpackConsts[0] / (c.DepthUnpackConsts[1] - d)


def mip_smart_average(c, d):
    """d: four arrays in the shader's order 00, 01 (y + 1), 10 (x + 1), 11"""
    dt = c.dt
    closest = np.fmin(np.fmin(d[0], d[1]), np.fmin(d[2], d[3]))
    falloff = dt(-1.0) / c.EffectRadius * c.EffectRadius
    w = [sat((t - closest) * (t - closest) * falloff + dt(1.0)) for t in d]
    one = dt(1.0)
    return dot4(w, d) / dot4(w, [one, one, one, one])


def prepare_depths(depth, constants, dt=np.float32):
    """depth (H, W) float32 -> [mip k: (4, h_k, w_k) uint16 fp16 bits for k in 0 .. 3]"""
    c = Consts(constants, dt)
    H, W = depth.shape
    hw, hh = half_size(W, H)
    gw, gh = -(-hw // 8) * 8, -(-hh // 8) * 8  # whole 8 x 8 groups: lanes past the extent gather clamped texels
    tx, ty = np.arange(gw), np.arange(gh)
    u = (dt(2.0) * tx.astype(dt) + dt(0.5)) * c.DepthBufferInverseDimensions[0]
    v = (dt(2.0) * ty.astype(dt) + dt(0.5)) * c.DepthBufferInverseDimensions[1]
    ix, _ = linear_axis(u * dt(W) - dt(0.5), dt)
    iy, _ = linear_axis(v * dt(H) - dt(0.5), dt)
    x0, x1, y0, y1 = clamp_index(ix, W), clamp_index(ix + 1, W), clamp_index(iy, H), clamp_index(iy + 1, H)
    d = depth.astype(dt)
    level = np.stack([view_depth(c, d[np.ix_(y0, x0)]), view_depth(c, d[np.ix_(y0, x1)]), view_depth(c, d[np.ix_(y1, x0)]), view_depth(c, d[np.ix_(y1, x1)])])
    mips = []
    for k in range(DEPTH_MIPS):
        mips.append(half_bits(level[:, :mip_extent(hh, k), :mip_extent(hw, k)]))
        if k + 1 < DEPTH_MIPS:
            level = mip_smart_average(c, [level[:, 0::2, 0::2], level[:, 1::2, 0::2], level[:, 0::2, 1::2], level[:, 1::2, 1::2]])
    return mips


def prepare_normals(normal, constants, dt=np.float32):
    """normal (H, W) uint32 A2B10G10R10 -> (4, h, w, 4) uint8 RGBA8_SNORM"""
    c = Consts(constants, dt)
    H, W = normal.shape
    hw, hh = half_size(W, H)
    padded = np.zeros((2 * hh, 2 * hw), np.uint32)  # a load past the image is zero
    padded[:H, :W] = normal
    out = np.zeros((PASSES, hh, hw, 4), np.uint8)
    m = c.NormalsWorldToViewspaceMatrix  # m[column][row]
    for layer in range(PASSES):
        word = padded[layer >> 1::2, layer & 1::2]
        n = [((word >> s) & 1023).astype(dt) / dt(1023.0) * c.NormalsUnpackMul + c.NormalsUnpackAdd for s in (0, 10, 20)]
        vx = m[0][0] * n[0] + m[1][0] * n[1] + m[2][0] * n[2]
        vy = m[0][1] * n[0] + m[1][1] * n[1] + m[2][1] * n[2]
        vz = -(m[0][2] * n[0] + m[1][2] * n[1] + m[2][2] * n[2])
        length = np.sqrt(vx * vx + vy * vy + vz * vz)
        out[layer, ..., 0] = to_snorm8(vx / length, dt)
        out[layer, ..., 1] = to_snorm8(vy / length, dt)
        out[layer, ..., 2] = to_snorm8(vz / length, dt)
        out[layer, ..., 3] = to_snorm8(np.full_like(vx, 1.0), dt)
    return out


# ---- generate -------------------------------------------------------------------------------------------------------------------------
def _depth_tap(mips_f, p, u, v, lod, dt, stats):
    t = np.ceil(lod + dt(0.5)) - dt(1.0)
    with np.errstate(invalid="ignore"):
        mip = np.where(t > 0, np.where(t < 3, t, 3), 0).astype(np.int64)
    out = np.zeros(u.shape, dt)
    for k in range(DEPTH_MIPS):
        hk, wk = mips_f[k].shape[1:]
        x = np.fmin(np.fmax(np.floor(u * dt(wk)), 0), wk - 1).astype(np.int64)
        y = np.fmin(np.fmax(np.floor(v * dt(hk)), 0), hk - 1).astype(np.int64)
        out = np.where(mip == k, mips_f[k][p][y, x], out)
    if stats is not None:
        stats["mip"] = mip
        stats["outside"] = (u < 0) | (u >= 1) | (v < 0) | (v >= 1)
    return out


def _obscurance(c, n, d, falloff_mul_sq):
    dt = c.dt
    length_sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        n_dot_d = (n[0] * d[0] + n[1] * d[1] + n[2] * d[2]) / np.sqrt(length_sq)
    falloff = np.fmax(dt(0.0), length_sq * falloff_mul_sq + dt(1.0))
    return np.fmax(dt(0.0), n_dot_d - c.EffectHorizonAngleThreshold) * falloff


def pack_edges(e, dt):
    r = [np.rint(sat(t) * dt(3.05)) for t in e]
    return dot4(r, [dt(64.0) / dt(255.0), dt(16.0) / dt(255.0), dt(4.0) / dt(255.0), dt(1.0) / dt(255.0)])


def unpack_edges(c, packed_value):
    dt = c.dt
    packed = (packed_value * dt(255.5)).astype(np.uint32)
    return [sat(((packed >> s) & 3).astype(dt) / dt(3.0) + c.InvSharpness) for s in (6, 4, 2, 0)]


def generate(depth_mips, normals, constants4, quality, base=False, dt=np.float32, importance=None, base_ssao=None, load_counter=None):
    """One launch of GenerateQ3Base (base=True), GenerateQ2 (QUALITY_HIGH) or GenerateQ3 (QUALITY_HIGHEST) over the four passes.
    depth_mips: prepare_depths' list; normals (4, h, w, 4) uint8; Q3 also takes the importance map (ih, iw) uint8, the base pass's output
    (4, h, w, 2) uint8 and the load counter.  Returns (out (4, h, w, 2) uint8, info): info["flag"] (4, h, w) bool marks texels where some
    tap's lod + 0.5 lies within 2^-10 of 1, 2 or 3; info["taps"] (4, h, w) the tap pairs taken; info["max_mip"] the highest mip read;
    info["outside"] whether some tap landed outside the image; info["values"] the two channels before the store."""
    level = 3 if (base or quality == QUALITY_HIGHEST) else 2
    adaptive = level == 3 and not base
    mips_f = [m.view(np.float16).astype(dt) for m in depth_mips]
    hh, hw = mips_f[0].shape[1:]
    out = np.zeros((PASSES, hh, hw, 2), np.uint8)
    info = {"flag": np.zeros((PASSES, hh, hw), bool), "taps": np.zeros((PASSES, hh, hw), np.int32), "max_mip": 0, "outside": False,
            "values": np.zeros((PASSES, hh, hw, 2), dt)}
    X, Y = np.meshgrid(np.arange(hw), np.arange(hh))
    one, half, zero = dt(1.0), dt(0.5), dt(0.0)
    for p in range(PASSES):
        c = Consts(constants4[p], dt)
        svx, svy = X.astype(dt), Y.astype(dt)
        inv_w, inv_h = c.DeinterleavedDepthBufferInverseDimensions
        uvx = (svx + half) * inv_w + c.DeinterleavedDepthBufferNormalisedOffset[0]
        uvy = (svy + half) * inv_h + c.DeinterleavedDepthBufferNormalisedOffset[1]
        ix, _ = linear_axis(uvx * dt(hw) - half, dt)
        iy, _ = linear_axis(uvy * dt(hh) - half, dt)
        d0 = mips_f[0][p]
        xl, xc, xr = mirror(ix - 1, hw), mirror(ix, hw), mirror(ix + 1, hw)
        yt, yc, yb = mirror(iy - 1, hh), mirror(iy, hh), mirror(iy + 1, hh)
        pix_z, pix_lz, pix_tz, pix_rz, pix_bz = d0[yc, xc], d0[yc, xl], d0[yt, xc], d0[yc, xr], d0[yb, xc]
        nsx, nsy = (svx + half) * c.SSAOBufferInverseDimensions[0], (svy + half) * c.SSAOBufferInverseDimensions[1]
        centre = [(c.NDCToViewMul[0] * nsx + c.NDCToViewAdd[0]) * pix_z, (c.NDCToViewMul[1] * nsy + c.NDCToViewAdd[1]) * pix_z, pix_z]
        npad = np.zeros((hh + 2, hw + 2, 3), dt)  # zero outside the image
        npad[1:-1, 1:-1] = snorm8(normals[p][..., :3], dt)
        n = [npad[1:-1, 1:-1, k] for k in range(3)]
        size_x = centre[2] * c.NDCToViewMul[0] * c.SSAOBufferInverseDimensions[0]
        size_y = centre[2] * c.NDCToViewMul[1] * c.SSAOBufferInverseDimensions[1]
        centre_length = np.sqrt(centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2])
        too_close = sat(centre_length * c.EffectSamplingRadiusNearLimitRec) * dt(0.8) + dt(0.2)
        effect_radius = c.EffectRadius * too_close
        lookup = (dt(0.85) * effect_radius) / size_x
        falloff_mul_sq = dt(-1.0) / (effect_radius * effect_radius)
        pri = (svy * dt(2.0) + svx).astype(np.uint32) % 5
        rs = c.PatternRotScaleMatrices[pri]  # (h, w, 4)
        m00, m01, m10, m11 = rs[..., 0] * lookup, rs[..., 1] * lookup, rs[..., 2] * lookup, rs[..., 3] * lookup
        osum, wsum = np.zeros((hh, hw), dt), np.zeros((hh, hw), dt)
        edges = [np.ones((hh, hw), dt) for _ in range(4)]
        centre = [t * c.DepthPrecisionOffsetMod for t in centre]
        if not base:
            dl, dr, dtt, db = pix_lz - pix_z, pix_rz - pix_z, pix_tz - pix_z, pix_bz - pix_z
            adj = [dl + dr, dr + dl, dtt + db, db + dtt]
            denom = pix_z * dt(0.040)
            edges = [sat(dt(1.3) - np.fmin(np.abs(e), np.abs(a)) / denom) for e, a in zip((dl, dr, dtt, db), adj)]
            vx, vy = centre[0] / centre[2], centre[1] / centre[2]
            zs = [pix_lz - centre[2], pix_rz - centre[2], pix_tz - centre[2], pix_bz - centre[2]]
            modified = dt(4.0) * falloff_mul_sq
            firsts = [(-size_x, zero), (size_x, zero), (zero, -size_y), (zero, size_y)]
            add = [_obscurance(c, n, [fx + vx * z, fy + vy * z, zero + one * z], modified) for (fx, fy), z in zip(firsts, zs)]
            osum = osum + c.DetailAOStrength * dot4(add, edges)
            for k, (ox, oy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
                nb = npad[1 + oy:hh + 1 + oy, 1 + ox:hw + 1 + ox]
                edges[k] = edges[k] * sat(n[0] * nb[..., 0] + n[1] * nb[..., 1] + n[2] * nb[..., 2] + half)
        with np.errstate(invalid="ignore", divide="ignore"):
            mip_offset = np.log2(lookup) + dt(-4.3)
        first, last = 0, np.full((hh, hw), BASE_TAPS if base else Q2_TAPS)
        if adaptive:
            imp = importance
            ih, iw = imp.shape
            full_u, full_v = nsx + c.PerPassFullResUVOffset[0], nsy + c.PerPassFullResUVOffset[1]
            importance_value = sample_linear(lambda x, y: unorm8(imp[y, x], dt), iw, ih, full_u, full_v, dt)
            osum = osum * ((dt(BASE_TAPS) / dt(MAX_TAPS)) + (importance_value * dt(FLEXIBLE_TAPS) / dt(MAX_TAPS)))
            wsum = wsum + unorm8(base_ssao[p][..., 1], dt) * dt(BASE_TAPS * 4.0)
            osum = osum + unorm8(base_ssao[p][..., 0], dt) * wsum
            with np.errstate(invalid="ignore", divide="ignore"):
                average = dt(np.uint32(load_counter)) * c.LoadCounterAvgDiv
                importance_value = importance_value * sat(c.AdaptiveSampleCountLimit / average)
            additional = (dt(FLEXIBLE_TAPS) * importance_value + dt(1.5)).astype(np.uint32).astype(np.int64)
            first, last = BASE_TAPS, np.minimum(MAX_TAPS, additional + BASE_TAPS)
        info["taps"][p] = last - first
        for i in range(first, int(last.max())):
            active = i < last
            s = PATTERN[i].astype(dt)
            ox, oy = np.rint(m00 * s[0] + m01 * s[1]), np.rint(m10 * s[0] + m11 * s[1])
            lod = s[3] + mip_offset
            with np.errstate(invalid="ignore"):
                near = np.zeros((hh, hw), bool)
                for k in (1, 2, 3):
                    near |= np.abs(lod + half - dt(k)) <= dt(LOD_FLAG_DISTANCE)
            info["flag"][p] |= near & active
            if adaptive:
                du, dv = ox * inv_w, oy * inv_h
                uvs = [(uvx + du, uvy + dv), (uvx - du, uvy - dv)]
            else:
                uvs = [(ox * inv_w + uvx, oy * inv_h + uvy), (-ox * inv_w + uvx, -oy * inv_h + uvy)]
            for u, v in uvs:
                stats = {}
                z = _depth_tap(mips_f, p, u, v, lod, dt, stats)
                info["max_mip"] = max(info["max_mip"], int(stats["mip"][active].max()) if active.any() else 0)
                info["outside"] = info["outside"] or bool((stats["outside"] & active).any())
                hx = (c.DepthBufferUVToViewMul[0] * u + c.DepthBufferUVToViewAdd[0]) * z
                hy = (c.DepthBufferUVToViewMul[1] * v + c.DepthBufferUVToViewAdd[1]) * z
                delta = [hx - centre[0], hy - centre[1], z - centre[2]]
                obscurance = _obscurance(c, n, delta, falloff_mul_sq)
                reduct = np.fmax(zero, -delta[2])
                reduct = sat(reduct * c.NegRecEffectRadius + dt(2.0))
                weight = dt(0.6) * reduct + (one - dt(0.6))
                if not adaptive:
                    weight = weight * (one * s[2])
                osum = np.where(active, osum + obscurance * weight, osum)
                wsum = np.where(active, wsum + weight, wsum)
        with np.errstate(invalid="ignore", divide="ignore"):
            obscurance = osum / wsum
        if base:
            values = [obscurance, wsum / (dt(BASE_TAPS) * dt(4.0))]
        else:
            fade_out = sat(centre[2] * c.EffectFadeOutMul + c.EffectFadeOutAdd)
            edge_fade = sat((one - edges[0] - edges[1]) * dt(0.35)) + sat((one - edges[2] - edges[3]) * dt(0.35))
            fade_out = fade_out * sat(one - edge_fade)
            obscurance = c.EffectShadowStrength * obscurance
            obscurance = np.fmin(obscurance, c.EffectShadowClamp)
            obscurance = obscurance * fade_out
            values = [np.power(sat(one - obscurance), c.EffectShadowPow), pack_edges(edges, dt)]
        info["values"][p, ..., 0], info["values"][p, ..., 1] = values
        out[p, ..., 0], out[p, ..., 1] = to_unorm8(values[0], dt), to_unorm8(values[1], dt)
    return out, info


# ---- importance map -------------------------------------------------------------------------------------------------------------------
def importance_generate(pong, constants, dt=np.float32):
    """pong (4, h, w, 2) uint8 (the base pass) -> (importance (ih, iw) uint8, values before the store)"""
    c = Consts(constants, dt)
    _, hh, hw, _ = pong.shape
    iw, ih = half_size(hw, hh)
    X, Y = np.meshgrid(np.arange(iw), np.arange(ih))
    u = (dt(2.0) * X.astype(dt) + dt(0.5)) * c.SSAOBufferInverseDimensions[0]
    v = (dt(2.0) * Y.astype(dt) + dt(0.5)) * c.SSAOBufferInverseDimensions[1]
    ix, _ = linear_axis(u * dt(hw) - dt(0.5), dt)
    iy, _ = linear_axis(v * dt(hh) - dt(0.5), dt)
    x0, x1, y0, y1 = clamp_index(ix, hw), clamp_index(ix + 1, hw), clamp_index(iy, hh), clamp_index(iy + 1, hh)
    min_v, max_v = np.full((ih, iw), 1.0, dt), np.zeros((ih, iw), dt)
    for p in range(PASSES):
        vals = []
        for x, y in ((x0, y1), (x1, y1), (x1, y0), (x0, y0)):
            t = c.EffectShadowStrength * unorm8(pong[p][y, x, 0], dt)
            t = dt(1.0) - t
            vals.append(np.power(sat(t), c.EffectShadowPow))
        max_v = np.fmax(max_v, np.fmax(np.fmax(vals[0], vals[1]), np.fmax(vals[2], vals[3])))
        min_v = np.fmin(min_v, np.fmin(np.fmin(vals[0], vals[1]), np.fmin(vals[2], vals[3])))
    values = np.power(sat((max_v - min_v) * dt(2.0)), dt(0.8))
    return to_unorm8(values, dt), values


def importance_postprocess(src, constants, b, dt=np.float32):
    """PostprocessImportanceMapA (b False) or B.  Returns (map uint8, load counter contribution or None)."""
    c = Consts(constants, dt)
    ih, iw = src.shape
    X, Y = np.meshgrid(np.arange(iw), np.arange(ih))
    tap = lambda u, v: sample_linear(lambda x, y: unorm8(src[y, x], dt), iw, ih, u, v, dt)
    u = (X.astype(dt) + dt(0.5)) * c.ImportanceMapInverseDimensions[0]
    v = (Y.astype(dt) + dt(0.5)) * c.ImportanceMapInverseDimensions[1]
    centre = tap(u, v)
    hx, hy = dt(0.5) * c.ImportanceMapInverseDimensions[0], dt(0.5) * c.ImportanceMapInverseDimensions[1]
    three = dt(3.0)
    if not b:
        vals = [tap(u + -hx * three, v + -hy), tap(u + hx, v + -hy * three), tap(u + hx * three, v + hy), tap(u + -hx, v + hy * three)]
    else:
        vals = [tap(u + -hx, v + -hy * three), tap(u + hx * three, v + -hy), tap(u + hx, v + hy * three), tap(u + -hx * three, v + hy)]
    q = dt(0.25)
    avg = dot4(vals, [q, q, q, q])
    max_val = np.fmax(centre, np.fmax(np.fmax(vals[0], vals[2]), np.fmax(vals[1], vals[3])))
    result = max_val + dt(1.0) * (avg - max_val)
    counter = None
    if b:
        ninth = ((X % 3) + (Y % 3)) == 0
        counter = int((sat(result) * dt(255.0) + dt(0.5)).astype(np.uint32)[ninth].sum(dtype=np.uint64) & 0xffffffff)
    return to_unorm8(result, dt), counter


# ---- blur and apply -------------------------------------------------------------------------------------------------------------------
def blur(ping, constants, passes, dt=np.float32):
    """EdgeSensitiveBlur<passes>: ping (4, h, w, 2) uint8 -> pong.  Evaluated on the image extended by passes + 1 mirrored texels a side:
    a group's results that the image keeps depend on nothing further out, so they equal the shader's tile by tile."""
    c = Consts(constants, dt)
    _, hh, hw, _ = ping.shape
    pad = passes + 1
    X, Y = np.meshgrid(np.arange(-pad, hw + pad), np.arange(-pad, hh + pad))
    u = (X.astype(dt) + dt(0.5)) * c.SSAOBufferInverseDimensions[0]
    v = (Y.astype(dt) + dt(0.5)) * c.SSAOBufferInverseDimensions[1]
    out = np.zeros_like(ping)
    half = dt(0.5)
    for p in range(PASSES):
        layer = ping[p]
        ssao = sample_linear(lambda x, y: unorm8(layer[y, x, 0], dt), hw, hh, u, v, dt, mirrored=True)
        packed = sample_linear(lambda x, y: unorm8(layer[y, x, 1], dt), hw, hh, u, v, dt, mirrored=True)
        e = unpack_edges(c, packed)
        cur = f16(ssao, dt)
        for _ in range(passes):
            left, right = np.roll(cur, 1, axis=1), np.roll(cur, -1, axis=1)
            top, bottom = np.roll(cur, 1, axis=0), np.roll(cur, -1, axis=0)
            total, weight = cur * half, np.full(cur.shape, 0.5, dt)
            for value, edge in zip((left, right, top, bottom), e):
                total = total + value * edge
                weight = weight + edge
            cur = f16(total / weight, dt)
        out[p, ..., 0] = to_unorm8(cur, dt)[pad:-pad, pad:-pad]
        out[p, ..., 1] = to_unorm8(packed, dt)[pad:-pad, pad:-pad]
    return out


def apply(ssao, constants, width, height, dt=np.float32):
    """Apply: ssao (4, h, w, 2) uint8 (ping, or pong after a blur) -> (height, width) uint8"""
    c = Consts(constants, dt)
    _, hh, hw, _ = ssao.shape
    X, Y = np.meshgrid(np.arange(width), np.arange(height))
    hx, hy, mx, my = X // 2, Y // 2, X % 2, Y % 2
    ic, ih_, iv, id_ = mx + my * 2, (1 - mx) + my * 2, mx + (1 - my) * 2, (1 - mx) + (1 - my) * 2
    centre = ssao[ic, hy, hx]
    ao = unorm8(centre[..., 0], dt)
    e = unpack_edges(c, unorm8(centre[..., 1], dt))
    fmx, fmy, fmxe, fmye = mx.astype(dt), my.astype(dt), e[1] - e[0], e[3] - e[2]
    inx, iny = X.astype(dt), Y.astype(dt)
    isx, isy = c.SSAOBufferInverseDimensions
    half = dt(0.5)
    tap = lambda layer, u, v: sample_linear(lambda x, y: unorm8(ssao[layer, y, x, 0], dt), hw, hh, u, v, dt)
    ao_h = tap(ih_, (inx + (fmx + fmxe - half)) * half * isx, (iny + (half - fmy)) * half * isy)
    ao_v = tap(iv, (inx + (half - fmx)) * half * isx, (iny + (fmy - half + fmye)) * half * isy)
    ao_d = tap(id_, (inx + (fmx - half + fmxe)) * half * isx, (iny + (fmy - half + fmye)) * half * isy)
    one = np.ones(ao.shape, dt)
    wy, wz = (e[0] + e[1]) * half, (e[2] + e[3]) * half
    ww = (wy + wz) * half
    weights = [one, wy, wz, ww]
    total = dot4(weights, [one, one, one, one])
    return to_unorm8(dot4([ao, ao_h, ao_v, ao_d], weights) / total, dt)


# ---- the whole pass ---------------------------------------------------------------------------------------------------------------------
def chain(depth, normal, constants4, quality, blur_passes, dt=np.float32):
    """FFX_CACAO_GraniteDraw: every stage on the previous stage's stored bytes.  Returns a dict of every intermediate and "output"."""
    H, W = depth.shape
    r = {"depth_mips": prepare_depths(depth, constants4[0], dt), "normals": prepare_normals(normal, constants4[0], dt), "load_counter": 0}
    if quality == QUALITY_HIGHEST:
        r["base"], r["base_info"] = generate(r["depth_mips"], r["normals"], constants4, quality, True, dt)
        r["importance_0"], _ = importance_generate(r["base"], constants4[0], dt)
        r["importance_a"], _ = importance_postprocess(r["importance_0"], constants4[0], False, dt)
        r["importance"], r["load_counter"] = importance_postprocess(r["importance_a"], constants4[0], True, dt)
        r["ping"], r["info"] = generate(r["depth_mips"], r["normals"], constants4, quality, False, dt, r["importance"], r["base"], r["load_counter"])
    else:
        r["ping"], r["info"] = generate(r["depth_mips"], r["normals"], constants4, quality, False, dt)
    final = r["ping"]
    if blur_passes:
        r["pong"] = blur(r["ping"], constants4[0], blur_passes, dt)
        final = r["pong"]
    r["output"] = apply(final, constants4[0], W, H, dt)
    return r
