"""Directional-light shadows restated in float64 numpy: lights/directional.frag with SHADOWS (compute_lighting, compute_shadow_cascade, the
narrow and the wide PCF lookup through the LinearShadow sampler, vsm()), lights/resolve_vsm.frag and the two VSM blurs.  The sampler model is
DESIGN.md 7.17's: the footprint and weights of the LinearClamp fetch (its 2^-8 snap included), the weights applied to the 0 / 1 results of
`ref >= texel`, coordinates clamped to the edge; a D16_UNORM texel is v / 65535.

Independent of granite_amd/csrc/shadow_core.hpp in precision and in form (arrays, not lanes); tests/test_shadow_ref_cpu.py holds it to the
executed shaders (tests/golden/shadow_shader_v1.npz), and the distance between the two -- the size of an fp32 evaluation's own error -- is
what the GPU tests' bounds are derived from.

Every lookup also reports its knife edge: the smallest |ref - texel| over the taps that have a non-zero weight.  The compare is the one
discontinuity of the feature; a pixel within KNIFE_EDGE of it may fall on either side in fp32."""
import numpy as np

MODE_PCF, MODE_PCF_WIDE, MODE_VSM = 1, 2, 3
KNIFE_EDGE = 2.0 ** -20
SNAP = 1.0 / 256.0
PI_SIC = float(np.float32(3.1415628))
NUM_CASCADES = 4


def f64(a):
    return np.asarray(a, np.float64)


def const32(v):
    """a literal as the shader's fp32 holds it"""
    return float(np.float32(v))


def to_half_bits(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).view(np.uint16)


def ulp_distance(a, b):
    """Per channel: |a - b| of two float arrays after rounding to fp16, in fp16 ulps at the larger magnitude, after the standing absolute
    allowance of 1e-4 is taken off (tests/env_ref.py: ulp_distance)."""
    a = to_half_bits(a).view(np.float16).astype(np.float64)
    b = to_half_bits(b).view(np.float16).astype(np.float64)
    mag = np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -14)
    return np.maximum(np.abs(a - b) - 1e-4, 0.0) / np.exp2(np.floor(np.log2(mag)) - 10.0)


def ulp32_distance(a, b):
    """|a - b| of two fp32 arrays in fp32 ulps at the larger magnitude (moments)"""
    a, b = f64(a), f64(b)
    mag = np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -126)
    return np.abs(a - b) / np.exp2(np.floor(np.log2(mag)) - 23.0)


# ---- texels and samplers --------------------------------------------------------------------------------------------------------------
def depth_values(maps):
    """(layers, h, w) uint16 (D16_UNORM) or float32 (D32_SFLOAT) -> float64"""
    maps = np.asarray(maps)
    return maps.astype(np.float64) / 65535.0 if maps.dtype == np.uint16 else maps.astype(np.float64)


def linear_axis(f):
    fl = np.floor(f + SNAP)
    a = f - fl
    a = np.where(a < SNAP, 0.0, a)
    return fl.astype(np.int64), a


def footprint(u, v, w, h):
    x0, a = linear_axis(u * w - 0.5)
    y0, b = linear_axis(v * h - 0.5)
    xs = (np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1))
    ys = (np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1))
    weights = ((1.0 - a) * (1.0 - b), a * (1.0 - b), (1.0 - a) * b, a * b)
    return xs, ys, weights


def linear_shadow(texels, layer, u, v, ref):
    """-> (term, knife edge); texels (layers, h, w) float64, layer / u / v / ref arrays of one shape"""
    _, h, w = texels.shape
    xs, ys, weights = footprint(u, v, w, h)
    term, edge = np.zeros_like(ref), np.full(ref.shape, np.inf)
    for (ix, iy), wt in zip(((0, 0), (1, 0), (0, 1), (1, 1)), weights):
        t = texels[layer, ys[iy], xs[ix]]
        term = term + wt * (ref >= t)
        edge = np.where(wt != 0.0, np.minimum(edge, np.abs(ref - t)), edge)
    return term, edge


def linear_moments(texels, layer, u, v):
    """texels (layers, h, w, 2) -> (..., 2)"""
    _, h, w, _ = texels.shape
    xs, ys, weights = footprint(u, v, w, h)
    out = np.zeros(u.shape + (2,))
    for (ix, iy), wt in zip(((0, 0), (1, 0), (0, 1), (1, 1)), weights):
        out = out + wt[..., None] * texels[layer, ys[iy], xs[ix]]
    return out


def pcf_kernel(p):
    p2 = p * p
    return np.exp2(-0.375 * p2) * (1.0 - p2 / 9.0)


def pcf_wide(texels, layer, u, v, ref):
    """SAMPLE_PCF_GATHER with SHADOW_MAP_PCF_KERNEL_WIDE -> (term, knife edge)"""
    _, h, w = texels.shape
    ix, iy = u * w - 1.5, v * h - 1.5
    fx, fy = np.floor(ix), np.floor(iy)
    cx, cy = ix - fx, iy - fy
    # the gathers' footprint: floor((floored / size) * size - 0.5) = floored - 1
    x_first, y_first = fx.astype(np.int64) - 1, fy.astype(np.int64) - 1
    offsets = (2.0, 1.0, 0.0, -1.0, -2.0, -3.0)
    hw = [pcf_kernel(cx + o) for o in offsets]
    vw = [pcf_kernel(cy + o) for o in offsets]
    var, total, edge = np.zeros_like(ref), np.zeros_like(ref), np.full(ref.shape, np.inf)
    for j in range(6):
        y = np.clip(y_first + j, 0, h - 1)
        for i in range(6):
            t = texels[layer, y, np.clip(x_first + i, 0, w - 1)]
            k = hw[i] * vw[j]
            var = var + k * (ref >= t)
            total = total + k
            edge = np.where(k != 0.0, np.minimum(edge, np.abs(ref - t)), edge)
    return var / total, edge


def vsm(depth, moments):
    mx, my = moments[..., 0], moments[..., 1]
    variance = np.maximum(my - mx * mx, const32(0.00001))
    d = depth - mx
    term = variance / (variance + d * d)
    term = np.clip((term - 0.25) / 0.75, 0.0, 1.0)
    return np.where(depth > mx, term, 1.0)


def layer_term(mode, texels, layer, clip):
    """-> (term, knife edge) of one lookup per pixel at light-space positions clip (..., 3)"""
    u, v, z = clip[..., 0], clip[..., 1], clip[..., 2]
    if mode == MODE_VSM:
        m = linear_moments(texels, layer, u, v)
        # vsm's own branch, depth > moments.x, is continuous: the term is 1 at d = 0
        return vsm(z, m), np.full(z.shape, np.inf)
    if mode == MODE_PCF_WIDE:
        return pcf_wide(texels, layer, u, v, z)
    return linear_shadow(texels, layer, u, v, z)


# ---- cascades ---------------------------------------------------------------------------------------------------------------------------
def compute_shadow_cascade(pos, camera_pos, camera_front, log_bias):
    """-> layer_near, layer_far, shadow_lerp, white_lerp"""
    view_z = np.maximum((f64(camera_front) * (pos - f64(camera_pos))).sum(-1), 0.0)
    with np.errstate(divide="ignore"):
        cascade = np.maximum(np.log2(view_z) + float(log_bias), 0.0)
    near = np.minimum(np.minimum(cascade, float(NUM_CASCADES)).astype(np.int64), NUM_CASCADES - 1)
    far = np.minimum(near + 1, NUM_CASCADES - 1)
    begin = const32(0.8)
    inv_begin = float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.8)))
    lerp = inv_begin * np.maximum((cascade - np.floor(cascade)) - begin, 0.0)
    lerp = np.where(near == far, 0.0, lerp)
    far = np.where(lerp == 0.0, near, far)
    max_cascade = float(NUM_CASCADES)
    white = np.clip((100.0 / max_cascade) * (cascade - float(np.float32(0.99) * np.float32(max_cascade))), 0.0, 1.0)
    return near, far, lerp, white


def light_clip(transform, pos):
    """transform: 16 floats, column-major -> (..., 3)"""
    m = f64(transform).reshape(4, 4).T  # rows
    with np.errstate(invalid="ignore"):  # positions of far-plane pixels are not finite and are not used
        return pos @ m[:3, :3].T + m[:3, 3]


def shadow_term(mode, maps, transforms, cascaded, pos, camera_pos, camera_front, log_bias):
    """get_directional_shadow_term -> (term, knife edge, cascade or None)"""
    texels = f64(maps) if mode == MODE_VSM else depth_values(maps)
    transforms = f64(transforms).reshape(4, 16)
    if not cascaded:
        zero = np.zeros(pos.shape[:-1], np.int64)
        term, edge = layer_term(mode, texels, zero, light_clip(transforms[0], pos))
        return term, edge, None
    near, far, lerp, white = compute_shadow_cascade(pos, camera_pos, camera_front, log_bias)
    clips = np.stack([light_clip(transforms[i], pos) for i in range(NUM_CASCADES)])
    pick = lambda layer: np.take_along_axis(clips, layer[None, ..., None], 0)[0]
    term, edge = layer_term(mode, texels, near, pick(near))
    term_far, edge_far = layer_term(mode, texels, far, pick(far))
    blended = lerp > 0.0
    term = np.where(blended, term * (1.0 - lerp) + term_far * lerp, term)
    edge = np.where(blended, np.minimum(edge, edge_far), edge)
    term = term * (1.0 - white) + white
    edge = np.where(white >= 1.0, np.inf, edge)  # the lookups no longer reach the result
    return term, edge, (near, far, lerp, white)


# ---- the fragment -------------------------------------------------------------------------------------------------------------------------
def world_position(inv_vp, width, height, depth):
    """depth (h, w) -> (h, w, 3); inv_vp 16 floats, column-major"""
    m = f64(inv_vp).reshape(4, 4).T
    x = 2.0 * ((np.arange(width) + 0.5) * const32(1.0 / width)) - 1.0
    y = 2.0 * ((np.arange(height) + 0.5) * const32(1.0 / height)) - 1.0
    ndc = np.stack([np.broadcast_to(x[None, :], depth.shape), np.broadcast_to(y[:, None], depth.shape), f64(depth), np.ones(depth.shape)], -1)
    clip = ndc @ m.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return clip[..., :3] / clip[..., 3:4]


def normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def compute_lighting(base, normal, metallic, roughness_in, term, pos, camera_pos, direction, color):
    roughness = roughness_in * 0.75 + 0.25
    L = f64(direction)
    V = normalize(f64(camera_pos) - pos)
    H = normalize(V + L)
    dot = lambda a, b: (a * b).sum(-1)
    NoV, NoL, HoV = np.clip(dot(normal, V), const32(0.001), 1.0), np.clip(dot(normal, L), const32(0.001), 1.0), np.clip(dot(H, V), const32(0.001), 1.0)
    metal = metallic[..., None]
    F0 = const32(0.04) * (1.0 - metal) + base * metal
    f = ((1.0 - HoV) ** 5.0)[..., None]
    fresnel = F0 * (1.0 - f) + f
    NoH = np.clip(dot(normal, H), const32(0.0001), 1.0)
    m2 = (roughness * roughness) ** 2
    d = (NoH * m2 - NoH) * NoH + 1.0
    D = m2 / (PI_SIC * d * d)
    k = (roughness + 1.0) ** 2 * 0.125
    G = 0.25 / np.maximum((NoV * (1.0 - k) + k) * (NoL * (1.0 - k) + k), const32(0.001))
    lit = f64(color) * (NoL * term)[..., None]
    specref = lit * fresnel * (G * D)[..., None]
    diffref = lit * (1.0 - fresnel) * float(np.float32(1.0) / np.float32(PI_SIC))
    return specref + diffref * base * (1.0 - metal)


def decode_gbuffer(albedo, normal, pbr, srgb_table):
    """albedo (h, w) uint32 R8G8B8A8_SRGB, normal (h, w) uint32 A2B10G10R10, pbr (h, w) uint16 R8G8 -> base, N, metallic, roughness"""
    table = f64(srgb_table)
    albedo, normal, pbr = np.asarray(albedo, np.uint32), np.asarray(normal, np.uint32), np.asarray(pbr, np.uint16)
    base = np.stack([table[(albedo >> s) & 255] for s in (0, 8, 16)], -1)
    n = np.stack([((normal >> s) & 1023).astype(np.float64) / 1023.0 * 2.0 - 1.0 for s in (0, 10, 20)], -1)
    return base, n, (pbr & 255).astype(np.float64) / 255.0, (pbr >> 8).astype(np.float64) / 255.0


def sample_r8(image, u, v):
    """an R8_UNORM image through LinearClamp"""
    h, w = image.shape
    xs, ys, weights = footprint(u, v, w, h)
    texels = image.astype(np.float64) / 255.0
    out = np.zeros(u.shape)
    for (ix, iy), wt in zip(((0, 0), (1, 0), (0, 1), (1, 1)), weights):
        out = out + wt * texels[ys[iy], xs[ix]]
    return out


def directional_light(case, srgb_table):
    """The frame of one case (tests/shadow_cases.py) -> dict: colour (h, w, 3) the fragment's output before the blend, hdr (h, w, 3) emissive +
    colour, term, edge, lit / dark: hdr with the term forced to 1 / 0 (what a pixel on a knife edge must lie between), cascade."""
    h, w = case["depth"].shape
    base, normal, metallic, roughness = decode_gbuffer(case["albedo"], case["normal"], case["pbr"], srgb_table)
    pos = world_position(case["inv_view_projection"], w, h, case["depth"])
    far = case["depth"] == 0.0
    pos = np.where(far[..., None], 0.0, pos)
    term, edge, cascade = shadow_term(case["mode"], case["maps"], case["transforms"], case["cascaded"], pos, case["camera_pos"], case["camera_front"],
                                      case["cascade_log_bias"])
    ambient = np.zeros((h, w, 3))
    if case["fallback"]:
        ao = 1.0
        if case.get("ambient_occlusion") is not None:
            u = (np.arange(w) + 0.5) * const32(1.0 / w)
            v = (np.arange(h) + 0.5) * const32(1.0 / h)
            ao = sample_r8(case["ambient_occlusion"], np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w)))[..., None]
        ambient = ao * base * const32(0.05)
    emissive = np.asarray(case["emissive"], np.uint16).view(np.float16).astype(np.float64)[..., :3]
    with np.errstate(invalid="ignore", divide="ignore"):
        shade = lambda t: np.where(far[..., None], 0.0, compute_lighting(base, normal, metallic, roughness, t, pos, case["camera_pos"], case["direction"], case["color"]) + ambient)
        colour = shade(term)
        lit, dark = shade(np.ones_like(term)), shade(np.zeros_like(term))
    return dict(colour=colour, hdr=emissive + colour, lit=emissive + lit, dark=emissive + dark, term=np.where(far, 1.0, term), edge=np.where(far, np.inf, edge),
                cascade=cascade, far=far)


# ---- the VSM chain -------------------------------------------------------------------------------------------------------------------------
def vsm_moments(depth):
    """(h, w) uint16 or float32 -> (h, w, 2): resolve_vsm.frag, whose value is an fp32 texel"""
    z = depth_values(depth[None])[0] if depth.dtype == np.uint16 else depth.astype(np.float64)
    z = np.float32(z).astype(np.float64)  # subpassLoad returns the fp32 value of the texel
    return np.stack([z, z * z], -1)


def vsm_blur(moments, out_w, out_h, up):
    """(layers, h, w, 2) -> (layers, out_h, out_w, 2): vsm_down_blur.frag (up = 0) or vsm_up_blur.frag"""
    layers, h, w, _ = moments.shape
    texels = f64(moments)
    s = 0.875 if up else 1.75
    taps = ((0.25, 0.0, 0.0), (0.0625, -s, s), (0.125, 0.0, s), (0.0625, s, s), (0.125, -s, 0.0), (0.125, s, 0.0), (0.0625, -s, -s), (0.125, 0.0, -s), (0.0625, s, -s))
    u = np.broadcast_to(((np.arange(out_w) + 0.5) / out_w)[None, :], (out_h, out_w))
    v = np.broadcast_to(((np.arange(out_h) + 0.5) / out_h)[:, None], (out_h, out_w))
    inv_x, inv_y = const32(1.0 / w), const32(1.0 / h)
    out = np.zeros((layers, out_h, out_w, 2))
    for layer in range(layers):
        index = np.full((out_h, out_w), layer, np.int64)
        for weight, ox, oy in taps:
            out[layer] += weight * linear_moments(texels, index, u + ox * inv_x, v + oy * inv_y)
    return out
