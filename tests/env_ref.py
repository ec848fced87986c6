"""Environment baking in float64 numpy, restated from the formulae: the lat-long lookup of skybox_latlon.frag, the linear blit of
generate_mipmap, the GGX prefilter of util/ibl_specular.frag (Hammersley points, the shader's PI and up-vector switch), the hemisphere
sum of util/ibl_diffuse.frag (the two loop counters stepped in fp32 as the shader steps them, everything else float64), and the
project's cube sampling model: Vulkan's face table with ties Z over Y over X, bilinear taps with the linear_axis snap,
footprint texels off a face resolved through the direction of their centre, trilinear by linear_axis(lod).

A cube chain is a list of float64 arrays [6, n, n, 4], one per level; on disk and on the device it is the GTX payload layout
(levels in order, six faces a level, rows tightly packed), fp16.  Every level is rounded to fp16 where the device stores it."""
import numpy as np

SNAP = 1.0 / 256.0
SHADER_PI = 3.1415628
SAMPLES = 1024
DELTA = np.float32(0.025)

# Vulkan's cube face table as bases: a direction on face f is MAJOR[f] + sc * U_AXIS[f] + tc * V_AXIS[f]
MAJOR = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
U_AXIS = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
V_AXIS = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.float64)


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def level_size(size, level):
    return max(size >> level, 1)


def full_chain_levels(size):
    return int(size).bit_length()


def chain_texels(size, levels):
    return sum(6 * level_size(size, l) ** 2 for l in range(levels))


def chain_offset(size, level, face):
    """Byte offset of a face of a level: 8 bytes a texel; a level is 48 n^2 bytes, so every level starts 16-byte aligned."""
    n = level_size(size, level)
    return 8 * (chain_texels(size, level) + face * n * n)


def unpack_chain(bits, size, levels):
    bits = np.asarray(bits, np.uint16).reshape(-1)
    out, at = [], 0
    for l in range(levels):
        n = level_size(size, l)
        out.append(bits[at:at + 6 * n * n * 4].view(np.float16).astype(np.float64).reshape(6, n, n, 4))
        at += 6 * n * n * 4
    return out


def to_half(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16)


def pack_chain(levels):
    return np.concatenate([to_half(a).reshape(-1) for a in levels]).view(np.uint16)


def round_half(a):
    return to_half(a).astype(np.float64)


# ---- sampler --------------------------------------------------------------------------------------------------------------------------
def linear_axis(f):
    fl = np.floor(f + SNAP)
    a = f - fl
    return fl.astype(np.int64), np.where(a < SNAP, 0.0, a)


def select_face(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    is_z = (az >= ax) & (az >= ay)
    is_y = ~is_z & (ay >= ax)
    face = np.where(is_z, np.where(z < 0, 5, 4), np.where(is_y, np.where(y < 0, 3, 2), np.where(x < 0, 1, 0)))
    ma = np.where(is_z, az, np.where(is_y, ay, ax))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 0.5 * np.einsum("...i,...i->...", d, U_AXIS[face]) / ma + 0.5
        t = 0.5 * np.einsum("...i,...i->...", d, V_AXIS[face]) / ma + 0.5
    return face, s, t


def face_direction(face, sc, tc):
    return MAJOR[face] + U_AXIS[face] * sc[..., None] + V_AXIS[face] * tc[..., None]


def texel_directions(matrices, n):
    """[6, n, n, 3]: (inverse(proj * look) * (ndc, 1, 1)).xyz at the pixel centres, as skybox.vert gives it; not normalised."""
    m = np.asarray(matrices, np.float64).reshape(6, 4, 4)  # [face, column, row]
    p = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    px, py = p[None, None, :, None], p[None, :, None, None]
    return (m[:, 0, :3][:, None, None, :] * px + m[:, 1, :3][:, None, None, :] * py + (m[:, 2, :3] + m[:, 3, :3])[:, None, None, :])


def footprint(level, face, x, y):
    n = level.shape[1]
    inside = (x >= 0) & (y >= 0) & (x < n) & (y < n)
    d = face_direction(face, (2 * x + 1 - n) / n, (2 * y + 1 - n) / n)  # integer numerators: a corner stays an exact tie
    other, s, t = select_face(d)
    ox, oy = np.clip(np.floor(s * n), 0, n - 1).astype(np.int64), np.clip(np.floor(t * n), 0, n - 1).astype(np.int64)
    return level[np.where(inside, face, other), np.where(inside, y, oy), np.where(inside, x, ox), :3]


def sample_level(level, d):
    n = level.shape[1]
    face, s, t = select_face(d)
    ix, a = linear_axis(s * n - 0.5)
    iy, b = linear_axis(t * n - 0.5)
    out = footprint(level, face, ix, iy) * ((1 - a) * (1 - b))[..., None]
    out += footprint(level, face, ix + 1, iy) * (a * (1 - b))[..., None]
    out += footprint(level, face, ix, iy + 1) * ((1 - a) * b)[..., None]
    out += footprint(level, face, ix + 1, iy + 1) * (a * b)[..., None]
    return out


def sample_trilinear(chain, d, lod):
    lod = min(max(float(lod), 0.0), len(chain) - 1.0)
    l0, w = linear_axis(np.float64(lod))
    l0, w = int(l0), float(w)
    out = sample_level(chain[l0], d)
    if w != 0.0 and l0 + 1 < len(chain):
        out = out * (1.0 - w) + sample_level(chain[l0 + 1], d) * w
    return out


def nearest_level(lod, levels):
    lod = min(max(float(lod), 0.0), levels - 1.0)
    return int(min(max(np.ceil(lod + 0.5) - 1, 0), levels - 1))


def normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


# ---- equirect -> cube -------------------------------------------------------------------------------------------------------------------
def latlon(equirect, d):
    """skybox_latlon.frag: LinearWrap tap of an [h, w, 4] image along directions d."""
    h, w = equirect.shape[:2]
    v = normalize(d)
    vx = np.where(np.abs(v[..., 0]) < 0.00001, 0.00001, v[..., 0])
    u = np.arctan2(v[..., 2], vx) * 0.1591 + 0.5
    t = np.arcsin(-v[..., 1]) * 0.3183 + 0.5
    ix, a = linear_axis(u * w - 0.5)
    iy, b = linear_axis(t * h - 0.5)
    tap = lambda x, y: equirect[y % h, x % w, :3]
    return (tap(ix, iy) * ((1 - a) * (1 - b))[..., None] + tap(ix + 1, iy) * (a * (1 - b))[..., None] +
            tap(ix, iy + 1) * ((1 - a) * b)[..., None] + tap(ix + 1, iy + 1) * (a * b)[..., None])


def blit_level(src, n):
    """generate_mipmap: [6, m, m, 4] -> [6, n, n, 4], a linear-filter blit per face, clamped to the face, rounded to fp16."""
    m = src.shape[1]
    i, a = linear_axis((np.arange(n) + 0.5) * (m / n) - 0.5)
    i0, i1 = np.clip(i, 0, m - 1), np.clip(i + 1, 0, m - 1)
    rows = src[:, i0] * (1 - a)[None, :, None, None] + src[:, i1] * a[None, :, None, None]
    return round_half(rows[:, :, i0] * (1 - a)[None, None, :, None] + rows[:, :, i1] * a[None, None, :, None])


def equirect_to_cube(matrices, equirect_bits, size, levels):
    equirect = np.asarray(equirect_bits, np.uint16).view(np.float16).astype(np.float64)
    level0 = np.ones((6, size, size, 4))
    level0[..., :3] = latlon(equirect, texel_directions(matrices, size))
    chain = [round_half(level0)]
    for l in range(1, levels):
        chain.append(blit_level(chain[-1], level_size(size, l)))
    return chain


# ---- ibl_specular.frag ------------------------------------------------------------------------------------------------------------------
def hammersley():
    i = np.arange(SAMPLES, dtype=np.uint64)
    rev = np.zeros(SAMPLES, np.uint64)
    for bit in range(32):
        rev |= ((i >> np.uint64(bit)) & np.uint64(1)) << np.uint64(31 - bit)
    return i.astype(np.float64) / SAMPLES, rev.astype(np.float64) * 2.3283064365386963e-10


def roughness_of(level, levels):
    t = level / (levels - 1) if levels > 1 else 0.0
    return 0.001 * (1.0 - t) + t


def specular_level(matrices, chain, n, lod, roughness):
    xi_x, xi_y = hammersley()
    a = roughness * roughness
    phi = 2.0 * SHADER_PI * xi_x
    cos_theta = np.sqrt((1.0 - xi_y) / (1.0 + (a * a - 1.0) * xi_y))
    sin_theta = np.sqrt(1.0 - cos_theta * cos_theta)
    h_t = np.stack([np.cos(phi) * sin_theta, np.sin(phi) * sin_theta, cos_theta], -1)  # [1024, 3]
    nrm = normalize(texel_directions(matrices, n)).reshape(-1, 3)
    up = np.where((np.abs(nrm[:, 2]) < 0.999)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    tangent = normalize(np.cross(up, nrm))
    bitangent = np.cross(nrm, tangent)
    h = normalize(tangent[:, None] * h_t[None, :, 0:1] + bitangent[:, None] * h_t[None, :, 1:2] + nrm[:, None] * h_t[None, :, 2:3])
    v = nrm[:, None]
    l = normalize(2.0 * (v * h).sum(-1, keepdims=True) * h - v)
    ndotl = np.maximum((v * l).sum(-1), 0.0)
    colour = sample_trilinear(chain, l, lod) * ndotl[..., None]
    out = np.ones((nrm.shape[0], 4))
    out[:, :3] = colour.sum(1) / ndotl.sum(1)[:, None]
    return out.reshape(6, n, n, 4)


def specular(matrices, chain, out_size, out_levels):
    base = np.log2(chain[0].shape[1]) - np.log2(out_size)
    return [round_half(specular_level(matrices, chain, level_size(out_size, l), base + l, roughness_of(l, out_levels))) for l in range(out_levels)]


def check_up_switch(matrices, out_size, out_levels):
    """No tested texel direction may sit on the 0.999 up-vector switch, where fp32 and float64 could take different frames."""
    for l in range(out_levels):
        nz = np.abs(normalize(texel_directions(matrices, level_size(out_size, l)))[..., 2])
        assert (np.abs(nz - 0.999) > 1e-5).all(), (out_size, l)


# ---- ibl_diffuse.frag -------------------------------------------------------------------------------------------------------------------
def loop_values(limit):
    """for (float a = 0.0; a < limit; a += 0.025): the values a takes, stepped in fp32."""
    out, a, limit = [], np.float32(0.0), np.float32(limit)
    while a < limit:
        out.append(a)
        a = np.float32(a + DELTA)
    return np.array(out, np.float64)


def diffuse_angles():
    phi = loop_values(np.float32(2.0) * np.float32(SHADER_PI))
    theta = loop_values(np.float32(0.5) * np.float32(SHADER_PI))
    assert (phi.size, theta.size) == (252, 63) and phi.size * theta.size == 15876
    return phi, theta


def diffuse(matrices, chain, out_size):
    lod = max(np.log2(out_size) - 5.0, 0.0)
    level = chain[nearest_level(lod, len(chain))]
    phi, theta = diffuse_angles()
    sp, cp = np.repeat(np.sin(phi), theta.size), np.repeat(np.cos(phi), theta.size)
    st, ct = np.tile(np.sin(theta), phi.size), np.tile(np.cos(theta), phi.size)
    out = np.ones((6, out_size, out_size, 4))
    dirs = normalize(texel_directions(matrices, out_size))
    for face in range(6):
        for y in range(out_size):
            d = dirs[face, y]  # [n, 3]
            right = np.cross(np.array([0.0, 1.0, 0.0]), d)
            up = np.cross(d, right)
            sample = right[:, None] * (st * cp)[None, :, None] + up[:, None] * (st * sp)[None, :, None] + d[:, None] * ct[None, :, None]
            total = (sample_level(level, sample) * (ct * st)[None, :, None]).sum(1)
            out[face, y, :, :3] = SHADER_PI * total * (1.0 / (phi.size * theta.size))
    return round_half(out)


# ---- comparison -------------------------------------------------------------------------------------------------------------------------
def ulp_distance(a_bits, b_bits):
    """Per channel: |a - b| in fp16 ulps at the larger magnitude, after the standing absolute allowance of 1e-4 is taken off."""
    a = np.asarray(a_bits, np.uint16).view(np.float16).astype(np.float64)
    b = np.asarray(b_bits, np.uint16).view(np.float16).astype(np.float64)
    mag = np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -14)
    return np.maximum(np.abs(a - b) - 1e-4, 0.0) / np.exp2(np.floor(np.log2(mag)) - 10.0)


def report(name, got_bits, ref_bits):
    d = ulp_distance(got_bits, ref_bits).reshape(-1, 4)
    print(f"{name:12s} executed shaders (fp32) against env_ref (float64): max {d.max():.3f} fp16 ulps beyond abs 1e-4; "
          f"{int((d > 2.0).any(axis=1).sum())} of {d.shape[0]} texels beyond 2 ulps, {int((d > 1.0).any(axis=1).sum())} beyond 1")
    return d
