"""numpy float32 restatement of the sky pass: lights/atmospheric_scatter.h, skybox.frag without HAVE_EMISSIVE and
lights/volumetric_light_setup_sky.comp, single operations in the shader's order (every array is float32, every constant a float32, so
each numpy operation is one IEEE fp32 operation).  The decisions (quadratic < 0; t_diff > 0 and no earth hit) are made of + - * sqrt and
come out as the executed shader's; values differ from it through exp and pow alone.  float64 is no yardstick here: the cancellation in
length(sample_pos) - E_radius makes the shader's own fp32 result differ from a float64 one by up to 1.7e-3 relative.

The textured variant (the cube lookup) has no numpy restatement: the host build of csrc/sky_core.hpp is held to the golden bit for bit
(tests/test_sky_core_cpu.py)."""
import numpy as np

F = np.float32
B_RAYLEIGH = np.array([5.5e-6, 13.0e-6, 22.4e-6], F)
B_MIE = F(21.0e-6)
B_ABSORPTION = np.array([2.04e-5, 4.97e-5, 1.95e-6], F)
G = F(0.7)
G2 = G * G
H_RAYLEIGH, H_MIE, H_ABSORPTION, ABSORPTION_FALLOFF = F(8000.0), F(1200.0), F(30000.0), F(4000.0)
E_RADIUS, H_ATMOSPHERE = F(6.371e6), F(100000.0)


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def length(a):
    return np.sqrt(dot(a, a))


def trace_to_sphere(pos, direction, radius):
    b = F(2.0) * dot(pos, direction)
    c = dot(pos, pos) - radius * radius
    quadratic = b * b - F(4.0) * c
    miss = quadratic < F(0.0)
    with np.errstate(invalid="ignore"):
        q = np.sqrt(np.where(miss, F(0.0), quadratic))
    t0 = np.where(miss, F(0.0), (-b - q) * F(0.5))
    t1 = np.where(miss, F(0.0), (-b + q) * F(0.5))
    return t0.astype(F), t1.astype(F)


def sample_optical_depth(h, step_length):
    depth_r = np.exp(-h / H_RAYLEIGH) * step_length
    depth_m = np.exp(-h / H_MIE) * step_length
    denom = (H_ABSORPTION - h) / ABSORPTION_FALLOFF
    depth_a = (F(1.0) / (denom * denom + F(1.0))) * depth_r
    depth = depth_r[..., None] * B_RAYLEIGH + (depth_m * B_MIE)[..., None] + depth_a[..., None] * B_ABSORPTION
    return depth, depth_r, depth_m


def height(sample_pos):
    return np.maximum(length(sample_pos) - E_RADIUS, F(0.0))


def accumulate_optical_depth(pos, direction, t, light_steps):
    acc = np.zeros(pos.shape, F)
    step_length = t / F(light_steps)
    for i in range(light_steps):
        t_dir = (F(i) + F(0.5)) * step_length
        sample_pos = pos + t_dir[..., None] * direction
        acc = acc + sample_optical_depth(height(sample_pos), step_length)[0]
    return acc


def scatter_mask(v, camera_height):
    """(marched, t_start, t_diff, pos) of normalised directions v (n, 3)."""
    camera_height = np.maximum(F(camera_height), F(0.0))
    pos = np.zeros(v.shape, F)
    pos[..., 1] = E_RADIUS + camera_height
    a0, a1 = trace_to_sphere(pos, v, E_RADIUS + H_ATMOSPHERE)
    a0 = np.maximum(a0, F(0.0))
    e0, e1 = trace_to_sphere(pos, v, F(0.98) * E_RADIUS)
    intersects_earth = (e0 > F(0.0)) | (e1 > F(0.0))
    t_diff = np.maximum(a1 - a0, F(0.0))
    return (t_diff > F(0.0)) & ~intersects_earth, a0, t_diff, pos


def rayleigh_mie_scatter(v, l, camera_height, primary_steps, light_steps):
    """v (n, 3) float32 normalised, l (3,) -> (n, 3) float32."""
    v = np.ascontiguousarray(v, F)
    l = np.asarray(l, F)
    marched, t_start, t_diff, pos = scatter_mask(v, camera_height)
    out = np.zeros(v.shape, F)
    if not marched.any():
        return out
    v, t_start, t_diff, pos = v[marched], t_start[marched], t_diff[marched], pos[marched]
    acc = np.zeros(v.shape, F)
    in_r = np.zeros(v.shape, F)
    in_m = np.zeros(v.shape, F)
    step_length = t_diff / F(primary_steps)
    lv = np.broadcast_to(l, v.shape)
    for i in range(primary_steps):
        t_view = (F(i) + F(0.5)) * step_length + t_start
        sample_pos = pos + t_view[..., None] * v
        sample, depth_r, depth_m = sample_optical_depth(height(sample_pos), step_length)
        t_sun = trace_to_sphere(sample_pos, lv, E_RADIUS + H_ATMOSPHERE)[1]
        total = acc + F(0.5) * sample + accumulate_optical_depth(sample_pos, lv, t_sun, light_steps)
        transmittance = np.exp(-total)
        acc = acc + sample
        in_r = in_r + depth_r[..., None] * transmittance
        in_m = in_m + depth_m[..., None] * transmittance
    cos_theta = dot(v, lv)
    mumu = cos_theta * cos_theta
    phase_r = F(3.0) / F(50.2654824574) * (F(1.0) + mumu)
    phase_m = F(3.0) / F(25.1327412287) * ((F(1.0) - G2) * (mumu + F(1.0))) / (np.power(F(1.0) + G2 - F(2.0) * cos_theta * G, F(1.5)) * (F(2.0) + G2))
    in_r = in_r * (phase_r[..., None] * B_RAYLEIGH)
    in_m = in_m * (phase_m * B_MIE)[..., None]
    out[marched] = in_r + in_m
    assert out.dtype == F
    return out


def normalize(d):
    return d / length(d)[..., None]


def pixel_directions(inv, width, height_):
    """(height, width, 3): ((c0 * px + c1 * py) + c2) + c3 at the pixel centres, Position = 2 (pixel + 0.5) / size - 1."""
    inv = np.asarray(inv, F).reshape(4, 4)  # inv[c] is column c
    px = (F(2.0) * (np.arange(width, dtype=F) + F(0.5)) / F(width) - F(1.0))[None, :, None]
    py = (F(2.0) * (np.arange(height_, dtype=F) + F(0.5)) / F(height_) - F(1.0))[:, None, None]
    return (inv[0, :3] * px + inv[1, :3] * py + inv[2, :3] + inv[3, :3]).astype(F)


def apply_procedural(depth, inv, color, camera_height, sun_direction):
    """(height, width, 3) float32: color * scatter where depth == 0, 0 elsewhere."""
    h, w = depth.shape
    far = depth == F(0.0)
    out = np.zeros((h, w, 3), F)
    d = pixel_directions(inv, w, h)[far]
    if d.size:
        out[far] = np.asarray(color, F) * rayleigh_mie_scatter(normalize(d), sun_direction, camera_height, 16, 8)
    return out


BASE_DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
POS_DU = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], F)
POS_DV = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], F)


def sky_cube(size, sun_color, camera_y, sun_direction):
    """(6, size, size, 4) float32, alpha 1."""
    inv_resolution = F(1.0) / F(size)
    uv = F(2.0) * ((np.arange(size, dtype=F) + F(0.5)) * inv_resolution) - F(1.0)
    u, v = uv[None, None, :, None], uv[None, :, None, None]
    n = BASE_DIRS[:, None, None, :] + POS_DU[:, None, None, :] * u + POS_DV[:, None, None, :] * v
    rgb = np.asarray(sun_color, F) * rayleigh_mie_scatter(normalize(n.reshape(-1, 3).astype(F)), sun_direction, camera_y, 32, 16)
    out = np.ones((6, size, size, 4), F)
    out[..., :3] = rgb.reshape(6, size, size, 3)
    return out


# ---- distances ------------------------------------------------------------------------------------------------------------------------
def to_half_bits(values):
    with np.errstate(over="ignore"):
        return np.asarray(values, F).astype(np.float16).view(np.uint16)


def ulp_distance(a, b):
    """Per channel: |a - b| of two float arrays after rounding to fp16, in fp16 ulps at the larger magnitude, after the standing absolute
    allowance of 1e-4 is taken off (tests/env_ref.py: ulp_distance)."""
    a = to_half_bits(a).view(np.float16).astype(np.float64)
    b = to_half_bits(b).view(np.float16).astype(np.float64)
    mag = np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -14)
    return np.maximum(np.abs(a - b) - 1e-4, 0.0) / np.exp2(np.floor(np.log2(mag)) - 10.0)


def zero_mask(rgb, far):
    return far & (rgb == 0.0).all(axis=-1)
