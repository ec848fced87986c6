"""The ocean's three compute shaders restated in numpy (ocean/generate_fft.comp, bake_maps.comp, mipmap.comp).

generate() is float64 from the point where the shader stops being discontinuous: the wave vector, its length, the square root and the
quantised angular velocity are taken in fp32 exactly as the shader takes them (a last-bit difference there flips round() and moves the
bin's phase by time / period radians); the rotation, the sum with the mirrored bin, the gradient factor and the band amplitude follow in
float64.  bake_maps() and mipmap() take a dtype: float64 is the formula, float32 repeats the shader's fp32 operations one by one and gives
its bytes.

LinearWrap model, as granite_amd/csrc/ocean_core.hpp states it: linear_axis(u * size - 0.5) per axis (exact weights, 2^-8 snap onto
texel centres), the two lerps of linear_combine, texel indices and offsets modulo the size (Euclidean)."""
import numpy as np

HEIGHT, GRADIENT_NORMAL, GRADIENT_DISPLACEMENT = 0, 1, 2
NUM_FREQ_BANDS = 8
LAMBDA = np.float32(1.2)
SNAP = 1.0 / 256.0
HALF_MIN_NORMAL = 2.0 ** -14
# tests/golden/make_ocean_golden.py prints, per case, how far the executed fp32 shader lies from generate() in units of one fp16 ulp of
# (|a| + |b|) g band; the largest over all cases was 0.772.  The bound of every generate test: that maximum plus one
# unit for a second fp16 rounding boundary.
GENERATE_MEASURED_UNITS = 0.772
GENERATE_BOUND_UNITS = GENERATE_MEASURED_UNITS + 1.0


def half_to_float(bits, dtype=np.float64):
    return np.ascontiguousarray(bits).view(np.float16).astype(dtype)


def float_to_half(values):
    """round to nearest even, overflow to infinity: the bits of an fp16 store"""
    with np.errstate(over="ignore"):
        return np.asarray(values).astype(np.float16).view(np.uint16)


# ---- push blocks, as bytes ---------------------------------------------------------------------------------------------------------
def generate_push(mod_factor, n, freq_to_band_mod, time, period):
    """gr_push_ocean_generate as 7 dwords: mod_factor[2], N[2] = (N.x, N.y), freq_to_band_mod, time, period"""
    p = np.zeros(7, np.uint32)
    p[0:2] = np.array(mod_factor, np.float32).view(np.uint32)
    p[2:4] = n
    p[4:7] = np.array([freq_to_band_mod, time, period], np.float32).view(np.uint32)
    return p


def bake_push(inv_size, scale):
    return np.array(list(inv_size) + list(scale), np.float32)


def mipmap_push(result_mod, inv_resolution, count, lod=0.0):
    p = np.zeros(9, np.uint32)
    p[0:4] = np.array(result_mod, np.float32).view(np.uint32)
    p[4:6] = np.array(inv_resolution, np.float32).view(np.uint32)
    p[6:8] = count
    p[8:9] = np.array([lod], np.float32).view(np.uint32)
    return p


# ---- generate_fft.comp ---------------------------------------------------------------------------------------------------------------
def alias(n):
    i = np.arange(n, dtype=np.float64)
    return np.where(i > 0.5 * n, i - n, i)


def generate(distribution, push, variant, bands=None):
    """distribution (N.y, N.x, 2) float32 -> (spectrum complex128 (N.y, N.x), s float64): the value the shader packs, before the fp16
    rounding, and the size of its terms before they cancel, (|a| + |b|) g band."""
    f32 = np.float32
    pf = push.view(np.float32)
    nx, ny = int(push[2]), int(push[3])
    d = np.asarray(distribution, np.float32).reshape(ny, nx, 2)
    a = d[..., 0].astype(np.float64) + 1j * d[..., 1].astype(np.float64)
    wy, wx = (ny - np.arange(ny)) & (ny - 1), (nx - np.arange(nx)) & (nx - 1)
    b = a[wy][:, wx]
    fx, fy = np.meshgrid(alias(nx), alias(ny))
    # fp32, operation by operation: k, x * x + y * y, sqrt, G * k_len, sqrt, * period, round (half away from zero), / period
    kx, ky = f32(pf[0]) * fx.astype(f32), f32(pf[1]) * fy.astype(f32)
    k_len = np.sqrt(kx * kx + ky * ky)
    scaled = np.sqrt(f32(9.81) * k_len) * f32(pf[6])
    angular_velocity = np.floor(scaled.astype(np.float64) + 0.5).astype(f32) / f32(pf[6])
    assert k_len.dtype == f32 and scaled.dtype == f32 and angular_velocity.dtype == f32
    # float64 from here
    w = angular_velocity.astype(np.float64) * float(pf[5])
    rot = np.cos(w) + 1j * np.sin(w)
    res = a * rot + np.conj(b * rot)
    kx, ky, k_len = kx.astype(np.float64), ky.astype(np.float64), k_len.astype(np.float64)
    g = np.ones_like(k_len)
    if variant == GRADIENT_NORMAL:
        res = res * (-ky + 1j * kx)
        g = k_len
    elif variant == GRADIENT_DISPLACEMENT:
        denominator = k_len + float(f32(0.00001))
        res = res * (-ky / denominator + 1j * kx / denominator)
        g = k_len / denominator
    amplitude = np.ones_like(k_len)
    if bands is not None:
        bands = np.asarray(bands, np.float32).astype(np.float64)
        band = np.clip(np.maximum(fx, fy) * float(pf[4]), 0.0, float(f32(NUM_FREQ_BANDS) - f32(1.001)))
        low = band.astype(np.int64)
        t = band - np.floor(band)
        amplitude = bands[low] * (1.0 - t) + bands[low + 1] * t
        res = res * amplitude
    return res, (np.abs(a) + np.abs(b)) * g * np.abs(amplitude)


def half_ulp_of(s):
    """one fp16 ulp at magnitude s, with the floor of the smallest fp16 normal"""
    s = np.maximum(np.asarray(s, np.float64), HALF_MIN_NORMAL)
    return 2.0 ** (np.floor(np.log2(s)) - 10.0)


def generate_distance(out_bits, spectrum, s):
    """largest distance of packed half2 words (N.y, N.x) uint32 from `spectrum`, in fp16 ulps of s"""
    out_bits = np.asarray(out_bits, np.uint32).reshape(spectrum.shape)
    re = half_to_float((out_bits & 0xffff).astype(np.uint16))
    im = half_to_float((out_bits >> 16).astype(np.uint16))
    return float((np.maximum(np.abs(re - spectrum.real), np.abs(im - spectrum.imag)) / half_ulp_of(s)).max())


# ---- LinearWrap ----------------------------------------------------------------------------------------------------------------------
def linear_axis(f, dtype):
    fl = np.floor(f + dtype(SNAP))
    a = f - fl
    a = np.where(a < dtype(SNAP), dtype(0.0), a)
    return fl.astype(np.int64), a.astype(dtype)


def sample(image, u, v, offset=(0, 0), dtype=np.float32, wrap=True):
    """image (h, w, C) of dtype; u, v arrays of dtype -> (..., C).  wrap=False clamps instead (only to show that a case tests the wrap)."""
    h, w = image.shape[:2]
    x0, a = linear_axis(u * dtype(w) - dtype(0.5), dtype)
    y0, b = linear_axis(v * dtype(h) - dtype(0.5), dtype)
    x0, y0 = x0 + offset[0], y0 + offset[1]
    if wrap:
        fetch = lambda x, y: image[np.mod(y, h), np.mod(x, w)]
    else:
        fetch = lambda x, y: image[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
    a, b = a[..., None], b[..., None]
    one = dtype(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        top = np.where(a == 0, fetch(x0, y0), fetch(x0, y0) * (one - a) + fetch(x0 + 1, y0) * a)
        bottom = np.where(a == 0, fetch(x0, y0 + 1), fetch(x0, y0 + 1) * (one - a) + fetch(x0 + 1, y0 + 1) * a)
        return np.where(b == 0, top, top * (one - b) + bottom * b).astype(dtype)


# ---- bake_maps.comp ------------------------------------------------------------------------------------------------------------------
def bake_maps(height_bits, displacement_bits, push, dtype=np.float32, wrap=True):
    """height (h, w) and displacement (dh, dw, 2) as fp16 bits, push = bake_push(...) -> (grad_jacobian, height_displacement) bits
    (h, w, 4).  Both coordinate pairs advance by inv_size.xy; the displacement pair starts at half a displacement texel."""
    push = np.asarray(push, np.float32).astype(dtype)
    inv, scale = push[0:4], push[4:8]
    height = half_to_float(height_bits, dtype)[..., None]
    displacement = half_to_float(displacement_bits, dtype)
    h, w = height.shape[:2]
    gx, gy = np.meshgrid(np.arange(w).astype(dtype), np.arange(h).astype(dtype))
    half, lam = dtype(0.5), dtype(LAMBDA)
    px, py = gx * inv[0], gy * inv[1]
    u, v = px + half * inv[0], py + half * inv[1]
    du, dv = px + half * inv[2], py + half * inv[3]
    tap = lambda o: sample(height, u, v, o, dtype, wrap)[..., 0]
    hgt, x0, x1, y0, y1 = tap((0, 0)), tap((-1, 0)), tap((1, 0)), tap((0, -1)), tap((0, 1))
    grad_x, grad_y = (scale[0] * half) * (x1 - x0), (scale[1] * half) * (y1 - y0)
    dtap = lambda o: sample(displacement, du, dv, o, dtype, wrap)
    d = lam * dtap((0, 0))
    ddx = ((half * lam) * (dtap((1, 0)) - dtap((-1, 0)))) * scale[2]
    ddy = ((half * lam) * (dtap((0, 1)) - dtap((0, -1)))) * scale[3]
    one = dtype(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        j = (one + ddx[..., 0]) * (one + ddy[..., 1]) - ddx[..., 1] * ddy[..., 0]
    zero = np.zeros_like(hgt)
    return float_to_half(np.stack([grad_x, grad_y, j, zero], -1)), float_to_half(np.stack([hgt, d[..., 0], d[..., 1], zero], -1))


# ---- mipmap.comp ---------------------------------------------------------------------------------------------------------------------
def mipmap(in_bits, push, dtype=np.float32, wrap=True):
    """in (h, w, C) fp16 bits, push = mipmap_push(...) -> (count.y, count.x, C) fp16 bits"""
    in_bits = np.asarray(in_bits)
    if in_bits.ndim == 2:
        in_bits = in_bits[..., None]
    channels = in_bits.shape[2]
    pf = push.view(np.float32).astype(dtype)
    cx, cy = int(push[6]), int(push[7])
    gx, gy = np.meshgrid(np.arange(cx).astype(dtype), np.arange(cy).astype(dtype))
    u, v = (dtype(2.0) * gx + dtype(1.0)) * pf[4], (dtype(2.0) * gy + dtype(1.0)) * pf[5]
    with np.errstate(invalid="ignore", over="ignore"):
        return float_to_half(pf[0:channels] * sample(half_to_float(in_bits, dtype), u, v, (0, 0), dtype, wrap))


def mip_chain(level0_bits, levels, last_result_mod=(1.0, 1.0, 1.0, 1.0)):
    """generate_mipmaps level by level: level i from level i - 1 as stored, result_mod on the last level only"""
    chain = [np.asarray(level0_bits)]
    for i in range(1, levels):
        src = chain[-1]
        h, w = src.shape[:2]
        mod = last_result_mod if i + 1 == levels else (1.0, 1.0, 1.0, 1.0)
        push = mipmap_push(mod, (np.float32(1.0) / np.float32(w), np.float32(1.0) / np.float32(h)), (max(w >> 1, 1), max(h >> 1, 1)), float(i - 1))
        chain.append(mipmap(src, push).reshape((max(h >> 1, 1), max(w >> 1, 1)) + src.shape[2:]))
    return chain
