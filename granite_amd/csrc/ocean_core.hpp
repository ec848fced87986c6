// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The ocean's two compute passes, the per-lane arithmetic: ocean/generate_fft.comp, ocean/bake_maps.comp and ocean/mipmap.comp of the
// FFT update, ocean/update_lod.comp and ocean/cull_blocks.comp of the LOD update.  Shared by the
// gfx950 kernels (ocean.hip) and by a host build the CPU tests hold to the executed shaders (tests/cpp/ocean_core_host.cpp): the
// kernels add the mapping of bins and texels to lanes, nothing else.  Both builds compile this header with -ffp-contract=off and with
// correctly rounded fp32 sqrt and division: generate_bin quantises an angular velocity with round(), and a last-bit difference in
// x * x + y * y, the square root, the product with period or the division flips it, which moves a bin's phase by time / period radians.
//
// LinearWrap sampling model (the reference leaves it to the Vulkan implementation):
//   - per axis linear_axis(u * size - 0.5): exact fp32 weights, a coordinate within 2^-8 of a texel centre reads that texel alone;
//   - the four texels are joined as linear_combine joins them: two lerps along x, t * (1 - a) + t' * a, then one along y; a weight
//     of exactly 0 does not read its texel;
//   - texel indices, textureLodOffset's offset included, are taken modulo the size (Euclidean: -1 is size - 1).
// fp16 conversion, linear_axis and the Euclidean modulo are core_base.hpp's.
#pragma once
#include "core_base.hpp"

namespace gr_ocean
{
using gr_core::float_to_half_pinned;
using gr_core::half_to_float;
using gr_core::linear_axis;
using gr_core::wrapi;

constexpr uint32_t NUM_FREQ_BANDS = 8u;
constexpr float GRAVITY = 9.81f;
constexpr float LAMBDA = 1.2f;
enum Variant : uint32_t { HEIGHT = 0, GRADIENT_NORMAL = 1, GRADIENT_DISPLACEMENT = 2, VARIANT_COUNT = 3 };

struct c2
{
	float x, y;
};
// cmul of generate_fft.comp: (a.x b.x - b.y a.y, a.y b.x + b.y a.x), each product rounded before the sum
GR_HD c2 cmul(c2 a, c2 b) { return {a.x * b.x - b.y * a.y, a.y * b.x + b.y * a.x}; }

struct GenerateArgs
{
	float mod_x, mod_y;
	uint32_t nx, ny;
	float freq_to_band_mod, time, period;
	uint32_t variant;
	uint32_t use_bands;
	float bands[NUM_FREQ_BANDS];
};

// i > N / 2 goes negative (the Nyquist bin itself stays positive)
GR_HD float alias(uint32_t i, uint32_t n)
{
	const float f = float(i);
	return f > 0.5f * float(n) ? f - float(n) : f;
}

GR_HD float band_amplitude(const GenerateArgs &g, float fx, float fy)
{
	const float bx = fx * g.freq_to_band_mod, by = fy * g.freq_to_band_mod;
	float band = bx > by ? bx : by;
	const float top = float(NUM_FREQ_BANDS) - 1.001f;
	band = band > 0.0f ? (band > top ? top : band) : 0.0f; // a NaN lands on 0, so the index below stays inside bands[]
	const int low = int(band);
	const float t = band - floorf(band);
	return g.bands[low] * (1.0f - t) + g.bands[low + 1] * t;
}

// Bin (x, y) of the animated spectrum; `a` is the distribution at the bin, `b` at its mirror ((N - i) & (N - 1)).  sincosf is the
// full-range one: w reaches thousands of radians.
GR_HD uint32_t generate_bin(const GenerateArgs &g, uint32_t x, uint32_t y, c2 a, c2 b)
{
	const float fx = alias(x, g.nx), fy = alias(y, g.ny);
	const float kx = g.mod_x * fx, ky = g.mod_y * fy;
	const float k_len = sqrtf(kx * kx + ky * ky);
	float angular_velocity = sqrtf(GRAVITY * k_len);
	angular_velocity = roundf(angular_velocity * g.period) / g.period;
	const float w = angular_velocity * g.time;
	float sw, cw;
	sincosf(w, &sw, &cw);
	const c2 rot = {cw, sw};
	a = cmul(a, rot);
	b = cmul(b, rot);
	c2 res = {a.x + b.x, a.y + -b.y};
	if (g.variant == GRADIENT_NORMAL)
		res = cmul(res, {-ky, kx});
	else if (g.variant == GRADIENT_DISPLACEMENT)
		res = cmul(res, {-ky / (k_len + 0.00001f), kx / (k_len + 0.00001f)});
	if (g.use_bands)
	{
		const float amplitude = band_amplitude(g, fx, fy);
		res.x *= amplitude;
		res.y *= amplitude;
	}
	return float_to_half_pinned(res.x) | (float_to_half_pinned(res.y) << 16);
}

// ---- LinearWrap over a linear image of C fp16 channels a texel ---------------------------------------------------------------
struct Texture
{
	const uint8_t *ptr;
	int w, h;
	uint32_t pitch;
};
template <int C> struct Texel
{
	float v[C];
};
template <int C> GR_HD Texel<C> fetch_wrap(const Texture &t, int x, int y)
{
	const uint16_t *p = reinterpret_cast<const uint16_t *>(t.ptr + size_t(wrapi(y, t.h)) * t.pitch) + size_t(wrapi(x, t.w)) * C;
	Texel<C> r;
	for (int c = 0; c < C; c++)
		r.v[c] = half_to_float(p[c]);
	return r;
}
template <int C> GR_HD Texel<C> lerp(const Texel<C> &lo, const Texel<C> &hi, float t)
{
	Texel<C> r;
	for (int c = 0; c < C; c++)
		r.v[c] = lo.v[c] * (1.0f - t) + hi.v[c] * t;
	return r;
}
// textureLodOffset(sampler, (u, v), 0, (ox, oy))
template <int C> GR_HD Texel<C> sample_wrap(const Texture &t, float u, float v, int ox, int oy)
{
	int x0, y0;
	float a, b;
	linear_axis(u * float(t.w) - 0.5f, x0, a);
	linear_axis(v * float(t.h) - 0.5f, y0, b);
	x0 += ox;
	y0 += oy;
	const Texel<C> top = a == 0.0f ? fetch_wrap<C>(t, x0, y0) : lerp(fetch_wrap<C>(t, x0, y0), fetch_wrap<C>(t, x0 + 1, y0), a);
	if (b == 0.0f)
		return top;
	const Texel<C> bottom = a == 0.0f ? fetch_wrap<C>(t, x0, y0 + 1) : lerp(fetch_wrap<C>(t, x0, y0 + 1), fetch_wrap<C>(t, x0 + 1, y0 + 1), a);
	return lerp(top, bottom, b);
}

struct uint2_bits
{
	uint32_t x, y;
};
GR_HD uint2_bits pack4(float x, float y, float z, float w)
{
	return {float_to_half_pinned(x) | (float_to_half_pinned(y) << 16), float_to_half_pinned(z) | (float_to_half_pinned(w) << 16)};
}

// ---- bake_maps.comp ------------------------------------------------------------------------------------------------------------
struct BakeArgs
{
	Texture height, displacement; // R16F, RG16F
	float inv_size[4], scale[4];
};
// Texel (x, y): what the shader stores to iHeightDisplacement and to iGradJacobian.  Both coordinate pairs advance by inv_size.xy; the
// displacement pair only starts at half a displacement texel, as the shader has it.
GR_HD void bake_texel(const BakeArgs &a, uint32_t x, uint32_t y, uint2_bits &height_displacement, uint2_bits &grad_jacobian)
{
	const float px = float(x) * a.inv_size[0], py = float(y) * a.inv_size[1];
	const float u = px + 0.5f * a.inv_size[0], v = py + 0.5f * a.inv_size[1];
	const float du = px + 0.5f * a.inv_size[2], dv = py + 0.5f * a.inv_size[3];

	const float h = sample_wrap<1>(a.height, u, v, 0, 0).v[0];
	const float x0 = sample_wrap<1>(a.height, u, v, -1, 0).v[0], x1 = sample_wrap<1>(a.height, u, v, 1, 0).v[0];
	const float y0 = sample_wrap<1>(a.height, u, v, 0, -1).v[0], y1 = sample_wrap<1>(a.height, u, v, 0, 1).v[0];
	const float grad_x = (a.scale[0] * 0.5f) * (x1 - x0), grad_y = (a.scale[1] * 0.5f) * (y1 - y0);

	const Texel<2> d = sample_wrap<2>(a.displacement, du, dv, 0, 0);
	const Texel<2> dxp = sample_wrap<2>(a.displacement, du, dv, 1, 0), dxm = sample_wrap<2>(a.displacement, du, dv, -1, 0);
	const Texel<2> dyp = sample_wrap<2>(a.displacement, du, dv, 0, 1), dym = sample_wrap<2>(a.displacement, du, dv, 0, -1);
	const float half_lambda = 0.5f * LAMBDA;
	const float ddx_x = (half_lambda * (dxp.v[0] - dxm.v[0])) * a.scale[2], ddx_y = (half_lambda * (dxp.v[1] - dxm.v[1])) * a.scale[2];
	const float ddy_x = (half_lambda * (dyp.v[0] - dym.v[0])) * a.scale[3], ddy_y = (half_lambda * (dyp.v[1] - dym.v[1])) * a.scale[3];
	const float j = (1.0f + ddx_x) * (1.0f + ddy_y) - ddx_y * ddy_x;

	height_displacement = pack4(h, LAMBDA * d.v[0], LAMBDA * d.v[1], 0.0f);
	grad_jacobian = pack4(grad_x, grad_y, j, 0.0f);
}

// ---- mipmap.comp ---------------------------------------------------------------------------------------------------------------
struct MipmapArgs
{
	Texture in;
	float result_mod[4], inv_resolution[2];
	uint32_t count_x, count_y;
};
// Texel (x, y) of the output, C channels: one LinearWrap tap at (2 gid + 1) * inv_resolution, times result_mod.
template <int C> GR_HD void mipmap_texel(const MipmapArgs &a, uint32_t x, uint32_t y, uint16_t *out)
{
	const float u = (2.0f * float(x) + 1.0f) * a.inv_resolution[0], v = (2.0f * float(y) + 1.0f) * a.inv_resolution[1];
	const Texel<C> t = sample_wrap<C>(a.in, u, v, 0, 0);
	for (int c = 0; c < C; c++)
		out[c] = uint16_t(float_to_half_pinned(a.result_mod[c] * t.v[c]));
}

// ---- update_lod.comp -----------------------------------------------------------------------------------------------------------
// The LOD pass.  Sums are written in the shaders' operation order: dot() adds its products left to right.
constexpr uint32_t MAX_LOD_INDIRECT = 8u;
struct UpdateLodArgs
{
	float camera[3]; // shifted_camera_pos
	float max_lod;
	int offset_x, offset_y; // image_offset
	int n;                  // num_threads, square and a power of two
	float base_x, base_y, size_x, size_y;
	float lod_bias;
};
GR_HD float square_dist(const UpdateLodArgs &a, float px, float pz)
{
	const float dx = a.camera[0] - px, dy = a.camera[1] - 0.0f, dz = a.camera[2] - pz;
	return (dx * dx + dy * dy) + dz * dz;
}
// Block (x, y): the texel it stores to, (id + image_offset) & (n - 1), and the R16F bits of its LOD.
GR_HD uint16_t update_lod_texel(const UpdateLodArgs &a, int x, int y, int &image_x, int &image_y)
{
	const float x00 = a.base_x + float(x) * a.size_x, y00 = a.base_y + float(y) * a.size_y;
	const float x10 = x00 + 1.0f * a.size_x, y10 = y00 + 0.0f * a.size_y;
	const float x01 = x00 + 0.0f * a.size_x, y01 = y00 + 1.0f * a.size_y;
	const float x11 = x00 + 1.0f * a.size_x, y11 = y00 + 1.0f * a.size_y;
	const float xc = x00 + 0.5f * a.size_x, yc = y00 + 0.5f * a.size_y;
	float d = square_dist(a, xc, yc);
	d = fminf(d, square_dist(a, x00, y00));
	d = fminf(d, square_dist(a, x10, y10));
	d = fminf(d, square_dist(a, x01, y01));
	d = fminf(d, square_dist(a, x11, y11));
	float lod = 0.5f * log2f(d + 1.0f) + a.lod_bias;
	lod = fminf(fmaxf(lod, 0.0f), a.max_lod);
	image_x = (x + a.offset_x) & (a.n - 1);
	image_y = (y + a.offset_y) & (a.n - 1);
	return uint16_t(float_to_half_pinned(lod));
}

// ---- cull_blocks.comp ----------------------------------------------------------------------------------------------------------
struct Patch // PatchData of ocean.inc
{
	float offsets[2], inner_lod, padding, lods[4];
};
struct CullArgs
{
	float world_offset[3];
	int offset_x, offset_y; // image_offset
	int n;                  // num_threads, square and a power of two
	float base_x, base_y, size_x, size_y, resolution_x, resolution_y;
	float range_lo, range_hi, guard_band;
	uint32_t lod_stride;
	float max_lod;
	uint32_t handle_edge_lods, wrap;
	float frustum[6][4];
	Texture lods; // R16F, n x n
};
// frustum_cull: the block's box, widened by the guard band and the heightmap range, against six planes; the corner farthest along
// a plane's normal decides, and the first plane that has it behind ends the test.
GR_HD bool box_in_frustum(const CullArgs &a, int x, int y)
{
	const float min_x = a.base_x + float(x) * a.size_x, min_z = a.base_y + float(y) * a.size_y;
	const float max_x = min_x + a.size_x, max_z = min_z + a.size_y;
	const float lo[3] = {(min_x - a.guard_band) + a.world_offset[0], a.range_lo + a.world_offset[1], (min_z - a.guard_band) + a.world_offset[2]};
	const float hi[3] = {(max_x + a.guard_band) + a.world_offset[0], a.range_hi + a.world_offset[1], (max_z + a.guard_band) + a.world_offset[2]};
	for (int i = 0; i < 6; i++)
	{
		const float *p = a.frustum[i];
		const float cx = p[0] > 0.0f ? hi[0] : lo[0], cy = p[1] > 0.0f ? hi[1] : lo[1], cz = p[2] > 0.0f ? hi[2] : lo[2];
		if (((cx * p[0] + cy * p[1]) + cz * p[2]) + 1.0f * p[3] < 0.0f)
			return false;
	}
	return true;
}
// A nearest tap at texel coordinate c of the n x n LOD image: NearestWrap (c mod n; & (n - 1) is Euclidean on two's complement) or
// NearestClamp.  For a power-of-two n and |c| < 2^20 this is the texel that uv = (c + 0.5) / n selects.
GR_HD float lod_tap(const CullArgs &a, int cx, int cy)
{
	if (a.wrap)
	{
		cx &= a.n - 1;
		cy &= a.n - 1;
	}
	else
	{
		cx = cx < 0 ? 0 : (cx > a.n - 1 ? a.n - 1 : cx);
		cy = cy < 0 ? 0 : (cy > a.n - 1 ? a.n - 1 : cy);
	}
	return half_to_float(*reinterpret_cast<const uint16_t *>(a.lods.ptr + size_t(cy) * a.lods.pitch + size_t(cx) * 2u));
}
// Block (x, y) that passed the box test: its patch and its bucket.  The bucket is the shader's int(min(inner, min of the four)), kept
// inside 0 .. max_lod whatever the image holds (the shader indexes with it unchecked; an image of update_lod's never leaves the range).
GR_HD int cull_patch(const CullArgs &a, int x, int y, Patch &patch)
{
	const int cx = x + a.offset_x, cy = y + a.offset_y;
	const float centre = lod_tap(a, cx, cy);
	float l[4] = {lod_tap(a, cx - 1, cy), lod_tap(a, cx + 1, cy), lod_tap(a, cx, cy - 1), lod_tap(a, cx, cy + 1)};
	for (float &v : l)
		v = fmaxf(v, centre);
	if (a.handle_edge_lods)
	{
		if (x == 0)
			l[0] = a.max_lod;
		if (x == a.n - 1)
			l[1] = a.max_lod;
		if (y == 0)
			l[2] = a.max_lod;
		if (y == a.n - 1)
			l[3] = a.max_lod;
	}
	const float least = fminf(centre, fminf(fminf(l[0], l[2]), fminf(l[1], l[3])));
	patch = {{float(cx) * a.resolution_x, float(cy) * a.resolution_y}, centre, 0.0f, {l[0], l[1], l[2], l[3]}};
	return least >= 0.0f ? (least > a.max_lod ? int(a.max_lod) : int(least)) : 0;
}
} // namespace gr_ocean
