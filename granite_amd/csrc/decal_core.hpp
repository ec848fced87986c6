// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Volumetric decals: the arithmetic of assets/shaders/lights/clusterer_bindless_binning_decal.comp (compute_decal_screen_bb,
// test_decal) and of lights/volumetric_decal.h (apply_volumetric_decals), and this project's model of the texture fetch that header
// leaves to the sampler.  Plain functions: decal.hip calls them from its kernels, tests/cpp/decal_core_host.cpp builds the same text for
// the host, where tests/test_decal_core_cpu.py holds it to the executed shaders (tests/golden/decal_shader_v1.npz).
//
// Floating point: every operation is one IEEE fp32 operation in the order the shaders and oracle/ref_build/glsl_cpu.hpp perform it: dot
// sums left to right, matrix x vector sums column by column, mix(a, b, t) = a * (1 - t) + b * t.  Build without contraction and with
// correctly rounded division and square root.  The one exception is log2 of the texel footprint: the host takes it in double and rounds
// to fp32, the device takes the hardware's 1-ulp v_log_f32; the level blend weight is the only value it reaches.
//
// The texture fetch (a deferred pass has no rasteriser derivatives, so this is a statement, not a restatement):
//   - DefaultGeometryFilterWrap without anisotropy: REPEAT addressing, bilinear, linear between mip levels;
//   - level l of a w0 x h0 texture is max(1, w0 >> l) x max(1, h0 >> l) RGBA8 texels, levels tightly packed one after another;
//   - bilinear: f = u * w - 0.5, i0 = floor(f) wrapped into [0, w), i1 = i0 + 1 wrapped, a = f - floor(f); rows are blended
//     horizontally, then the two rows vertically; sRGB texels are decoded (rgb through the 256-entry table, alpha / 255) before;
//   - derivatives come from the aligned 2 x 2 pixel quad: d/dx = uv(x | 1, y) - uv(x & ~1, y), d/dy = uv(x, y | 1) - uv(x, y & ~1), each
//     pixel's uv taken at its own depth for the same decal; an axis with a pixel outside the image or at depth 0 contributes 0;
//   - rho = max(|d/dx * (w0, h0)|, |d/dy * (w0, h0)|), Euclidean; lambda = log2(rho), 0 where rho is zero or not finite, clamped to
//     [0, num_levels - 1]; levels floor(lambda) and min(floor(lambda) + 1, num_levels - 1) are blended by fract(lambda).
//
// What the shaders leave to their environment and this text decides:
//   - int(z * z_scale) is undefined in GLSL outside int's range; here NaN and anything below 1 give slice 0 and anything from
//     z_max_index + 1 on gives z_max_index, which equals the shader's clamp wherever the shader's conversion is defined;
//   - chunk and decal indices taken from the range buffer are held to num_decals_32 and num_decals; a texture index outside the table
//     skips the decal and reads nothing.
#pragma once
#include <cmath>
#include <cstdint>
#include "core_base.hpp"

namespace gr_decal
{
constexpr uint32_t FORMAT_RGBA8_UNORM = 37u, FORMAT_RGBA8_SRGB = 43u; // GR_FORMAT_R8G8B8A8_UNORM / _SRGB (VkFormat values)

struct Vec2 { float x, y; };
using Vec3 = gr_core::f3;
struct Vec4 { float x, y, z, w; };

// GLSL min / max as glsl_cpu.hpp has them (fminf / fmaxf): the other operand where one is NaN.
GR_HD float min_f(float a, float b) { return fminf(a, b); }
GR_HD float max_f(float a, float b) { return fmaxf(a, b); }

// column-major mat4 x vec4, summed column by column
GR_HD Vec4 mul_mat4(const float *m, float x, float y, float z, float w)
{
	Vec4 r = {m[0] * x, m[1] * x, m[2] * x, m[3] * x};
	r = {r.x + m[4] * y, r.y + m[5] * y, r.z + m[6] * y, r.w + m[7] * y};
	r = {r.x + m[8] * z, r.y + m[9] * z, r.z + m[10] * z, r.w + m[11] * z};
	r = {r.x + m[12] * w, r.y + m[13] * w, r.z + m[14] * w, r.w + m[15] * w};
	return r;
}

// ---- clusterer_bindless_binning_decal.comp ---------------------------------------------------------------------------------------------
struct ScreenBB
{
	Vec4 bb = {1.0f, 1.0f, -1.0f, -1.0f};
	float lo_w = 1.0f, hi_w = -1.0f;
};
GR_HD void update_bb(ScreenBB &s, const Vec4 &clip)
{
	s.lo_w = min_f(s.lo_w, clip.w);
	s.hi_w = max_f(s.hi_w, clip.w);
	const float px = clip.x / clip.w, py = clip.y / clip.w;
	s.bb = {min_f(s.bb.x, px), min_f(s.bb.y, py), max_f(s.bb.z, px), max_f(s.bb.w, py)};
}
GR_HD Vec4 add4(const Vec4 &a, const float *col) { return {a.x + col[0], a.y + col[1], a.z + col[2], a.w + col[3]}; }

// compute_decal_screen_bb (:37-67): the unit box's eight corners, built from corner0 and the columns
GR_HD Vec4 compute_decal_screen_bb(const float *mvp)
{
	ScreenBB s;
	const Vec4 corner0 = mul_mat4(mvp, -0.5f, -0.5f, -0.5f, 1.0f);
	update_bb(s, corner0);
	const Vec4 corner1 = add4(corner0, mvp + 0);
	update_bb(s, corner1);
	const Vec4 corner2 = add4(corner0, mvp + 4);
	update_bb(s, corner2);
	const Vec4 corner3 = add4(corner1, mvp + 4);
	update_bb(s, corner3);
	update_bb(s, add4(corner0, mvp + 8));
	update_bb(s, add4(corner1, mvp + 8));
	update_bb(s, add4(corner2, mvp + 8));
	update_bb(s, add4(corner3, mvp + 8));
	if (s.hi_w <= 0.0f)
		return {-10.0f, -10.0f, -10.0f, -10.0f};
	if (s.lo_w <= 0.0f)
		return {-1.0f, -1.0f, 1.0f, 1.0f};
	return s.bb;
}

// test_decal (:28-31), strict on both sides
GR_HD bool test_decal(float u, float v, float stride_u, float stride_v, const Vec4 &bb)
{
	return u + stride_u > bb.x && v + stride_v > bb.y && u < bb.z && v < bb.w;
}

// 2.0 * vec2(cell) * inv_resolution - 1.0 for one axis (:80,98)
GR_HD float cell_uv(uint32_t cell, float inv_resolution) { return 2.0f * float(cell) * inv_resolution - 1.0f; }

// ---- volumetric_decal.h ------------------------------------------------------------------------------------------------------------------
// clustering.vert:10-13 / clustering.frag:37-39: clip = inv_view_projection * (ndc.xy, depth, 1), pos = clip.xyz / clip.w
GR_HD Vec3 world_position(const float *inv_vp, uint32_t x, uint32_t y, float inv_width, float inv_height, float depth)
{
	const float ndc_x = 2.0f * (float(x) + 0.5f) * inv_width - 1.0f;
	const float ndc_y = 2.0f * (float(y) + 0.5f) * inv_height - 1.0f;
	const Vec4 clip = mul_mat4(inv_vp, ndc_x, ndc_y, depth, 1.0f);
	return {clip.x / clip.w, clip.y / clip.w, clip.z / clip.w};
}

// ivec2(gl_FragCoord.xy * inv_resolution * xy_scale), clamped to the grid, for one axis (:26-27)
GR_HD int cluster_cell(uint32_t p, float inv_resolution, float xy_scale, int resolution)
{
	const int c = int((float(p) + 0.5f) * inv_resolution * xy_scale); // >= 0 and far below 2^31 for every image the launcher takes
	return c < resolution - 1 ? c : resolution - 1;
}

// int(dot(pos - camera_base, camera_front) * z_scale) clamped to [0, z_max_index] (:31-33)
GR_HD int z_slice(const Vec3 &pos, const float *camera_base, const float *camera_front, float z_scale, int z_max_index)
{
	const float dx = pos.x - camera_base[0], dy = pos.y - camera_base[1], dz = pos.z - camera_base[2];
	const float z = (dx * camera_front[0] + dy * camera_front[1] + dz * camera_front[2]) * z_scale;
	if (!(z >= 1.0f))
		return 0;
	if (z >= float(z_max_index + 1))
		return z_max_index;
	return int(z);
}

// cluster_mask_range (clusterer_bindless_buffers.h:17-27)
GR_HD uint32_t cluster_mask_range(uint32_t mask, uint32_t range_x, uint32_t range_y, uint32_t start_index)
{
	auto clamp_u = [](uint32_t v, uint32_t lo, uint32_t hi) { v = v > lo ? v : lo; return v < hi ? v : hi; };
	range_x = clamp_u(range_x, start_index, start_index + 32u);
	range_y = clamp_u(range_y + 1u, range_x, start_index + 32u);
	const uint32_t num_bits = range_y - range_x;
	const uint32_t range_mask = num_bits == 32u ? 0xffffffffu : ((1u << num_bits) - 1u) << (range_x - start_index);
	return mask & range_mask;
}

// uvw = (dot(row0, (pos, 1)), dot(row1, ..), dot(row2, ..)) (:50-56); rows = 12 floats of a mat_affine
GR_HD Vec3 decal_uvw(const float *rows, const Vec3 &pos)
{
	auto row_dot = [&](const float *r) { return r[0] * pos.x + r[1] * pos.y + r[2] * pos.z + r[3] * 1.0f; };
	return {row_dot(rows), row_dot(rows + 4), row_dot(rows + 8)};
}
GR_HD bool uvw_in_range(const Vec3 &uvw) { return fabsf(uvw.x) < 0.5f && fabsf(uvw.y) < 0.5f && fabsf(uvw.z) < 0.5f; }

// ---- the texture fetch --------------------------------------------------------------------------------------------------------------------
struct Texture // gr_decal_texture
{
	const void *levels;
	uint32_t width, height, num_levels, format;
};
static_assert(sizeof(Texture) == 24, "gr_decal_texture");

GR_HD float log2_rho(float rho)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_logf(rho);
#else
	return float(log2(double(rho)));
#endif
}

// lambda from the quad's differences (zero for an axis that does not count)
GR_HD float texture_lod(float dudx, float dvdx, float dudy, float dvdy, uint32_t width, uint32_t height, uint32_t num_levels)
{
	const float w = float(width), h = float(height);
	const float ax = dudx * w, ay = dvdx * h, bx = dudy * w, by = dvdy * h;
	const float len_x = sqrtf(ax * ax + ay * ay), len_y = sqrtf(bx * bx + by * by);
	const float rho = max_f(len_x, len_y);
	if (!(rho > 0.0f) || !(rho <= 3.402823466e38f))
		return 0.0f;
	const float lambda = log2_rho(rho);
	const float top = float(num_levels - 1u);
	return lambda > 0.0f ? (lambda < top ? lambda : top) : 0.0f;
}

GR_HD int wrap_repeat(int i, int n)
{
	i %= n;
	return i < 0 ? i + n : i;
}

GR_HD Vec4 decode_texel(uint32_t texel, bool srgb, const float *srgb_table)
{
	const uint32_t r = texel & 255u, g = (texel >> 8) & 255u, b = (texel >> 16) & 255u, a = texel >> 24;
	if (srgb)
		return {srgb_table[r], srgb_table[g], srgb_table[b], float(a) / 255.0f};
	return {float(r) / 255.0f, float(g) / 255.0f, float(b) / 255.0f, float(a) / 255.0f};
}

GR_HD Vec4 mix4(const Vec4 &a, const Vec4 &b, float t)
{
	const float s = 1.0f - t;
	return {a.x * s + b.x * t, a.y * s + b.y * t, a.z * s + b.z * t, a.w * s + b.w * t};
}

// one bilinear fetch at `level`; `offset` = texels before that level
GR_HD Vec4 sample_level(const Texture &t, uint32_t level, float u, float v, const float *srgb_table)
{
	uint32_t offset = 0u;
	for (uint32_t l = 0; l < level; l++)
	{
		const uint32_t lw = t.width >> l, lh = t.height >> l;
		offset += (lw ? lw : 1u) * (lh ? lh : 1u);
	}
	const int w = int((t.width >> level) ? (t.width >> level) : 1u), h = int((t.height >> level) ? (t.height >> level) : 1u);
	const float fx = u * float(w) - 0.5f, fy = v * float(h) - 0.5f;
	const float flx = floorf(fx), fly = floorf(fy);
	const float a = fx - flx, b = fy - fly;
	// |uvw| < 0.5 for every fetch that is used, so u, v lie in (0, 1) and the floors are far inside int
	const int x0 = wrap_repeat(int(flx), w), y0 = wrap_repeat(int(fly), h);
	const int x1 = wrap_repeat(x0 + 1, w), y1 = wrap_repeat(y0 + 1, h);
	const uint32_t *texels = static_cast<const uint32_t *>(t.levels) + offset;
	const bool srgb = t.format == FORMAT_RGBA8_SRGB;
	const Vec4 t00 = decode_texel(texels[y0 * w + x0], srgb, srgb_table), t10 = decode_texel(texels[y0 * w + x1], srgb, srgb_table);
	const Vec4 t01 = decode_texel(texels[y1 * w + x0], srgb, srgb_table), t11 = decode_texel(texels[y1 * w + x1], srgb, srgb_table);
	return mix4(mix4(t00, t10, a), mix4(t01, t11, a), b);
}

GR_HD Vec4 sample_texture(const Texture &t, float u, float v, float lambda, const float *srgb_table)
{
	const float base = floorf(lambda);
	const uint32_t l0 = uint32_t(base), l1 = l0 + 1u < t.num_levels ? l0 + 1u : t.num_levels - 1u;
	const Vec4 c0 = sample_level(t, l0, u, v, srgb_table);
	const float weight = lambda - base;
	// a whole lambda (every magnified fetch: lambda clamps to 0): c0 * 1 + c1 * 0 is c0 itself for the finite, non-negative values a
	// texel decodes to, so the second level is not fetched
	if (weight == 0.0f)
		return c0;
	const Vec4 c1 = sample_level(t, l1, u, v, srgb_table);
	return mix4(c0, c1, weight);
}

// base_color = mix(base_color, decal_color, decal_color.a), rgb only: the G-buffer's alpha is never changed
GR_HD Vec3 blend_decal(const Vec3 &base, const Vec4 &decal)
{
	const float s = 1.0f - decal.w;
	return {base.x * s + decal.x * decal.w, base.y * s + decal.y * decal.w, base.z * s + decal.z * decal.w};
}
} // namespace gr_decal
