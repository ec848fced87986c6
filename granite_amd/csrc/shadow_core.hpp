// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Directional-light shadows, the per-pixel arithmetic: lights/directional.frag with SHADOWS, compute_lighting of lights/lighting.h,
// compute_shadow_cascade and both get_directional_shadow_term of lights/lighting_resources.h, lights/pcf.h (both kernels), lights/vsm.h,
// lights/resolve_vsm.frag and post/vsm_{down,up}_blur.frag.  Shared by the gfx950 kernels (shadow.hip) and by a host build the CPU tests hold
// to the executed shaders (tests/cpp/shadow_core_host.cpp).  Every line is one IEEE fp32 operation in the shader's order and the file is
// compiled without contraction; log2f, exp2f and powf are the only calls whose results may differ between device and host.
//
// The LinearShadow sampler (vulkan/device.cpp: compare GREATER_OR_EQUAL, linear, clamp to edge): the footprint and the two
// weights are those of the LinearClamp model (core_base.hpp: linear_axis, with its snap onto texel centres); each of the four texels,
// its coordinates clamped to the edge, is compared with the reference first -- 1 where ref >= texel, else 0 -- and the weights blend the four
// results, horizontally then vertically.  A gather with a reference returns the four compare results of the footprint at
// floor(uv * size - 0.5), in the order (0, 1), (1, 1), (1, 0), (0, 0).  A D16_UNORM texel is v / 65535.
#pragma once
#include "core_base.hpp"

namespace gr_shadow
{
using gr_core::clampi;
using gr_core::dot3;
using gr_core::f3;
using gr_core::SAMPLER_SNAP;

constexpr int NUM_CASCADES = 4; // SHADOW_NUM_CASCADES
constexpr int MODE_PCF = 1, MODE_PCF_WIDE = 2, MODE_VSM = 3; // GR_SHADOW_*
constexpr float PI_SIC = 3.1415628f; // pbr.h:4-6 (sic)

// One layer of the shadow map; every layer has the size and the format of the others.
struct Layer
{
	const uint8_t *ptr;
	uint32_t pitch;
};
struct Maps
{
	Layer layer[NUM_CASCADES];
	int width, height;
};

// ---- texels ------------------------------------------------------------------------------------------------------------------------
template <bool D16> GR_HD float depth_texel(const Layer &l, int x, int y)
{
	const uint8_t *row = l.ptr + size_t(y) * l.pitch;
	if (D16)
		return float(reinterpret_cast<const uint16_t *>(row)[x]) / 65535.0f;
	return reinterpret_cast<const float *>(row)[x];
}
GR_HD float compare(float ref, float texel) { return ref >= texel ? 1.0f : 0.0f; }

// linear_axis with the edge clamp made before the conversion to int: a coordinate far outside the map, infinite or NaN reads the edge
// texels and converts nothing that an int does not hold.  i0 and i1 are the clamped indices of the footprint's two texels.
GR_HD void clamped_axis(float f, int size, int &i0, int &i1, float &weight)
{
	const float fl = floorf(f + SAMPLER_SNAP);
	float a = f - fl;
	if (a < SAMPLER_SNAP)
		a = 0.0f;
	const int i = int(fminf(fmaxf(fl, -1.0f), float(size)));
	i0 = clampi(i, 0, size - 1);
	i1 = clampi(i + 1, 0, size - 1);
	weight = a;
}
// The two lerps of a bilinear fetch in the order every sampler of the oracle uses (oracle_common.h: linear_combine).
GR_HD float linear_combine(float t00, float t10, float t01, float t11, float a, float b)
{
	const float top = (a == 0.0f) ? t00 : t00 * (1.0f - a) + t10 * a;
	if (b == 0.0f)
		return top;
	const float bot = (a == 0.0f) ? t01 : t01 * (1.0f - a) + t11 * a;
	return top * (1.0f - b) + bot * b;
}

// texture(sampler2DArrayShadow, vec4(uv, layer, ref)) and textureProjLod(sampler2DShadow, vec4(uv, ref, 1), 0) through LinearShadow
template <bool D16> GR_HD float linear_shadow(const Layer &l, int w, int h, float u, float v, float ref)
{
	int x0, x1, y0, y1;
	float a, b;
	clamped_axis(u * float(w) - 0.5f, w, x0, x1, a);
	clamped_axis(v * float(h) - 0.5f, h, y0, y1, b);
	return linear_combine(compare(ref, depth_texel<D16>(l, x0, y0)), compare(ref, depth_texel<D16>(l, x1, y0)), compare(ref, depth_texel<D16>(l, x0, y1)),
	                      compare(ref, depth_texel<D16>(l, x1, y1)), a, b);
}

// textureLod(sampler2D[Array], uv, 0).xy of an R32G32_SFLOAT image through LinearClamp
GR_HD void linear_moments(const Layer &l, int w, int h, float u, float v, float &mx, float &my)
{
	int x0, x1, y0, y1;
	float a, b;
	clamped_axis(u * float(w) - 0.5f, w, x0, x1, a);
	clamped_axis(v * float(h) - 0.5f, h, y0, y1, b);
	const float *r0 = reinterpret_cast<const float *>(l.ptr + size_t(y0) * l.pitch), *r1 = reinterpret_cast<const float *>(l.ptr + size_t(y1) * l.pitch);
	mx = linear_combine(r0[2 * x0], r0[2 * x1], r1[2 * x0], r1[2 * x1], a, b);
	my = linear_combine(r0[2 * x0 + 1], r0[2 * x1 + 1], r1[2 * x0 + 1], r1[2 * x1 + 1], a, b);
}

// ---- lights/vsm.h ------------------------------------------------------------------------------------------------------------------
GR_HD float vsm(float depth, float mx, float my)
{
	float shadow_term = 1.0f;
	if (depth > mx)
	{
		const float variance = fmaxf(my - mx * mx, 0.00001f);
		const float d = depth - mx;
		shadow_term = variance / (variance + d * d);
		shadow_term = fminf(fmaxf((shadow_term - 0.25f) / 0.75f, 0.0f), 1.0f);
	}
	return shadow_term;
}

// ---- lights/pcf.h ------------------------------------------------------------------------------------------------------------------
GR_HD float pcf_kernel(float p)
{
	const float p2 = p * p;
	return exp2f(-0.375f * p2) * (1.0f - p2 / 9.0f);
}

// SAMPLE_PCF_GATHER with SHADOW_MAP_PCF_KERNEL_WIDE: nine gathers over the 6 x 6 texels from floor(uv * size - 1.5), weighted by the
// windowed Gaussian and divided by the weights' sum.  SAMPLE_PCF_ADJUST moves uv to floored / size and each gather floors
// (floored / size) * size - 0.5 again: that is floored - 1 for every |floored| below 2^20 (two roundings move the product by less than
// 1 / 8), and beyond that -- or beyond the map, which is at most 16384 texels wide -- every tap reads the same edge texel.  The index
// is therefore formed from `floored` directly, clamped before it is converted.
template <bool D16> GR_HD float pcf_wide(const Layer &l, int w, int h, float u, float v, float ref_z)
{
	const float ix = u * float(w) - 1.5f, iy = v * float(h) - 1.5f;
	const float fx = floorf(ix), fy = floorf(iy);
	const float cx = ix - fx, cy = iy - fy;
	const int x_first = int(fminf(fmaxf(fx, -8.0f), float(w) + 8.0f)) - 1, y_first = int(fminf(fmaxf(fy, -8.0f), float(h) + 8.0f)) - 1;

	// horiz_coeff0.xyzw, horiz_coeff1.xy: the weights of the six columns, left to right; vert_*: of the six rows, top to bottom
	const float offsets[6] = {2.0f, 1.0f, 0.0f, -1.0f, -2.0f, -3.0f};
	float hw[6], vw[6];
	GR_UNROLL
	for (int i = 0; i < 6; i++)
	{
		hw[i] = pcf_kernel(cx + offsets[i]);
		vw[i] = pcf_kernel(cy + offsets[i]);
	}
	int xs[6];
	GR_UNROLL
	for (int i = 0; i < 6; i++)
		xs[i] = clampi(x_first + i, 0, w - 1);

	float var = 0.0f, total_w = 0.0f;
	GR_UNROLL
	for (int gy = 0; gy < 3; gy++)
	{
		const int r0 = clampi(y_first + 2 * gy, 0, h - 1), r1 = clampi(y_first + 2 * gy + 1, 0, h - 1);
		GR_UNROLL
		for (int gx = 0; gx < 3; gx++)
		{
			const int c0 = xs[2 * gx], c1 = xs[2 * gx + 1];
			// the gather's components and `horiz.xyyx * vert.yyxx`: (c0, r1), (c1, r1), (c1, r0), (c0, r0)
			const float g_x = compare(ref_z, depth_texel<D16>(l, c0, r1)), g_y = compare(ref_z, depth_texel<D16>(l, c1, r1));
			const float g_z = compare(ref_z, depth_texel<D16>(l, c1, r0)), g_w = compare(ref_z, depth_texel<D16>(l, c0, r0));
			const float k_x = hw[2 * gx] * vw[2 * gy + 1], k_y = hw[2 * gx + 1] * vw[2 * gy + 1];
			const float k_z = hw[2 * gx + 1] * vw[2 * gy], k_w = hw[2 * gx] * vw[2 * gy];
			var = var + (((g_x * k_x + g_y * k_y) + g_z * k_z) + g_w * k_w);
			total_w = total_w + ((k_x + k_z) + (k_y + k_w));
		}
	}
	return var / total_w;
}

// SAMPLE_PCF_KERNEL / SAMPLE_PCF_KERNEL_LAYER_NOPROJ and the VSM lookup of one layer at the light-space position `clip`.  The plain
// variants divide by w = 1, which changes no value.
template <int MODE, bool D16> GR_HD float layer_term(const Layer &l, int w, int h, f3 clip)
{
	if (MODE == MODE_VSM)
	{
		float mx, my;
		linear_moments(l, w, h, clip.x, clip.y, mx, my);
		return vsm(clip.z, mx, my);
	}
	if (MODE == MODE_PCF_WIDE)
		return pcf_wide<D16>(l, w, h, clip.x, clip.y, clip.z);
	return linear_shadow<D16>(l, w, h, clip.x, clip.y, clip.z);
}

// ---- compute_shadow_cascade (lighting_resources.h) ------------------------------------------------------------------------------------
struct Cascade
{
	int layer_near, layer_far;
	float shadow_lerp, white_lerp;
};
GR_HD Cascade compute_shadow_cascade(f3 world_pos, f3 camera_pos, f3 camera_front, float cascade_log_bias)
{
	const f3 rel = {world_pos.x - camera_pos.x, world_pos.y - camera_pos.y, world_pos.z - camera_pos.z};
	const float view_z = fmaxf(dot3(camera_front, rel), 0.0f);
	float shadow_cascade = log2f(view_z) + cascade_log_bias; // view_z = 0: -inf, which the max below turns into cascade 0
	shadow_cascade = fmaxf(shadow_cascade, 0.0f);
	Cascade c;
	// int(shadow_cascade) of a value at or above the cascade count ends as the last layer: clamped before the conversion
	c.layer_near = int(fminf(shadow_cascade, float(NUM_CASCADES)));
	if (c.layer_near > NUM_CASCADES - 1)
		c.layer_near = NUM_CASCADES - 1;
	c.layer_far = c.layer_near + 1 < NUM_CASCADES - 1 ? c.layer_near + 1 : NUM_CASCADES - 1;

	constexpr float BEGIN_LERP_FRACT = 0.8f;
	constexpr float INV_BEGIN_LERP_FRACT = 1.0f / (1.0f - BEGIN_LERP_FRACT);
	c.shadow_lerp = INV_BEGIN_LERP_FRACT * fmaxf((shadow_cascade - floorf(shadow_cascade)) - BEGIN_LERP_FRACT, 0.0f);
	if (c.layer_near == c.layer_far)
		c.shadow_lerp = 0.0f;
	else if (c.shadow_lerp == 0.0f)
		c.layer_far = c.layer_near;

	constexpr float MAX_CASCADE = float(NUM_CASCADES);
	constexpr float INV_MAX_CASCADE = 100.0f / MAX_CASCADE;
	c.white_lerp = fminf(fmaxf(INV_MAX_CASCADE * (shadow_cascade - 0.99f * MAX_CASCADE), 0.0f), 1.0f);
	return c;
}

// (SHADOW_TRANSFORMS[i] * vec4(world_pos, 1)).xyz, m column-major
GR_HD f3 light_clip(const float *m, f3 p)
{
	return {((m[0] * p.x + m[4] * p.y) + m[8] * p.z) + m[12], ((m[1] * p.x + m[5] * p.y) + m[9] * p.z) + m[13],
	        ((m[2] * p.x + m[6] * p.y) + m[10] * p.z) + m[14]};
}
GR_HD float mix1(float a, float b, float t) { return a * (1.0f - t) + b * t; }

// One turn of the shader's `for (i = wave_minimum_layer; i <= wave_maximum_layer; i++)`: layer i's matrix and map are the same for
// every lane of the turn (scalar loads on the device); a lane whose layer_near is i takes the lookup as its near term, a lane that blends
// and whose layer_far is i as its far term.  The shader fetches after the loop, from the positions the loop selected: the same lookups.
// Walking i over a lane's own layer_near .. layer_far alone gives that lane the same two terms.
template <int MODE, bool D16>
GR_HD void cascade_turn(const Maps &maps, const float *transforms, int i, const Cascade &c, f3 world_pos, float &term_near, float &term_far)
{
	const bool is_near = i == c.layer_near, is_far = i != c.layer_near && i == c.layer_far && c.shadow_lerp > 0.0f;
	if (is_near || is_far)
	{
		const float term = layer_term<MODE, D16>(maps.layer[i], maps.width, maps.height, light_clip(transforms + 16 * i, world_pos));
		if (is_near)
			term_near = term;
		else
			term_far = term;
	}
}
// get_directional_shadow_term with SHADOW_CASCADES, behind the lookups
GR_HD float blend_cascade(const Cascade &c, float term_near, float term_far)
{
	float shadow_term = term_near;
	if (c.shadow_lerp > 0.0f)
		shadow_term = mix1(shadow_term, term_far, c.shadow_lerp);
	return mix1(shadow_term, 1.0f, c.white_lerp);
}

// ---- the fragment: directional.frag's main and compute_lighting (LIGHTING_NO_AMBIENT) ---------------------------------------------------
struct Material
{
	f3 base;   // linear base colour (its alpha, the ambient factor, is not read under LIGHTING_NO_AMBIENT)
	f3 normal; // the attachment's value * 2 - 1
	float metallic, roughness;
};
// A2B10G10R10 normal and R8G8 metallic / roughness words; base colour through the 256-entry sRGB decode table
GR_HD Material decode_material(uint32_t albedo, uint32_t normal, uint32_t pbr, const float *srgb_decode)
{
	Material m;
	m.base = {srgb_decode[albedo & 255u], srgb_decode[(albedo >> 8) & 255u], srgb_decode[(albedo >> 16) & 255u]};
	m.normal = {float(normal & 1023u) / 1023.0f * 2.0f - 1.0f, float((normal >> 10) & 1023u) / 1023.0f * 2.0f - 1.0f,
	            float((normal >> 20) & 1023u) / 1023.0f * 2.0f - 1.0f};
	m.metallic = gr_core::unorm8_to_float(pbr & 255u);
	m.roughness = gr_core::unorm8_to_float((pbr >> 8) & 255u);
	return m;
}

// vClip + depth * inverse_view_projection_col2, xyz / w; vClip = inv_view_projection * (ndc, 0, 1) at the pixel centre
// (oracle/ref_build/ref_lighting.cpp states the rasteriser's part the same way)
GR_HD f3 world_position(const float *inv_vp, const float *col2, float inv_width, float inv_height, uint32_t x, uint32_t y, float depth)
{
	const float ndc_x = 2.0f * ((float(x) + 0.5f) * inv_width) - 1.0f, ndc_y = 2.0f * ((float(y) + 0.5f) * inv_height) - 1.0f;
	float clip[4];
	GR_UNROLL
	for (int k = 0; k < 4; k++)
		clip[k] = (((inv_vp[k] * ndc_x + inv_vp[4 + k] * ndc_y) + inv_vp[8 + k] * 0.0f) + inv_vp[12 + k]) + depth * col2[k];
	return {clip[0] / clip[3], clip[1] / clip[3], clip[2] / clip[3]};
}

GR_HD f3 normalize_div(f3 a)
{
	const float l = sqrtf(dot3(a, a));
	return {a.x / l, a.y / l, a.z / l};
}
GR_HD float clamp1(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// compute_lighting: light_color * NoL * shadow_term * (...) multiplied from the left, as the shader spells it
GR_HD f3 compute_lighting(const Material &m, float shadow_term, f3 world_pos, f3 camera_pos, f3 light_direction, f3 light_color)
{
	const float roughness = m.roughness * 0.75f + 0.25f;
	const f3 L = light_direction;
	const f3 V = normalize_div({camera_pos.x - world_pos.x, camera_pos.y - world_pos.y, camera_pos.z - world_pos.z});
	const f3 H = normalize_div({V.x + L.x, V.y + L.y, V.z + L.z});
	const f3 N = m.normal;
	const float NoV = clamp1(dot3(N, V), 0.001f, 1.0f);
	const float NoL = clamp1(dot3(N, L), 0.001f, 1.0f);
	const float HoV = clamp1(dot3(H, V), 0.001f, 1.0f);

	const float one_minus_metallic = 1.0f - m.metallic;
	const f3 F0 = {0.04f * one_minus_metallic + m.base.x * m.metallic, 0.04f * one_minus_metallic + m.base.y * m.metallic,
	               0.04f * one_minus_metallic + m.base.z * m.metallic};
	const float f = powf(1.0f - HoV, 5.0f);
	const f3 fresnel = {F0.x * (1.0f - f) + 1.0f * f, F0.y * (1.0f - f) + 1.0f * f, F0.z * (1.0f - f) + 1.0f * f};

	// cook_torrance_specular: specular * G * D
	const float NoH = clamp1(dot3(N, H), 0.0001f, 1.0f);
	const float mm = roughness * roughness;
	const float m2 = mm * mm;
	const float d = (NoH * m2 - NoH) * NoH + 1.0f;
	const float D = m2 / (PI_SIC * d * d);
	const float r = roughness + 1.0f;
	const float k = r * r * (1.0f / 8.0f);
	const float Gv = NoV * (1.0f - k) + k;
	const float Gl = NoL * (1.0f - k) + k;
	const float G = 0.25f / fmaxf(Gv * Gl, 0.001f);
	const f3 cook = {fresnel.x * G * D, fresnel.y * G * D, fresnel.z * G * D};

	const f3 lit = {light_color.x * NoL * shadow_term, light_color.y * NoL * shadow_term, light_color.z * NoL * shadow_term};
	const f3 specref = {lit.x * cook.x, lit.y * cook.y, lit.z * cook.z};
	constexpr float INV_PI = 1.0f / PI_SIC;
	const f3 diffref = {lit.x * (1.0f - fresnel.x) * INV_PI, lit.y * (1.0f - fresnel.y) * INV_PI, lit.z * (1.0f - fresnel.z) * INV_PI};
	const f3 diffuse = {diffref.x * m.base.x * one_minus_metallic, diffref.y * m.base.y * one_minus_metallic, diffref.z * m.base.z * one_minus_metallic};
	return {specref.x + diffuse.x, specref.y + diffuse.y, specref.z + diffuse.z};
}

// textureLod(uAmbientOcclusion, gl_FragCoord.xy * inv_resolution, 0).x: an R8_UNORM image through LinearClamp
GR_HD float sample_ambient_occlusion(const uint8_t *ptr, uint32_t pitch, int w, int h, float u, float v)
{
	int x0, x1, y0, y1;
	float a, b;
	clamped_axis(u * float(w) - 0.5f, w, x0, x1, a);
	clamped_axis(v * float(h) - 0.5f, h, y0, y1, b);
	const uint8_t *r0 = ptr + size_t(y0) * pitch, *r1 = ptr + size_t(y1) * pitch;
	return linear_combine(gr_core::unorm8_to_float(r0[x0]), gr_core::unorm8_to_float(r0[x1]), gr_core::unorm8_to_float(r1[x0]),
	                      gr_core::unorm8_to_float(r1[x1]), a, b);
}
// FragColor += base_ambient * base_color.rgb * vec3(0.05) (VOLUMETRIC_DIFFUSE_FALLBACK)
GR_HD f3 add_ambient_fallback(f3 colour, f3 base, float base_ambient)
{
	return {colour.x + base_ambient * base.x * 0.05f, colour.y + base_ambient * base.y * 0.05f, colour.z + base_ambient * base.z * 0.05f};
}

// ---- the VSM chain -------------------------------------------------------------------------------------------------------------------
// vsm_down_blur.frag (spread 1.75) and vsm_up_blur.frag (0.875): nine LinearClamp taps around the output pixel's centre, offsets in texels
// of the input, weights 0.25 / 0.125 / 0.0625 in the shader's order of accumulation
GR_HD void vsm_blur(const Layer &in, int in_w, int in_h, float u, float v, float spread, float &out_x, float &out_y)
{
	const float inv_x = 1.0f / float(in_w), inv_y = 1.0f / float(in_h);
	const float ox[9] = {0.0f, -spread, 0.0f, spread, -spread, spread, -spread, 0.0f, spread};
	const float oy[9] = {0.0f, spread, spread, spread, 0.0f, 0.0f, -spread, -spread, -spread};
	const float weight[9] = {0.25f, 0.0625f, 0.125f, 0.0625f, 0.125f, 0.125f, 0.0625f, 0.125f, 0.0625f};
	float sx = 0.0f, sy = 0.0f;
	GR_UNROLL
	for (int i = 0; i < 9; i++)
	{
		float mx, my;
		linear_moments(in, in_w, in_h, u + ox[i] * inv_x, v + oy[i] * inv_y, mx, my);
		sx = i == 0 ? weight[i] * mx : sx + weight[i] * mx;
		sy = i == 0 ? weight[i] * my : sy + weight[i] * my;
	}
	out_x = sx;
	out_y = sy;
}
} // namespace gr_shadow
