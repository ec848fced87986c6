// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen; lights/atmospheric_scatter.h also (c) 2019 Dimas "Dimev",
// "Skythedragon" Leenman): see THIRD_PARTY_NOTICES.md at the repository root.
// The sky pass, the per-pixel arithmetic: skybox.vert / skybox.frag (both HAVE_EMISSIVE settings), lights/atmospheric_scatter.h and
// lights/volumetric_light_setup_sky.comp with inc/cube_coordinates.h.  Shared by the gfx950 kernels (sky.hip) and by a host build the
// CPU tests hold to the executed shaders (tests/cpp/sky_core_host.cpp).  Every line is one IEEE fp32 operation in the shader's order and
// the file is compiled without contraction; expf and powf are the only calls whose results may differ between device and host.  The two
// decisions of the scatter (quadratic < 0; t_diff > 0 and no earth hit) are made of + - * sqrt alone.
//
// The pixel's direction (the rasteriser's interpolation of vDirection is not bit-defined): the matrix is evaluated at
// the pixel centre, Position = 2 (pixel + 0.5) / size - 1, direction = ((c0 * Position.x + c1 * Position.y) + c2) + c3.
//
// texture(uSkybox, vDirection) (LinearClamp, implicit LOD) is env_core.hpp's cube model; the LOD is stated here:
//   - the derivatives come from the directions of the aligned 2 x 2 quad, (x & ~1, x | 1) and (y & ~1, y | 1); they depend on the pixel
//     position alone;
//   - each direction is projected onto the pixel's own face, (sc, tc) / |ma|;
//   - rho = max(|d/dx|, |d/dy|) * size / 2 with Euclidean lengths; lambda = log2(rho), 0 for a zero or non-finite rho, clamped to
//     [0, levels - 1]; a quad partner outside the image contributes 0;
//   - a direction whose face coordinates are not finite (a zero or non-finite vector) reads nothing and gives 0.
#pragma once
#include "env_core.hpp"

namespace gr_sky
{
using gr_core::dot3;
using gr_core::f3;
using gr_core::length3;

constexpr float B_RAYLEIGH[3] = {5.5e-6f, 13.0e-6f, 22.4e-6f};
constexpr float B_MIE = 21.0e-6f;
constexpr float B_ABSORPTION[3] = {2.04e-5f, 4.97e-5f, 1.95e-6f};
constexpr float G = 0.7f;
constexpr float G2 = G * G;
constexpr float H_RAYLEIGH = 8000.0f;
constexpr float H_MIE = 1200.0f;
constexpr float H_ABSORPTION = 30000.0f;
constexpr float ABSORPTION_FALLOFF = 4000.0f;
constexpr float E_RADIUS = 6.371e6f;
constexpr float H_ATMOSPHERE = 100000.0f;

constexpr int APPLY_PRIMARY_STEPS = 16, APPLY_LIGHT_STEPS = 8; // skybox.frag
constexpr int CUBE_PRIMARY_STEPS = 32, CUBE_LIGHT_STEPS = 16;  // volumetric_light_setup_sky.comp

GR_HD f3 add3(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
GR_HD f3 mul3(f3 a, f3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
GR_HD f3 scale3(f3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
// a / length(a): three divisions
GR_HD f3 normalize_div(f3 a)
{
	const float l = length3(a);
	return {a.x / l, a.y / l, a.z / l};
}

GR_HD float phase_rayleigh(float cos_theta)
{
	const float mumu = cos_theta * cos_theta;
	return 3.0f / (50.2654824574f) * (1.0f + mumu);
}
GR_HD float phase_mie(float cos_theta)
{
	const float g = G, gg = G2, mu = cos_theta;
	const float mumu = mu * mu;
	return 3.0f / (25.1327412287f) * ((1.0f - gg) * (mumu + 1.0f)) / (powf(1.0f + gg - 2.0f * mu * g, 1.5f) * (2.0f + gg));
}
GR_HD float density_rayleigh(float h) { return expf(-h / H_RAYLEIGH); }
GR_HD float density_mie(float h) { return expf(-h / H_MIE); }
GR_HD float density_mod_absorption(float h)
{
	const float denom = (H_ABSORPTION - h) / ABSORPTION_FALLOFF;
	return 1.0f / (denom * denom + 1.0f);
}

// false: quadratic < 0 and both roots are 0
GR_HD bool trace_to_sphere(f3 pos, f3 dir, float radius, float &t0, float &t1)
{
	const float b = 2.0f * dot3(pos, dir);
	const float c = dot3(pos, pos) - radius * radius;
	const float quadratic = b * b - 4.0f * c;
	if (quadratic < 0.0f)
	{
		t0 = 0.0f;
		t1 = 0.0f;
		return false;
	}
	const float q = sqrtf(quadratic);
	t0 = (-b - q) * 0.5f;
	t1 = (-b + q) * 0.5f;
	return true;
}

GR_HD f3 sample_optical_depth(float h, float &depth_r, float &depth_m, float step_length)
{
	depth_r = density_rayleigh(h) * step_length;
	depth_m = density_mie(h) * step_length;
	const float depth_a = density_mod_absorption(h) * depth_r;
	const float mie = depth_m * B_MIE;
	return {depth_r * B_RAYLEIGH[0] + mie + depth_a * B_ABSORPTION[0], depth_r * B_RAYLEIGH[1] + mie + depth_a * B_ABSORPTION[1],
	        depth_r * B_RAYLEIGH[2] + mie + depth_a * B_ABSORPTION[2]};
}

GR_HD float sample_height(f3 sample_pos) { return fmaxf(length3(sample_pos) - E_RADIUS, 0.0f); }

GR_HD f3 accumulate_optical_depth(f3 pos, f3 dir, float t, int light_steps)
{
	f3 accumulated = {0.0f, 0.0f, 0.0f};
	const float step_length = t / float(light_steps);
	for (int i = 0; i < light_steps; i++)
	{
		const float t_dir = (float(i) + 0.5f) * step_length;
		const f3 sample_pos = add3(pos, scale3(dir, t_dir));
		float depth_r, depth_m;
		accumulated = add3(accumulated, sample_optical_depth(sample_height(sample_pos), depth_r, depth_m, step_length));
	}
	return accumulated;
}

// The ray's range in the atmosphere, or false where the result is 0: the part of rayleigh_mie_scatter that decides.
GR_HD bool scatter_range(f3 pos, f3 v, float &t_start, float &t_diff)
{
	float atmos0, atmos1, earth0, earth1;
	trace_to_sphere(pos, v, E_RADIUS + H_ATMOSPHERE, atmos0, atmos1);
	atmos0 = fmaxf(atmos0, 0.0f);
	trace_to_sphere(pos, v, 0.98f * E_RADIUS, earth0, earth1);
	const bool intersects_earth = earth0 > 0.0f || earth1 > 0.0f;
	t_start = atmos0;
	t_diff = fmaxf(atmos1 - atmos0, 0.0f);
	return t_diff > 0.0f && !intersects_earth;
}

GR_HD f3 rayleigh_mie_scatter(f3 v, f3 l, float camera_height, int primary_steps, int light_steps)
{
	camera_height = fmaxf(camera_height, 0.0f);
	const f3 pos = {0.0f, E_RADIUS + camera_height, 0.0f};
	float t_start, t_diff;
	if (!scatter_range(pos, v, t_start, t_diff))
		return {0.0f, 0.0f, 0.0f};

	f3 accumulated = {0.0f, 0.0f, 0.0f}, inscatter_rayleigh = {0.0f, 0.0f, 0.0f}, inscatter_mie = {0.0f, 0.0f, 0.0f};
	const float step_length = t_diff / float(primary_steps);
	for (int i = 0; i < primary_steps; i++)
	{
		const float t_view = (float(i) + 0.5f) * step_length + t_start;
		const f3 sample_pos = add3(pos, scale3(v, t_view));
		float depth_r, depth_m;
		const f3 optical_depth_sample = sample_optical_depth(sample_height(sample_pos), depth_r, depth_m, step_length);

		float sun0, t_sun;
		trace_to_sphere(sample_pos, l, E_RADIUS + H_ATMOSPHERE, sun0, t_sun);
		const f3 total = add3(add3(accumulated, scale3(optical_depth_sample, 0.5f)), accumulate_optical_depth(sample_pos, l, t_sun, light_steps));
		const f3 transmittance = {expf(-total.x), expf(-total.y), expf(-total.z)};

		accumulated = add3(accumulated, optical_depth_sample);
		inscatter_rayleigh = add3(inscatter_rayleigh, scale3(transmittance, depth_r));
		inscatter_mie = add3(inscatter_mie, scale3(transmittance, depth_m));
	}

	const float cos_theta = dot3(v, l);
	const float pr = phase_rayleigh(cos_theta);
	inscatter_rayleigh = mul3(inscatter_rayleigh, f3{pr * B_RAYLEIGH[0], pr * B_RAYLEIGH[1], pr * B_RAYLEIGH[2]});
	inscatter_mie = scale3(inscatter_mie, phase_mie(cos_theta) * B_MIE);
	return add3(inscatter_rayleigh, inscatter_mie);
}

// ---- the pixel's direction ------------------------------------------------------------------------------------------------------
GR_HD f3 pixel_direction(const float *inv, uint32_t width, uint32_t height, uint32_t x, uint32_t y)
{
	const float px = 2.0f * (float(x) + 0.5f) / float(width) - 1.0f, py = 2.0f * (float(y) + 0.5f) / float(height) - 1.0f;
	return {inv[0] * px + inv[4] * py + inv[8] + inv[12], inv[1] * px + inv[5] * py + inv[9] + inv[13], inv[2] * px + inv[6] * py + inv[10] + inv[14]};
}

// skybox.frag without HAVE_EMISSIVE
GR_HD f3 sky_procedural(f3 direction, const float *color, const float *sun_direction, float camera_height)
{
	const f3 s = rayleigh_mie_scatter(normalize_div(direction), f3{sun_direction[0], sun_direction[1], sun_direction[2]}, camera_height, APPLY_PRIMARY_STEPS,
	                                  APPLY_LIGHT_STEPS);
	return {color[0] * s.x, color[1] * s.y, color[2] * s.z};
}

// ---- the textured variant ---------------------------------------------------------------------------------------------------------
// (sc, tc) / |ma| of `d` by the row of the Vulkan table that belongs to `face`, whichever axis of d is the longest.
GR_HD void project_on_face(int face, f3 d, float &u, float &v)
{
	float sc, tc, ma;
	switch (face)
	{
	case 0: ma = fabsf(d.x), sc = -d.z, tc = -d.y; break;
	case 1: ma = fabsf(d.x), sc = d.z, tc = -d.y; break;
	case 2: ma = fabsf(d.y), sc = d.x, tc = d.z; break;
	case 3: ma = fabsf(d.y), sc = d.x, tc = -d.z; break;
	case 4: ma = fabsf(d.z), sc = d.x, tc = -d.y; break;
	default: ma = fabsf(d.z), sc = -d.x, tc = -d.y; break;
	}
	u = sc / ma;
	v = tc / ma;
}

GR_HD float cube_lambda(const float *inv, uint32_t width, uint32_t height, uint32_t x, uint32_t y, int face, uint32_t size, uint32_t levels)
{
	const uint32_t x0 = x & ~1u, x1 = x | 1u, y0 = y & ~1u, y1 = y | 1u;
	float len_dx = 0.0f, len_dy = 0.0f;
	if (x1 < width)
	{
		float u0, v0, u1, v1;
		project_on_face(face, pixel_direction(inv, width, height, x0, y), u0, v0);
		project_on_face(face, pixel_direction(inv, width, height, x1, y), u1, v1);
		const float du = u1 - u0, dv = v1 - v0;
		len_dx = sqrtf(du * du + dv * dv);
	}
	if (y1 < height)
	{
		float u0, v0, u1, v1;
		project_on_face(face, pixel_direction(inv, width, height, x, y0), u0, v0);
		project_on_face(face, pixel_direction(inv, width, height, x, y1), u1, v1);
		const float du = u1 - u0, dv = v1 - v0;
		len_dy = sqrtf(du * du + dv * dv);
	}
	const float rho = fmaxf(len_dx, len_dy) * float(size) * 0.5f;
	float lambda = 0.0f;
	if (rho > 0.0f && rho <= 3.402823466e+38f)
		lambda = log2f(rho);
	const float top = float(levels - 1u);
	return lambda < 0.0f ? 0.0f : (lambda > top ? top : lambda);
}

// skybox.frag with HAVE_EMISSIVE: texture(uSkybox, vDirection).rgb * color
GR_HD f3 sky_textured(const gr_env::Cube &cube, const float *inv, uint32_t width, uint32_t height, uint32_t x, uint32_t y, const float *color)
{
	const f3 d = pixel_direction(inv, width, height, x, y);
	float sc, tc, ma;
	const int face = gr_env::select_face(d, sc, tc, ma);
	const float half_inv = 0.5f / ma;
	const float s = sc * half_inv + 0.5f, t = tc * half_inv + 0.5f;
	if (!(fabsf(s) <= 3.402823466e+38f && fabsf(t) <= 3.402823466e+38f))
		return {0.0f, 0.0f, 0.0f};
	const gr_env::LodPair lod = gr_env::trilinear_levels(cube_lambda(inv, width, height, x, y, face, cube.size, cube.levels), cube.levels);
	const f3 texel = gr_env::sample_cube(gr_env::cube_level(cube, lod.level0), gr_env::cube_level(cube, lod.level1), lod.weight, d);
	return {texel.x * color[0], texel.y * color[1], texel.z * color[2]};
}

// ---- volumetric_light_setup_sky.comp ------------------------------------------------------------------------------------------------
GR_HD f3 sky_cube_texel(uint32_t face, uint32_t x, uint32_t y, float inv_resolution, const float *sun_color, const float *sun_direction, float camera_y)
{
	// inc/cube_coordinates.h: base_dirs, pos_du, pos_dv
	const float base[6][3] = {{1.0f, 0.0f, 0.0f}, {-1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, -1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, -1.0f}};
	const float du[6][3] = {{0.0f, 0.0f, -1.0f}, {0.0f, 0.0f, 1.0f}, {1.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {-1.0f, 0.0f, 0.0f}};
	const float dv[6][3] = {{0.0f, -1.0f, 0.0f}, {0.0f, -1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, -1.0f}, {0.0f, -1.0f, 0.0f}, {0.0f, -1.0f, 0.0f}};
	const float u = 2.0f * ((float(x) + 0.5f) * inv_resolution) - 1.0f, v = 2.0f * ((float(y) + 0.5f) * inv_resolution) - 1.0f;
	const f3 n = {base[face][0] + du[face][0] * u + dv[face][0] * v, base[face][1] + du[face][1] * u + dv[face][1] * v, base[face][2] + du[face][2] * u + dv[face][2] * v};
	const f3 s = rayleigh_mie_scatter(normalize_div(n), f3{sun_direction[0], sun_direction[1], sun_direction[2]}, camera_y, CUBE_PRIMARY_STEPS, CUBE_LIGHT_STEPS);
	return {sun_color[0] * s.x, sun_color[1] * s.y, sun_color[2] * s.z};
}
} // namespace gr_sky
