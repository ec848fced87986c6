// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Environment baking, the per-texel arithmetic: skybox_latlon.frag (HAVE_EMISSIVE), the linear blit of generate_mipmap,
// util/ibl_specular.frag and util/ibl_diffuse.frag, and the cube sampler they read through.  Shared by the gfx950 kernels
// (environment.hip) and by a host build the CPU tests hold to the executed shaders (tests/cpp/env_core_host.cpp): the kernels add the
// split of a texel's taps over lanes, the LDS tables and the launch geometry around these functions, nothing else.
//
// A cube is an R16G16B16A16_SFLOAT mip chain laid out as a GTX payload: levels in order (each 48 * n^2 bytes, so every level starts
// 16-byte aligned), six faces +X -X +Y -Y +Z -Z per level, rows tightly packed, level l being max(size >> l, 1) texels a side.
//
// Cube sampling model (the reference leaves it to the Vulkan implementation):
//   - face and (s, t) from the major axis by the Vulkan table, ties resolved Z over Y over X;
//   - bilinear inside a level with the project's linear_axis rule (exact fp32 weights, 2^-8 snap onto texel centres);
//   - a footprint texel off the face is resolved seamlessly: its centre is turned back into a direction on the face plane and read
//     as the nearest texel of the face that direction selects;
//   - trilinear: lod clamped to [0, levels - 1], linear_axis(lod) gives floor(lod) and the weight of the next level.
#pragma once
#include "core_base.hpp"

namespace gr_env
{
using gr_core::clampi;
using gr_core::cross3;
using gr_core::dot3;
using gr_core::f3;
using gr_core::float_to_half;
using gr_core::half_to_float;
using gr_core::linear_axis;
using gr_core::make3;
using gr_core::normalize3;
using gr_core::wrapi;

constexpr float SHADER_PI = 3.1415628f; // as the two IBL shaders spell it
constexpr uint32_t SPECULAR_SAMPLES = 1024u;
constexpr float DIFFUSE_DELTA = 0.025f;
constexpr uint32_t DIFFUSE_PHI_STEPS = 252u, DIFFUSE_THETA_STEPS = 63u; // what the two float loops run to (checked on the host)
constexpr uint32_t MAX_LEVELS = 16u;

#if !defined(__HIPCC__)
struct uint2
{
	uint32_t x, y;
};
#endif

// ---- layout ----------------------------------------------------------------------------------------------------------------
GR_HD uint32_t level_size(uint32_t size, uint32_t level)
{
	const uint32_t n = level < 32u ? size >> level : 0u;
	return n ? n : 1u;
}
// log2(size) + 1: the levels of a full chain
GR_HD uint32_t full_chain_levels(uint32_t size)
{
	uint32_t levels = 0;
	for (; size; size >>= 1)
		levels++;
	return levels;
}
GR_HD uint64_t chain_offset(uint32_t size, uint32_t level, uint32_t face)
{
	uint64_t at = 0;
	for (uint32_t l = 0; l < level; l++)
	{
		const uint64_t n = level_size(size, l);
		at += 48u * n * n;
	}
	const uint64_t n = level_size(size, level);
	return at + 8u * n * n * face;
}

struct Cube
{
	const uint8_t *base;
	uint32_t size, levels;
};

// One level of a cube: faces `face_texels` texels apart.
struct CubeLevel
{
	const uint2 *texels;
	int n;
	uint32_t face_texels;
};
GR_HD CubeLevel cube_level(const Cube &c, uint32_t level)
{
	const uint32_t n = level_size(c.size, level);
	return {reinterpret_cast<const uint2 *>(c.base + chain_offset(c.size, level, 0)), int(n), n * n};
}
GR_HD f3 unpack_rgb(uint2 t) { return {half_to_float(t.x & 0xffffu), half_to_float(t.x >> 16), half_to_float(t.y & 0xffffu)}; }
GR_HD f3 load_texel(const CubeLevel &l, int face, int x, int y) { return unpack_rgb(l.texels[uint32_t(face) * l.face_texels + uint32_t(y * l.n + x)]); }
GR_HD uint2 pack_rgba(f3 c, float a) { return {float_to_half(c.x) | (float_to_half(c.y) << 16), float_to_half(c.z) | (float_to_half(a) << 16)}; }

// ---- cube addressing ---------------------------------------------------------------------------------------------------------
// Vulkan's table: major axis -> face, (sc, tc, |ma|).  Ties: Z over Y over X.
GR_HD int select_face(f3 d, float &sc, float &tc, float &ma)
{
	const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
	if (az >= ax && az >= ay)
	{
		ma = az;
		tc = -d.y;
		sc = d.z < 0.0f ? -d.x : d.x;
		return d.z < 0.0f ? 5 : 4;
	}
	if (ay >= ax)
	{
		ma = ay;
		sc = d.x;
		tc = d.y < 0.0f ? -d.z : d.z;
		return d.y < 0.0f ? 3 : 2;
	}
	ma = ax;
	tc = -d.y;
	sc = d.x < 0.0f ? d.z : -d.z;
	return d.x < 0.0f ? 1 : 0;
}
// The table read backwards: the direction through (sc, tc) on the plane |ma| = 1 of `face`.
GR_HD f3 face_direction(int face, float sc, float tc)
{
	switch (face)
	{
	case 0: return {1.0f, -tc, -sc};
	case 1: return {-1.0f, -tc, sc};
	case 2: return {sc, 1.0f, tc};
	case 3: return {sc, -1.0f, -tc};
	case 4: return {sc, -tc, 1.0f};
	default: return {-sc, -tc, -1.0f};
	}
}
// The direction the rasteriser gives texel (x, y) of `face` in an n x n viewport: inv = inverse(proj * look) of
// compute_cube_render_transform(0, face, 0.1, 100) (column major), applied to (ndc, 1, 1) as skybox.vert does; not normalised.
GR_HD f3 texel_direction(const float *inv, int n, int x, int y)
{
	const float px = (float(x) + 0.5f) / float(n) * 2.0f - 1.0f, py = (float(y) + 0.5f) / float(n) * 2.0f - 1.0f;
	return {inv[0] * px + inv[4] * py + inv[8] + inv[12], inv[1] * px + inv[5] * py + inv[9] + inv[13], inv[2] * px + inv[6] * py + inv[10] + inv[14]};
}

// A texel of the footprint: on the face it is read as it is, off the face through the direction of its centre.
GR_HD f3 footprint_texel(const CubeLevel &l, int face, int x, int y)
{
	if (uint32_t(x) < uint32_t(l.n) && uint32_t(y) < uint32_t(l.n))
		return load_texel(l, face, x, y);
	// (2 x + 1 - n) / n: the integer numerator keeps the two coordinates of a corner texel equal in magnitude, so that the tie between
	// the two neighbouring faces is a tie in fp32 as well (and goes Z over Y over X)
	const float fn = float(l.n);
	const f3 d = face_direction(face, float(2 * x + 1 - l.n) / fn, float(2 * y + 1 - l.n) / fn);
	float sc, tc, ma;
	const int other = select_face(d, sc, tc, ma);
	const float half_inv = 0.5f / ma;
	const int ox = clampi(int(floorf((sc * half_inv + 0.5f) * float(l.n))), 0, l.n - 1);
	const int oy = clampi(int(floorf((tc * half_inv + 0.5f) * float(l.n))), 0, l.n - 1);
	return load_texel(l, other, ox, oy);
}

GR_HD f3 sample_level(const CubeLevel &l, int face, float s, float t)
{
	int ix, iy;
	float a, b;
	linear_axis(s * float(l.n) - 0.5f, ix, a);
	linear_axis(t * float(l.n) - 0.5f, iy, b);
	f3 r = footprint_texel(l, face, ix, iy) * ((1.0f - a) * (1.0f - b));
	// a weight that snapped to 0 does not read its texel (0 * inf of an overflowed fp16 texel would be NaN)
	if (a != 0.0f)
		r = r + footprint_texel(l, face, ix + 1, iy) * (a * (1.0f - b));
	if (b != 0.0f)
	{
		r = r + footprint_texel(l, face, ix, iy + 1) * ((1.0f - a) * b);
		if (a != 0.0f)
			r = r + footprint_texel(l, face, ix + 1, iy + 1) * (a * b);
	}
	return r;
}

// TrilinearWrap.  level0 / level_weight come from trilinear_levels: they are the same for every tap of a launch's level.
struct LodPair
{
	uint32_t level0, level1;
	float weight; // of level1; 0 reads level0 alone
};
GR_HD LodPair trilinear_levels(float lod, uint32_t levels)
{
	const float top = float(levels - 1u);
	lod = lod < 0.0f ? 0.0f : (lod > top ? top : lod);
	int l0;
	float w;
	linear_axis(lod, l0, w);
	LodPair p;
	p.level0 = uint32_t(l0);
	p.level1 = p.level0 + 1u < levels ? p.level0 + 1u : levels - 1u;
	p.weight = p.level1 == p.level0 ? 0.0f : w;
	return p;
}
// LinearWrap (mipmap mode nearest): the level nearest to lod, Vulkan's ceil(lod + 0.5) - 1.
GR_HD uint32_t nearest_level(float lod, uint32_t levels)
{
	const float top = float(levels - 1u);
	lod = lod < 0.0f ? 0.0f : (lod > top ? top : lod);
	const int l = int(ceilf(lod + 0.5f)) - 1;
	return uint32_t(clampi(l, 0, int(levels) - 1));
}

GR_HD f3 sample_cube(const CubeLevel &l0, const CubeLevel &l1, float weight1, f3 dir)
{
	float sc, tc, ma;
	const int face = select_face(dir, sc, tc, ma);
	const float half_inv = 0.5f / ma;
	const float s = sc * half_inv + 0.5f, t = tc * half_inv + 0.5f;
	f3 r = sample_level(l0, face, s, t);
	if (weight1 != 0.0f)
		r = r * (1.0f - weight1) + sample_level(l1, face, s, t) * weight1;
	return r;
}

// ---- equirect -> cube level 0: skybox_latlon.frag with HAVE_EMISSIVE, colour (1, 1, 1), LinearWrap at LOD 0 --------------------------
struct Equirect
{
	const uint8_t *ptr;
	int w, h;
	uint32_t pitch;
};
GR_HD f3 equirect_texel(const Equirect &e, int x, int y)
{
	return unpack_rgb(*reinterpret_cast<const uint2 *>(e.ptr + size_t(wrapi(y, e.h)) * e.pitch + size_t(wrapi(x, e.w)) * 8u));
}
GR_HD f3 latlon(const Equirect &e, f3 direction)
{
	f3 v = normalize3(direction);
	if (fabsf(v.x) < 0.00001f)
		v.x = 0.00001f;
	const float u = atan2f(v.z, v.x) * 0.1591f + 0.5f, w = asinf(-v.y) * 0.3183f + 0.5f;
	int ix, iy;
	float a, b;
	linear_axis(u * float(e.w) - 0.5f, ix, a);
	linear_axis(w * float(e.h) - 0.5f, iy, b);
	f3 r = equirect_texel(e, ix, iy) * ((1.0f - a) * (1.0f - b));
	if (a != 0.0f)
		r = r + equirect_texel(e, ix + 1, iy) * (a * (1.0f - b));
	if (b != 0.0f)
	{
		r = r + equirect_texel(e, ix, iy + 1) * ((1.0f - a) * b);
		if (a != 0.0f)
			r = r + equirect_texel(e, ix + 1, iy + 1) * (a * b);
	}
	return r;
}

// ---- generate_mipmap: texel (x, y) of an n-texel face from the m-texel face above it, a linear-filter blit clamped to the face ---------
GR_HD void blit_texel(const uint2 *src, int m, int n, int x, int y, f3 &rgb, float &alpha)
{
	const float scale = float(m) / float(n);
	int ix, iy;
	float a, b;
	linear_axis((float(x) + 0.5f) * scale - 0.5f, ix, a);
	linear_axis((float(y) + 0.5f) * scale - 0.5f, iy, b);
	const int x0 = clampi(ix, 0, m - 1), x1 = clampi(ix + 1, 0, m - 1), y0 = clampi(iy, 0, m - 1), y1 = clampi(iy + 1, 0, m - 1);
	const uint2 t00 = src[y0 * m + x0], t10 = src[y0 * m + x1], t01 = src[y1 * m + x0], t11 = src[y1 * m + x1];
	const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
	rgb = unpack_rgb(t00) * w00;
	alpha = half_to_float(t00.y >> 16) * w00;
	if (a != 0.0f)
	{
		rgb = rgb + unpack_rgb(t10) * w10;
		alpha += half_to_float(t10.y >> 16) * w10;
	}
	if (b != 0.0f)
	{
		rgb = rgb + unpack_rgb(t01) * w01;
		alpha += half_to_float(t01.y >> 16) * w01;
		if (a != 0.0f)
		{
			rgb = rgb + unpack_rgb(t11) * w11;
			alpha += half_to_float(t11.y >> 16) * w11;
		}
	}
}

// ---- ibl_specular.frag -----------------------------------------------------------------------------------------------------------
GR_HD float radical_inverse(uint32_t bits)
{
	uint32_t r = 0;
	for (int i = 0; i < 32; i++)
		r |= ((bits >> i) & 1u) << (31 - i);
	return float(r) * 2.3283064365386963e-10f;
}
GR_HD float specular_roughness(uint32_t level, uint32_t levels)
{
	const float t = levels > 1u ? float(level) / float(levels - 1u) : 0.0f;
	return 0.001f * (1.0f - t) + 1.0f * t; // mix(0.001, 1, t)
}
struct SpecularSample
{
	float lx, ly, lz, ndotl; // L in the tangent frame of N; NdotL = max(L.z, 0)
};
// Sample i of the level: ImportanceSampleGGX and the reflection of V = N about H, in the frame (tangent, bitangent, N).  Nothing here
// depends on the texel, so a level's 1024 entries are computed once.
GR_HD SpecularSample specular_sample(uint32_t i, float roughness)
{
	const float xi_x = float(i) / float(SPECULAR_SAMPLES), xi_y = radical_inverse(i);
	const float a = roughness * roughness;
	const float phi = 2.0f * SHADER_PI * xi_x;
	const float cos_theta = sqrtf((1.0f - xi_y) / (1.0f + (a * a - 1.0f) * xi_y));
	const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
	const f3 h = normalize3(make3(cosf(phi) * sin_theta, sinf(phi) * sin_theta, cos_theta));
	const float two_vdoth = 2.0f * h.z;
	const f3 l = normalize3(make3(two_vdoth * h.x, two_vdoth * h.y, two_vdoth * h.z - 1.0f));
	return {l.x, l.y, l.z, l.z > 0.0f ? l.z : 0.0f};
}
struct Frame
{
	f3 tangent, bitangent, n;
};
GR_HD Frame specular_frame(f3 direction)
{
	Frame f;
	f.n = normalize3(direction);
	const f3 up = fabsf(f.n.z) < 0.999f ? make3(0.0f, 0.0f, 1.0f) : make3(1.0f, 0.0f, 0.0f);
	f.tangent = normalize3(cross3(up, f.n));
	f.bitangent = cross3(f.n, f.tangent);
	return f;
}
// Samples first, first + step, ... of `table` (SPECULAR_SAMPLES entries) added to (sum, weight).
GR_HD void specular_accumulate(const CubeLevel &l0, const CubeLevel &l1, float weight1, const Frame &f, const SpecularSample *table, uint32_t first, uint32_t step,
                                f3 &sum, float &weight)
{
	for (uint32_t i = first; i < SPECULAR_SAMPLES; i += step)
	{
		const SpecularSample s = table[i];
		if (s.ndotl > 0.0f)
		{
			const f3 dir = f.tangent * s.lx + f.bitangent * s.ly + f.n * s.lz;
			sum = sum + sample_cube(l0, l1, weight1, dir) * s.ndotl;
			weight += s.ndotl;
		}
	}
}

// ---- ibl_diffuse.frag ------------------------------------------------------------------------------------------------------------
// Entry k of the angle tables: the loop variable after k fp32 additions of sample_delta, as the shader's float loops step it.
GR_HD float diffuse_angle(uint32_t k)
{
	float angle = 0.0f;
	for (uint32_t i = 0; i < k; i++)
		angle += DIFFUSE_DELTA;
	return angle;
}
// How often `for (float a = 0; a < limit; a += sample_delta)` runs.
GR_HD uint32_t diffuse_steps(float limit)
{
	uint32_t n = 0;
	for (float a = 0.0f; a < limit; a += DIFFUSE_DELTA)
		n++;
	return n;
}
struct SinCos
{
	float s, c;
};
GR_HD Frame diffuse_frame(f3 direction)
{
	Frame f;
	f.n = normalize3(direction);
	f.tangent = cross3(make3(0.0f, 1.0f, 0.0f), f.n); // `right`: not normalised, as the shader has it
	f.bitangent = cross3(f.n, f.tangent);            // `up`
	return f;
}
// Taps first, first + step, ... of the 252 x 63 grid (phi outer, theta inner), phi[] and theta[] holding sin and cos of the angles.
GR_HD void diffuse_accumulate(const CubeLevel &l, const Frame &f, const SinCos *phi, const SinCos *theta, uint32_t first, uint32_t step, f3 &sum)
{
	for (uint32_t i = first; i < DIFFUSE_PHI_STEPS * DIFFUSE_THETA_STEPS; i += step)
	{
		const SinCos p = phi[i / DIFFUSE_THETA_STEPS], t = theta[i % DIFFUSE_THETA_STEPS];
		const f3 dir = f.tangent * (t.s * p.c) + f.bitangent * (t.s * p.s) + f.n * t.c;
		sum = sum + sample_cube(l, l, 0.0f, dir) * (t.c * t.s);
	}
}
GR_HD f3 diffuse_resolve(f3 sum) { return sum * SHADER_PI * (1.0f / float(DIFFUSE_PHI_STEPS * DIFFUSE_THETA_STEPS)); }
} // namespace gr_env
#include "host/math.hpp"
namespace gr_env
{
// Host only: inverse(proj * look) of compute_cube_render_transform(vec3(0), face, proj, look, 0.1, 100) (math/transforms.cpp) for the six
// faces, column major, with host/math.*: what skybox.vert multiplies the clip-space position by.
inline void face_inverse_matrices(float (*inv)[16])
{
	using namespace Granite;
	static const vec3 dirs[6] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
	static const vec3 ups[6] = {{0, 1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}, {0, 1, 0}, {0, 1, 0}};
	const mat4 proj = scale(vec3(-1.0f, 1.0f, 1.0f)) * perspective(0.5f * 3.14159265358979323846f, 1.0f, 0.1f, 100.0f);
	for (int face = 0; face < 6; face++)
	{
		const mat4 m = inverse(proj * mat4_cast(look_at(dirs[face], ups[face]))); // translate(-center) is the identity
		memcpy(inv[face], m.data(), 16 * sizeof(float));
	}
}
} // namespace gr_env
