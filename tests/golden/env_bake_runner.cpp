// TEST INFRASTRUCTURE ONLY -- used by make_env_bake_golden.py to record tests/golden/env_bake_shader_v1.npz.
//
// Runs the reference's skybox_latlon.frag (HAVE_EMISSIVE), util/ibl_specular.frag and util/ibl_diffuse.frag on the CPU, one invocation
// per texel of every face (and level), with vDirection as skybox.vert gives it at the pixel centre.  The shaders are re-spelled into
// gen/ by oracle/ref_build/glsl2cpp.py at generation time (a temporary directory, removed afterwards) and compiled as C++ against
// oracle/ref_build/glsl_cpu.hpp.  This file supplies what that header lacks: a samplerCube (the cube sampling model of DESIGN.md 7.8,
// written here from the Vulkan face table as basis vectors, not from csrc/env_core.hpp), a sampler2D with wrap addressing,
// bitfieldReverse, asin and the two-argument atan; and the linear blit of generate_mipmap, which is no shader in the reference.
//
// The object built with -DENV_MATRICES holds nothing but the per-face inverse(proj * look) of the reference's own
// compute_cube_render_transform (math/transforms.cpp, compiled from where it lies into the same temporary directory).
#include <cstddef>
#include <cstdint>

#ifdef ENV_MATRICES
#include "transforms.hpp"
#include "muglm/matrix_helper.hpp"
#include "muglm/muglm_impl.hpp"
#include <cstring>

extern "C" void ref_env_matrices(float *out)
{
	using namespace muglm;
	for (unsigned face = 0; face < 6; face++)
	{
		mat4 look, proj;
		Granite::compute_cube_render_transform(vec3(0.0f), face, proj, look, 0.1f, 100.0f);
		const mat4 inv = inverse(proj * look);
		for (int c = 0; c < 4; c++)
			for (int r = 0; r < 4; r++)
				out[face * 16 + c * 4 + r] = inv[c][r];
	}
}
#else
#include "glsl_cpu.hpp"

namespace glsl
{
// ---- the cube: an RGBA16F chain, levels in order, six faces a level, rows tightly packed ---------------------------------------
struct samplerCube
{
	const uint16_t *data = nullptr;
	int size = 0, levels = 0;
	bool trilinear = false; // TrilinearWrap, else LinearWrap (mipmap mode nearest)
};

namespace cube
{
inline int extent(const samplerCube &c, int level) { return (c.size >> level) > 0 ? (c.size >> level) : 1; }
inline const uint16_t *level_data(const samplerCube &c, int level)
{
	size_t at = 0;
	for (int l = 0; l < level; l++)
		at += size_t(6) * extent(c, l) * extent(c, l) * 4;
	return c.data + at;
}
// The Vulkan face table as bases: a direction on face f is major + sc * u_axis + tc * v_axis (|ma| = 1).
struct Basis
{
	vec3 major, u_axis, v_axis;
};
inline Basis basis(int face)
{
	switch (face)
	{
	case 0: return {vec3(1, 0, 0), vec3(0, 0, -1), vec3(0, -1, 0)};
	case 1: return {vec3(-1, 0, 0), vec3(0, 0, 1), vec3(0, -1, 0)};
	case 2: return {vec3(0, 1, 0), vec3(1, 0, 0), vec3(0, 0, 1)};
	case 3: return {vec3(0, -1, 0), vec3(1, 0, 0), vec3(0, 0, -1)};
	case 4: return {vec3(0, 0, 1), vec3(1, 0, 0), vec3(0, -1, 0)};
	default: return {vec3(0, 0, -1), vec3(-1, 0, 0), vec3(0, -1, 0)};
	}
}
// largest magnitude wins; on ties Z, then Y, then X
inline int face_of(const vec3 &d)
{
	const float mx = fabsf(d.x), my = fabsf(d.y), mz = fabsf(d.z);
	int axis = 2;
	float best = mz;
	if (my > best)
	{
		axis = 1;
		best = my;
	}
	if (mx > best)
		axis = 0;
	const float v = axis == 0 ? d.x : axis == 1 ? d.y : d.z;
	return 2 * axis + (v < 0.0f ? 1 : 0);
}
inline vec2 face_st(int face, const vec3 &d)
{
	const Basis b = basis(face);
	const float ma = fabsf(dot(d, b.major));
	return vec2(0.5f * dot(d, b.u_axis) / ma + 0.5f, 0.5f * dot(d, b.v_axis) / ma + 0.5f);
}
inline vec3 texel(const samplerCube &c, int level, int face, int x, int y)
{
	const int n = extent(c, level);
	const uint16_t *p = level_data(c, level) + ((size_t(face) * n + y) * n + x) * 4;
	return vec3(orc::half_to_float(p[0]), orc::half_to_float(p[1]), orc::half_to_float(p[2]));
}
// seamless: a texel off the face is the nearest texel along the direction of its centre
inline vec3 texel_seamless(const samplerCube &c, int level, int face, int x, int y)
{
	const int n = extent(c, level);
	if (x >= 0 && y >= 0 && x < n && y < n)
		return texel(c, level, face, x, y);
	const Basis b = basis(face);
	// (2 x + 1 - n) / n: the integer numerator keeps a corner's two coordinates equal in magnitude, so the tie there is a tie
	const float sc = float(2 * x + 1 - n) / float(n), tc = float(2 * y + 1 - n) / float(n);
	const vec3 d = b.major + b.u_axis * sc + b.v_axis * tc;
	const int other = face_of(d);
	const vec2 st = face_st(other, d);
	return texel(c, level, other, orc::clampi(int(floorf(st.x * float(n))), 0, n - 1), orc::clampi(int(floorf(st.y * float(n))), 0, n - 1));
}
inline vec3 bilinear(const samplerCube &c, int level, const vec3 &d)
{
	const int n = extent(c, level), face = face_of(d);
	const vec2 st = face_st(face, d);
	int x0, y0;
	float a, b;
	orc::linear_axis(st.x * float(n) - 0.5f, x0, a);
	orc::linear_axis(st.y * float(n) - 0.5f, y0, b);
	// a weight of exactly 0 does not read its texel (linear_combine does not use it then)
	const vec3 t00 = texel_seamless(c, level, face, x0, y0);
	const vec3 t10 = a == 0.0f ? t00 : texel_seamless(c, level, face, x0 + 1, y0);
	const vec3 t01 = b == 0.0f ? t00 : texel_seamless(c, level, face, x0, y0 + 1);
	const vec3 t11 = (a == 0.0f || b == 0.0f) ? t00 : texel_seamless(c, level, face, x0 + 1, y0 + 1);
	return orc::linear_combine(t00, t10, t01, t11, a, b);
}
} // namespace cube

inline vec4 textureLod(const samplerCube &c, const vec3 &d, float lod)
{
	const float top = float(c.levels - 1);
	lod = lod < 0.0f ? 0.0f : (lod > top ? top : lod);
	if (!c.trilinear)
		return vec4(cube::bilinear(c, orc::clampi(int(ceilf(lod + 0.5f)) - 1, 0, c.levels - 1), d), 1.0f);
	int l0;
	float w;
	orc::linear_axis(lod, l0, w);
	const vec3 lo = cube::bilinear(c, l0, d);
	if (w == 0.0f || l0 + 1 >= c.levels)
		return vec4(lo, 1.0f);
	return vec4(lo * (1.0f - w) + cube::bilinear(c, l0 + 1, d) * w, 1.0f);
}

// ---- LinearWrap over an RGBA16F image -----------------------------------------------------------------------------------------------
struct WrapTexture
{
	const uint16_t *data = nullptr;
	int w = 0, h = 0;
	vec4 texel(int x, int y) const
	{
		x = ((x % w) + w) % w;
		y = ((y % h) + h) % h;
		const uint16_t *p = data + (size_t(y) * w + x) * 4;
		return vec4(orc::half_to_float(p[0]), orc::half_to_float(p[1]), orc::half_to_float(p[2]), orc::half_to_float(p[3]));
	}
};
inline vec4 textureLod(const WrapTexture &t, const vec2 &uv, float)
{
	int x0, y0;
	float a, b;
	orc::linear_axis(uv.x * float(t.w) - 0.5f, x0, a);
	orc::linear_axis(uv.y * float(t.h) - 0.5f, y0, b);
	return orc::linear_combine(t.texel(x0, y0), t.texel(x0 + 1, y0), t.texel(x0, y0 + 1), t.texel(x0 + 1, y0 + 1), a, b);
}

inline uint bitfieldReverse(uint v)
{
	uint r = 0;
	for (int i = 0; i < 32; i++)
		r |= ((v >> i) & 1u) << (31 - i);
	return r;
}
inline float atan(float y, float x) { return atan2f(y, x); }
inline float asin(float v) { return asinf(v); }

namespace latlon
{
#define sampler2D WrapTexture
#define HAVE_EMISSIVE 1
#include "gen/skybox_latlon.inc"
#undef sampler2D
} // namespace latlon
namespace specular
{
#include "gen/ibl_specular.inc"
}
namespace diffuse
{
#include "gen/ibl_diffuse.inc"
}
} // namespace glsl

namespace
{
using namespace glsl;

int extent(int size, int level) { return (size >> level) > 0 ? (size >> level) : 1; }
size_t level_halfs(int size, int level)
{
	size_t at = 0;
	for (int l = 0; l < level; l++)
		at += size_t(6) * extent(size, l) * extent(size, l) * 4;
	return at;
}
// skybox.vert: (inv_local_view_projection * vec4(Position, 1, 1)).xyz at the centre of pixel (x, y) of an n x n viewport
vec3 direction(const float *inv, int n, int x, int y)
{
	const float px = (float(x) + 0.5f) / float(n) * 2.0f - 1.0f, py = (float(y) + 0.5f) / float(n) * 2.0f - 1.0f;
	const vec4 c0(inv[0], inv[1], inv[2], inv[3]), c1(inv[4], inv[5], inv[6], inv[7]), c2(inv[8], inv[9], inv[10], inv[11]), c3(inv[12], inv[13], inv[14], inv[15]);
	const vec4 r = c0 * px + c1 * py + c2 * 1.0f + c3 * 1.0f;
	return vec3(r.x, r.y, r.z);
}
void store(uint16_t *out, const vec4 &v)
{
	for (int c = 0; c < 4; c++)
		out[c] = orc::float_to_half_rne(v.d[c]);
}
} // namespace

// matrices: 6 x 16 floats, column major.  Every cube is a chain as described above, in fp16 bits.
extern "C" void ref_env_equirect_to_cube(const float *matrices, const uint16_t *equirect, int w, int h, uint16_t *cube, int size, int levels)
{
	latlon::uSkybox.data = equirect;
	latlon::uSkybox.w = w;
	latlon::uSkybox.h = h;
	latlon::registers.color = vec3(1.0f, 1.0f, 1.0f);
	for (int face = 0; face < 6; face++)
		for (int y = 0; y < size; y++)
			for (int x = 0; x < size; x++)
			{
				latlon::vDirection = direction(matrices + 16 * face, size, x, y);
				latlon::main();
				store(cube + ((size_t(face) * size + y) * size + x) * 4, vec4(latlon::Emissive, 1.0f));
			}
	// generate_mipmap: a linear-filter blit per face and level, the destination texel centre scaled by src / dst, clamped to the face
	for (int level = 1; level < levels; level++)
	{
		const int m = extent(size, level - 1), n = extent(size, level);
		for (int face = 0; face < 6; face++)
		{
			Texture src;
			src.data = cube + level_halfs(size, level - 1) + size_t(face) * m * m * 4;
			src.w = src.h = m;
			src.format = Format::RGBA16F;
			for (int y = 0; y < n; y++)
				for (int x = 0; x < n; x++)
					store(cube + level_halfs(size, level) + ((size_t(face) * n + y) * n + x) * 4, src.sample(vec2((float(x) + 0.5f) / float(n), (float(y) + 0.5f) / float(n))));
		}
	}
}

extern "C" void ref_env_specular(const float *matrices, const uint16_t *src, int src_size, int src_levels, uint16_t *out, int out_size, int out_levels)
{
	specular::uCube.data = src;
	specular::uCube.size = src_size;
	specular::uCube.levels = src_levels;
	specular::uCube.trilinear = true;
	const float base_lod = log2f(float(src_size)) - log2f(float(out_size));
	for (int level = 0; level < out_levels; level++)
	{
		const int n = extent(out_size, level);
		const float t = float(level) / float(out_levels - 1);
		specular::registers.lod = base_lod + float(level);
		specular::registers.roughness = 0.001f * (1.0f - t) + 1.0f * t;
		for (int face = 0; face < 6; face++)
			for (int y = 0; y < n; y++)
				for (int x = 0; x < n; x++)
				{
					specular::vDirection = direction(matrices + 16 * face, n, x, y);
					specular::main();
					store(out + level_halfs(out_size, level) + ((size_t(face) * n + y) * n + x) * 4, specular::FragColor);
				}
	}
}

extern "C" void ref_env_diffuse(const float *matrices, const uint16_t *src, int src_size, int src_levels, uint16_t *out, int out_size)
{
	diffuse::uCube.data = src;
	diffuse::uCube.size = src_size;
	diffuse::uCube.levels = src_levels;
	diffuse::uCube.trilinear = false;
	const float lod = log2f(float(out_size)) - 5.0f;
	diffuse::registers.lod = lod > 0.0f ? lod : 0.0f;
	for (int face = 0; face < 6; face++)
		for (int y = 0; y < out_size; y++)
			for (int x = 0; x < out_size; x++)
			{
				diffuse::vDirection = direction(matrices + 16 * face, out_size, x, y);
				diffuse::main();
				store(out + ((size_t(face) * out_size + y) * out_size + x) * 4, diffuse::FragColor);
			}
}
#endif
