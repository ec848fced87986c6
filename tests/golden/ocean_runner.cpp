// TEST INFRASTRUCTURE ONLY -- used by make_ocean_golden.py to record tests/golden/ocean_shader_v1.npz.
//
// Runs the reference's ocean/generate_fft.comp, ocean/bake_maps.comp and ocean/mipmap.comp on the CPU: the shaders are re-spelled into
// gen/ by oracle/ref_build/glsl2cpp.py at generation time (a temporary directory, removed afterwards) and compiled as C++ against
// oracle/ref_build/glsl_cpu.hpp with -ffp-contract=off.  Each object built from this file holds one shader with one set of #defines
// and exports one function, named by -DOCEAN_FN:
//   -DOCEAN_GENERATE  -DFREQ_BAND_MODULATION=0|1  [-DGRADIENT_NORMAL | -DGRADIENT_DISPLACEMENT]
//   -DOCEAN_BAKE      -DVERTEX_TEXTURE=0|1
//   -DOCEAN_MIPMAP    -DMIPMAP_R16F | -DMIPMAP_RG16F | -DMIPMAP_RGBA16F
// glsl_cpu.hpp's Texture clamps and its imageStore knows no RG16F; the ocean samples LinearWrap, so this file supplies a wrapping
// texture, an fp16 storage image and their textureLod / textureLodOffset / imageStore.  The sampling follows the model of DESIGN.md
// 7.10: linear_axis per axis, linear_combine of the four texels, indices (offset included) modulo the size.  One invocation per bin
// or texel, edge groups included, gl_GlobalInvocationID set per invocation.
#include <cstddef>
#include <cstdint>
#include "glsl_cpu.hpp"

namespace glsl
{
struct WrapTexture
{
	const uint16_t *data = nullptr;
	int w = 0, h = 0, channels = 1;
	vec4 texel(int x, int y) const
	{
		x = ((x % w) + w) % w;
		y = ((y % h) + h) % h;
		const uint16_t *p = data + (size_t(y) * w + x) * channels;
		vec4 r(0.0f, 0.0f, 0.0f, 1.0f);
		for (int c = 0; c < channels; c++)
			r.d[c] = orc::half_to_float(p[c]);
		return r;
	}
};
inline vec4 textureLodOffset(const WrapTexture &t, const vec2 &uv, float, const ivec2 &o)
{
	int x0, y0;
	float a, b;
	orc::linear_axis(uv.x * float(t.w) - 0.5f, x0, a);
	orc::linear_axis(uv.y * float(t.h) - 0.5f, y0, b);
	x0 += o.x;
	y0 += o.y;
	return orc::linear_combine(t.texel(x0, y0), t.texel(x0 + 1, y0), t.texel(x0, y0 + 1), t.texel(x0 + 1, y0 + 1), a, b);
}
inline vec4 textureLod(const WrapTexture &t, const vec2 &uv, float lod) { return textureLodOffset(t, uv, lod, ivec2(0, 0)); }

// ... and its imageStore writes no RG16F image: an fp16 image of 1, 2 or 4 channels, stores outside it dropped
struct HalfImage
{
	uint16_t *data = nullptr;
	int w = 0, h = 0, channels = 1;
};
inline void imageStore(HalfImage &img, const ivec2 &p, const vec4 &v)
{
	if (p.x < 0 || p.y < 0 || p.x >= img.w || p.y >= img.h)
		return;
	for (int c = 0; c < img.channels; c++)
		img.data[(size_t(p.y) * img.w + p.x) * img.channels + c] = orc::float_to_half_rne(v.d[c]);
}

// what the shaders use and the header has no spelling for
inline vec2 operator*(float s, const uvec2 &v) { return vec2(s * float(v.x), s * float(v.y)); }

namespace // every object holds its own shader
{
namespace shader
{
#define sampler2D WrapTexture
#define image2D HalfImage
#if defined(OCEAN_GENERATE)
#include "gen/generate_fft.inc"
#elif defined(OCEAN_BAKE)
#include "gen/bake_maps.inc"
#elif defined(OCEAN_MIPMAP)
#include "gen/mipmap.inc"
#endif
#undef sampler2D
#undef image2D
} // namespace shader
} // namespace
} // namespace glsl

using namespace glsl;

#if defined(OCEAN_GENERATE)
// push: the 7 dwords of the Registers block; bands: 8 floats (read only by the FREQ_BAND_MODULATION objects)
extern "C" void OCEAN_FN(const float *distribution, uint32_t *out, const void *push, const float *bands)
{
	namespace s = glsl::shader;
	const float *pf = static_cast<const float *>(push);
	const uint32_t *pu = static_cast<const uint32_t *>(push);
	s::registers.mod_factor = vec2(pf[0], pf[1]);
	s::registers.N = uvec2(pu[2], pu[3]);
	s::registers.freq_to_band_mod = pf[4];
	s::registers.time = pf[5];
	s::registers.period = pf[6];
	s::distribution = reinterpret_cast<vec2 *>(const_cast<float *>(distribution));
	s::fft_input = out;
#if FREQ_BAND_MODULATION
	for (int i = 0; i < 2; i++)
		s::freq_bands[i] = vec4(bands[4 * i], bands[4 * i + 1], bands[4 * i + 2], bands[4 * i + 3]);
#else
	(void)bands;
#endif
	for (uint32_t y = 0; y < pu[3]; y++)
		for (uint32_t x = 0; x < pu[2]; x++) // N.x / 64 groups of 64 a row
		{
			gl_GlobalInvocationID = uvec3(x, y, 0u);
			s::main();
		}
}
#elif defined(OCEAN_BAKE)
// Tightly packed images; push: inv_size[4], scale[4].  height_displacement is written by the VERTEX_TEXTURE = 1 object only.
extern "C" void OCEAN_FN(const uint16_t *height, int w, int h, const uint16_t *displacement, int dw, int dh, const float *push, uint16_t *grad_jacobian,
                         uint16_t *height_displacement)
{
	namespace s = glsl::shader;
	s::registers.inv_size = vec4(push[0], push[1], push[2], push[3]);
	s::registers.scale = vec4(push[4], push[5], push[6], push[7]);
	s::uHeight = {height, w, h, 1};
	s::uDisplacement = {displacement, dw, dh, 2};
	s::iGradJacobian = {grad_jacobian, w, h, 4};
#if VERTEX_TEXTURE
	s::iHeightDisplacement = {height_displacement, w, h, 4};
#else
	(void)height_displacement;
#endif
	for (int y = 0; y < (h + 7) / 8 * 8; y++)
		for (int x = 0; x < (w + 7) / 8 * 8; x++)
		{
			gl_GlobalInvocationID = uvec3(uint(x), uint(y), 0u);
			s::main();
		}
}
#elif defined(OCEAN_MIPMAP)
// push: result_mod[4], inv_resolution[2], count[2], lod
extern "C" void OCEAN_FN(const uint16_t *in, int w, int h, const void *push, uint16_t *out)
{
	namespace s = glsl::shader;
	const float *pf = static_cast<const float *>(push);
	const uint32_t *pu = static_cast<const uint32_t *>(push);
#if defined(MIPMAP_R16F)
	const int channels = 1;
#elif defined(MIPMAP_RG16F)
	const int channels = 2;
#else
	const int channels = 4;
#endif
	s::registers.result_mod = vec4(pf[0], pf[1], pf[2], pf[3]);
	s::registers.inv_resolution = vec2(pf[4], pf[5]);
	s::registers.count = uvec2(pu[6], pu[7]);
	s::registers.lod = pf[8];
	s::uInput = {in, w, h, channels};
	s::uImageOutput = {out, int(pu[6]), int(pu[7]), channels};
	for (uint32_t y = 0; y < (pu[7] + 7) / 8 * 8; y++)
		for (uint32_t x = 0; x < (pu[6] + 7) / 8 * 8; x++)
		{
			gl_GlobalInvocationID = uvec3(x, y, 0u);
			s::main();
		}
}
#endif
