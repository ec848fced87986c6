// TEST INFRASTRUCTURE ONLY -- used by make_ocean_lod_golden.py to record tests/golden/ocean_lod_shader_v1.npz.
//
// Runs the reference's ocean/update_lod.comp, ocean/init_counter_buffer.comp and ocean/cull_blocks.comp on the CPU, the way
// ocean_runner.cpp runs the FFT update's shaders: re-spelled into gen/ by oracle/ref_build/glsl2cpp.py at generation time (a temporary
// directory, removed afterwards) and compiled as C++ against oracle/ref_build/glsl_cpu.hpp with -ffp-contract=off.  One object per
// shader, one exported function each, named by -DOCEAN_FN:
//   -DOCEAN_UPDATE_LOD   -DOCEAN_INIT_COUNTERS   -DOCEAN_CULL
// What glsl_cpu.hpp lacks is supplied here: a nearest sampler over an R16F image with wrap or clamp addressing (the reference picks
// NearestWrap or NearestClamp on the host) with its textureLod / textureLodOffset, and mix on four-vectors with a boolean selector (atomicAdd, the R16F
// imageStore and equal on four-vectors are the header's).  The sampler takes the float route: texel floor(uv * size) + offset, then wrapped or clamped.
// One invocation per lane of every 8 x 8 group, edge groups included, in row order.
#include <cstddef>
#include <cstdint>
#include "glsl_cpu.hpp"

namespace glsl
{
struct NearestTexture
{
	const uint16_t *data = nullptr;
	int w = 0, h = 0;
	bool wrap = true;
	int address(int i, int size) const { return wrap ? ((i % size) + size) % size : (i < 0 ? 0 : (i >= size ? size - 1 : i)); }
};
inline vec4 textureLodOffset(const NearestTexture &t, const vec2 &uv, float, const ivec2 &o)
{
	const int x = t.address(int(floorf(uv.x * float(t.w))) + o.x, t.w), y = t.address(int(floorf(uv.y * float(t.h))) + o.y, t.h);
	return vec4(orc::half_to_float(t.data[size_t(y) * t.w + x]), 0.0f, 0.0f, 1.0f);
}
inline vec4 textureLod(const NearestTexture &t, const vec2 &uv, float lod) { return textureLodOffset(t, uv, lod, ivec2(0, 0)); }

inline vec4 mix(const vec4 &a, const vec4 &b, const bvec4 &t) { return vec4(t.x ? b.x : a.x, t.y ? b.y : a.y, t.z ? b.z : a.z, t.w ? b.w : a.w); }

namespace
{
namespace shader
{
#define sampler2D NearestTexture
#if defined(OCEAN_UPDATE_LOD)
#include "gen/update_lod.inc"
#elif defined(OCEAN_INIT_COUNTERS)
#include "gen/init_counter_buffer.inc"
#elif defined(OCEAN_CULL)
#include "gen/cull_blocks.inc"
#endif
#undef sampler2D
} // namespace shader
} // namespace
} // namespace glsl

using namespace glsl;

#if defined(OCEAN_UPDATE_LOD)
// push: the 16 dwords of gr_push_ocean_update_lod; image: n x n R16F, tightly packed
extern "C" void OCEAN_FN(const void *push, uint16_t *image, int n)
{
	namespace s = glsl::shader;
	const float *pf = static_cast<const float *>(push);
	const int32_t *pi = static_cast<const int32_t *>(push);
	s::registers.shifted_camera_pos = vec3(pf[0], pf[1], pf[2]);
	s::registers.max_lod = pf[3];
	s::registers.image_offset = ivec2(pi[4], pi[5]);
	s::registers.num_threads = ivec2(pi[6], pi[7]);
	s::registers.grid_base = vec2(pf[8], pf[9]);
	s::registers.grid_size = vec2(pf[10], pf[11]);
	s::registers.lod_bias = pf[12];
	s::uLODs.data = image;
	s::uLODs.w = s::uLODs.h = n;
	s::uLODs.format = Format::R16F;
	for (int y = 0; y < (n + 7) / 8 * 8; y++)
		for (int x = 0; x < (n + 7) / 8 * 8; x++)
		{
			gl_GlobalInvocationID = uvec3(uint(x), uint(y), 0u);
			s::main();
		}
}
#elif defined(OCEAN_INIT_COUNTERS)
// counts16: the uniform block's sixteen dwords; draws: 8 records of 8 dwords
extern "C" void OCEAN_FN(const uint32_t *counts16, uint32_t *draws)
{
	namespace s = glsl::shader;
	for (int i = 0; i < 4; i++)
		s::counts[i] = uvec4(counts16[4 * i], counts16[4 * i + 1], counts16[4 * i + 2], counts16[4 * i + 3]);
	static_assert(sizeof(s::IndirectDraw) == 32, "IndirectDraw is eight dwords");
	s::draws = reinterpret_cast<s::IndirectDraw *>(draws);
	for (uint x = 0; x < 8u; x++) // local_size_x = NUM_COUNTERS = 8, one group
	{
		gl_GlobalInvocationID = uvec3(x, 0u, 0u);
		s::main();
	}
}
#elif defined(OCEAN_CULL)
// push: the 24 dwords of gr_push_ocean_cull; frustum: 24 floats; lod: n x n R16F; patches: lod_stride * 8 records of 8 floats
extern "C" void OCEAN_FN(const void *push, const float *frustum, const uint16_t *lod, int n, int wrap, float *patches, uint32_t *draws)
{
	namespace s = glsl::shader;
	const float *pf = static_cast<const float *>(push);
	const int32_t *pi = static_cast<const int32_t *>(push);
	const uint32_t *pu = static_cast<const uint32_t *>(push);
	s::registers.world_offset = vec3(pf[0], pf[1], pf[2]);
	s::registers.image_offset = ivec2(pi[4], pi[5]);
	s::registers.num_threads = uvec2(pu[6], pu[7]);
	s::registers.inv_num_threads = vec2(pf[8], pf[9]);
	s::registers.grid_base = vec2(pf[10], pf[11]);
	s::registers.grid_size = vec2(pf[12], pf[13]);
	s::registers.grid_resolution = vec2(pf[14], pf[15]);
	s::registers.heightmap_range = vec2(pf[16], pf[17]);
	s::registers.guard_band = pf[18];
	s::registers.lod_stride = pu[19];
	s::registers.max_lod = pf[20];
	s::registers.handle_edge_lods = pi[21];
	for (int i = 0; i < 6; i++)
		s::frustum[i] = vec4(frustum[4 * i], frustum[4 * i + 1], frustum[4 * i + 2], frustum[4 * i + 3]);
	static_assert(sizeof(s::PatchData) == 32 && sizeof(s::IndirectDraw) == 32, "ocean.inc's records are eight dwords");
	s::patches = reinterpret_cast<s::PatchData *>(patches);
	s::draws = reinterpret_cast<s::IndirectDraw *>(draws);
	s::uLODs = {lod, n, n, wrap != 0};
	for (int y = 0; y < (n + 7) / 8 * 8; y++)
		for (int x = 0; x < (n + 7) / 8 * 8; x++)
		{
			gl_GlobalInvocationID = uvec3(uint(x), uint(y), 0u);
			s::main();
		}
}
#endif
