// TEST INFRASTRUCTURE ONLY -- used by make_meshlet_cull_golden.py to record tests/golden/meshlet_cull_shader_v1.npz.
//
// Runs the reference's meshlet_cull.comp on the CPU, the way meshlet_decode_runner.cpp and ocean_lod_runner.cpp run theirs: re-spelled
// into gen/ by oracle/ref_build/glsl2cpp.py at generation time (a temporary directory, removed afterwards) and compiled as C++ against
// oracle/ref_build/glsl_cpu.hpp with -ffp-contract=off.  One object per specialisation set, one exported function each, named by
// -DCULL_FN; the set is -DMESHLET_RENDER_PHASE (the shader's own macro), -DSPEC_ORTHO, -DSPEC_SKINNED, -DSPEC_FORCE_VISIBLE.
// What glsl_cpu.hpp lacks is supplied here, each as the GLSL specification (4.60, chapter 8) states it:
//   findMSB(int)            for a negative value the most significant 0 bit; -1 for 0 and for -1 (the header has the uint form only, and
//                           the shader calls it with max_delta - 1 = -1 for a span of zero)
//   transpose(mat3)         columns become rows
//   texelFetch / texelFetchOffset over a mip chain: level l of a w x h chain is max(w >> l, 1) x max(h >> l, 1) R32_SFLOAT texels,
//                           levels tightly packed one after the other (gr_mip_chain_offset); a fetch outside its level reads 0 (robust
//                           access) -- the cases never do, which the runner counts and returns
//   barrier()               a std::barrier over the 32 invocations of the group, which run as 32 threads: the shader's ballot() is built
//                           from shared memory, atomicOr and three barriers
//   gl_WorkGroupSize        (32, 1, 1)
// Workgroups run one after the other, in order, so the order of tasks in the output is the order of the groups.
#include <barrier>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include "glsl_cpu.hpp"

namespace glsl
{
struct HizChain
{
	const float *data = nullptr;
	int w = 0, h = 0, levels = 0;
	mutable uint32_t outside = 0;
};
inline vec4 texelFetch(const HizChain &t, const ivec2 &p, int lod)
{
	size_t offset = 0;
	for (int l = 0; l < lod; l++)
		offset += size_t(std::max(t.w >> l, 1)) * size_t(std::max(t.h >> l, 1));
	const int w = std::max(t.w >> lod, 1), h = std::max(t.h >> lod, 1);
	if (lod < 0 || lod >= t.levels || p.x < 0 || p.y < 0 || p.x >= w || p.y >= h)
	{
		__atomic_fetch_add(&t.outside, 1u, __ATOMIC_SEQ_CST);
		return vec4(0.0f);
	}
	return vec4(t.data[offset + size_t(p.y) * w + p.x], 0.0f, 0.0f, 1.0f);
}
inline vec4 texelFetchOffset(const HizChain &t, const ivec2 &p, int lod, const ivec2 &o) { return texelFetch(t, ivec2(p.x + o.x, p.y + o.y), lod); }
inline int findMSB(int v)
{
	if (v == 0 || v == -1)
		return -1;
	return findMSB(uint(v < 0 ? ~v : v));
}
inline mat3 transpose(const mat3 &m) { return mat3(vec3(m.c[0].x, m.c[1].x, m.c[2].x), vec3(m.c[0].y, m.c[1].y, m.c[2].y), vec3(m.c[0].z, m.c[1].z, m.c[2].z)); }

namespace
{
// per object: the sixteen objects are linked into one library, where an inline barrier() would be merged into one that knows one team only
std::barrier<> *team_barrier;
void barrier() { team_barrier->arrive_and_wait(); }
const uvec3 gl_WorkGroupSize(32u, 1u, 1u);

namespace shader
{
#define texture2D HizChain
#include "gen/meshlet_cull.inc"
#undef texture2D
} // namespace shader
} // namespace
} // namespace glsl

using namespace glsl;

struct CullRun
{
	const void *tasks, *aabbs, *transforms, *bounds, *draws;
	uint32_t *occluders, *output;
	const float *chain;
	int32_t chain_width, chain_height, chain_levels;
	uint32_t push[4];
	float camera[3];
	uint32_t frustum[56];
};

// Returns the number of texel fetches that fell outside their level (0 for every stored case).
extern "C" uint32_t CULL_FN(const CullRun *run)
{
	namespace s = glsl::shader;
	static_assert(sizeof(s::MeshAssetDrawTaskInfo) == 20 && sizeof(s::AABB) == 32 && sizeof(s::Bound) == 32 && sizeof(s::mat_affine) == 48 && sizeof(s::Draw) == 12,
	              "std430 records");
	static_assert(sizeof(s::frustum) == 212, "the Frustum block's members are packed as std140 has them");
	s::task_info.data = static_cast<s::MeshAssetDrawTaskInfo *>(const_cast<void *>(run->tasks));
	s::aabb.data = static_cast<s::AABB *>(const_cast<void *>(run->aabbs));
	s::transforms.data = static_cast<s::mat_affine *>(const_cast<void *>(run->transforms));
	s::bounds.data = static_cast<s::Bound *>(const_cast<void *>(run->bounds));
	s::input_draws.draws = static_cast<s::Draw *>(const_cast<void *>(run->draws));
	s::output_draws.data = run->output;
#if MESHLET_RENDER_PHASE > 0
	s::occluders.data = run->occluders;
#endif
#if MESHLET_RENDER_PHASE == 2
	s::uHiZDepth = HizChain{run->chain, run->chain_width, run->chain_height, run->chain_levels, 0u};
#endif
	memcpy(static_cast<void *>(&s::frustum), run->frustum, sizeof(s::frustum));
	s::global.camera_position = vec3(run->camera[0], run->camera[1], run->camera[2]);
	s::registers.offset = run->push[0];
	s::registers.count = run->push[1];
	s::registers.mdi_count_offset = run->push[2];
	s::registers.draw_indirect_offset = run->push[3];

	const uint32_t groups = (run->push[1] + 31u) / 32u;
	for (uint32_t wg = 0; wg < groups; wg++)
	{
		std::barrier<> team(32);
		team_barrier = &team;
		std::vector<std::thread> threads;
		for (uint32_t lane = 0; lane < 32u; lane++)
			threads.emplace_back([wg, lane] {
				gl_WorkGroupID = uvec3(wg, 0u, 0u);
				gl_LocalInvocationID = uvec3(lane, 0u, 0u);
				gl_LocalInvocationIndex = lane;
				gl_GlobalInvocationID = uvec3(wg * 32u + lane, 0u, 0u);
				s::main();
			});
		for (auto &t : threads)
			t.join();
	}
#if MESHLET_RENDER_PHASE == 2
	return s::uHiZDepth.outside;
#else
	return 0u;
#endif
}
