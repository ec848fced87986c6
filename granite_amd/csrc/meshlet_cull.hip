// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Meshlet culling: assets/shaders/meshlet_cull.comp as one gfx950 kernel.  The per-lane decisions are meshlet_cull.hpp's; this file
// holds the launch shape, the compaction and the launcher's refusals.  Built with -ffp-contract=off (Makefile: EXACT_SRCS).
//
// Shape: one wave64 is the group; no LDS, no barrier.
//   1. 64 lanes test 64 task AABBs (and the phase's occluder rule); one __ballot is the work mask.
//   2. The wave walks the set bits two tasks a turn: the low half-wave takes the lower task, the high half the next, lane & 31 is the
//      chunk.  One 64-bit ballot holds both halves' 32-bit ballots.
//   3. Lane 0 adds both halves' survivor counts to the count word with one agent-scope atomic; a lane's slot is the base plus its rank
//      in the 64-bit ballot, so a task's records are contiguous and in lane order, the lower task's first.  Each survivor writes its
//      five dwords with ordinary stores.
// The shader's 32-lane group with an LDS ballot of three barriers orders tasks differently among each other, which its atomics leave
// unspecified anyway.
#include "ctx.hpp"
#include "meshlet_cull.hpp"

namespace
{
using namespace gr_cull;
constexpr uint32_t WAVE = 64u;

template <int PHASE, bool ORTHO, bool SKINNED, bool FORCE_VISIBLE> __global__ __launch_bounds__(WAVE) void k_meshlet_cull(const CullArgs a)
{
	const uint32_t lane = threadIdx.x, half = lane >> 5, sub = lane & 31u;
	const uint32_t group_base = blockIdx.x * WAVE;
	unsigned long long work = __ballot(task_needs_work<PHASE, ORTHO>(a, group_base + lane));

	while (work != 0ull)
	{
		const uint32_t first = uint32_t(__ffsll(work)) - 1u;
		work &= work - 1ull;
		uint32_t second = first;
		const bool two = work != 0ull;
		if (two)
		{
			second = uint32_t(__ffsll(work)) - 1u;
			work &= work - 1ull;
		}
		const bool active = half == 0u || two;
		const uint32_t task_index = a.offset + group_base + (half == 0u ? first : second); // below task_count: task_needs_work said so

		Task task = {};
		uint32_t old_state = 0u, chunk = 0u;
		bool alloc_draw = false;
		if (active)
		{
			task = a.tasks[task_index];
			if (PHASE >= 1)
				old_state = occluder_word(a, task.occluder_state_offset);
			alloc_draw = chunk_visible<PHASE, ORTHO, SKINNED>(a, task, sub, old_state, chunk);
		}
		unsigned long long draws = __ballot(alloc_draw);
		if (PHASE == 2)
		{
			// every chunk visible in this frame, before the FORCE_VISIBLE decision
			if (active && sub == 0u)
				set_occluder_word(a, task.occluder_state_offset, uint32_t(draws >> (32u * half)));
			if (!FORCE_VISIBLE)
			{
				// drawn in phase 1 already
				if ((old_state >> sub) & 1u)
					alloc_draw = false;
				draws = __ballot(alloc_draw);
			}
		}
		if (draws == 0ull)
			continue;
		uint32_t base = 0u;
		if (lane == 0u)
			base = __hip_atomic_fetch_add(&a.output[a.mdi_count_offset], uint32_t(__popcll(draws)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		base = uint32_t(__shfl(int(base), 0));
		if (alloc_draw)
			write_draw(a, base + uint32_t(__popcll(draws & ((1ull << lane) - 1ull))), chunk, task_index);
	}
}

bool misaligned(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) != 0u; }
} // namespace

extern "C" int gr_meshlet_cull(gr_ctx *ctx, gr_stream stream, const gr_meshlet_cull_args *args, const gr_push_meshlet_cull *push)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, args);
	GR_CHECK_ARG(ctx, push);
	if (args->phase > 2u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: phase %u is not 0, 1 or 2", args->phase);
	if (args->flags & ~(GR_MESHLET_CULL_ORTHO | GR_MESHLET_CULL_SKINNED | GR_MESHLET_CULL_FORCE_VISIBLE))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: flags 0x%x holds bits that are no cull flag", args->flags);
	if (push->count == 0u)
		return GR_OK;
	const bool skinned = (args->flags & GR_MESHLET_CULL_SKINNED) != 0u;
	const struct
	{
		const char *name;
		const void *ptr;
		uintptr_t align;
		bool required;
		const char *why;
	} pointers[] = {
	    {"tasks", args->tasks, 4, true, ""},
	    {"aabbs", args->aabbs, 16, true, ""},
	    {"transforms", args->transforms, 16, !skinned, " (needed unless SKINNED)"},
	    {"bounds", args->bounds, 16, !skinned, " (needed unless SKINNED)"},
	    {"draws", args->draws, 4, true, ""},
	    {"occluders", args->occluders, 4, args->phase >= 1u, " (phases 1 and 2 need the occluder words)"},
	    {"output", args->output, 4, true, ""},
	    {"chain", args->chain, 4, args->phase == 2u, " (phase 2 needs the HiZ chain)"},
	};
	for (const auto &p : pointers)
	{
		if (p.required && !p.ptr)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: %s is null%s", p.name, p.why);
		if (p.ptr && misaligned(p.ptr, p.align))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: %s is not %u-byte aligned", p.name, unsigned(p.align));
	}
	const gr_meshlet_frustum &f = args->frustum;
	if (args->phase == 2u)
	{
		if (args->chain_levels == 0u || args->chain_levels > 16u || args->chain_width == 0u || args->chain_height == 0u || args->chain_width > 32768u ||
		    args->chain_height > 32768u)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: chain %u x %u with %u levels is not 1 .. 32768 each way with 1 .. 16 levels", args->chain_width,
			                 args->chain_height, args->chain_levels);
		if (f.hiz_min_lod < 0 || f.hiz_min_lod > 8)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: frustum.hiz_min_lod %d is not 0 .. 8", f.hiz_min_lod);
		if (f.hiz_resolution[0] != int32_t(args->chain_width << f.hiz_min_lod) || f.hiz_resolution[1] != int32_t(args->chain_height << f.hiz_min_lod))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: frustum.hiz_resolution %d x %d is not the chain's %u x %u << hiz_min_lod %d", f.hiz_resolution[0],
			                 f.hiz_resolution[1], args->chain_width, args->chain_height, f.hiz_min_lod);
		if (f.hiz_max_lod != int32_t(args->chain_levels) - 1 + f.hiz_min_lod)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: frustum.hiz_max_lod %d is not chain_levels - 1 + hiz_min_lod = %d", f.hiz_max_lod,
			                 int32_t(args->chain_levels) - 1 + f.hiz_min_lod);
	}
	if (push->mdi_count_offset >= args->output_dwords)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: mdi_count_offset %u is outside output_dwords %llu", push->mdi_count_offset,
		                 static_cast<unsigned long long>(args->output_dwords));
	if (push->draw_indirect_offset >= args->output_dwords)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_cull: draw_indirect_offset %u is outside output_dwords %llu", push->draw_indirect_offset,
		                 static_cast<unsigned long long>(args->output_dwords));

	CullArgs a = {};
	a.tasks = reinterpret_cast<const Task *>(args->tasks);
	a.aabbs = reinterpret_cast<const AABB *>(args->aabbs);
	a.transforms = reinterpret_cast<const Affine *>(args->transforms);
	a.bounds = reinterpret_cast<const Bound *>(args->bounds);
	a.draws = reinterpret_cast<const Draw *>(args->draws);
	a.occluders = args->occluders;
	a.output = args->output;
	a.chain = static_cast<const float *>(args->chain);
	a.task_count = args->task_count;
	a.aabb_count = args->aabb_count;
	a.transform_count = args->transforms ? args->transform_count : 0u;
	a.bound_count = args->bounds ? args->bound_count : 0u;
	a.draw_count = args->draw_count;
	a.occluder_count = args->occluders ? args->occluder_count : 0u;
	a.output_dwords = args->output_dwords;
	a.chain_width = args->chain_width;
	a.chain_height = args->chain_height;
	a.chain_levels = args->chain_levels;
	a.offset = push->offset;
	a.count = push->count;
	a.mdi_count_offset = push->mdi_count_offset;
	a.draw_indirect_offset = push->draw_indirect_offset;
	memcpy(a.camera_position, args->camera_position, sizeof(a.camera_position));
	static_assert(sizeof(a.frustum) == sizeof(args->frustum), "the frustum block is the shader's");
	memcpy(&a.frustum, &args->frustum, sizeof(a.frustum));

	const dim3 grid(push->count / WAVE + (push->count % WAVE != 0u)), block(WAVE);
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "meshlet_cull"};
	const bool ortho = (args->flags & GR_MESHLET_CULL_ORTHO) != 0u, force = (args->flags & GR_MESHLET_CULL_FORCE_VISIBLE) != 0u;
	if (args->phase == 0u)
		with_flags([&](auto o, auto sk) { hipLaunchKernelGGL((k_meshlet_cull<0, decltype(o)::value, decltype(sk)::value, false>), grid, block, 0, s, a); }, ortho, skinned);
	else if (args->phase == 1u)
		with_flags([&](auto o, auto sk) { hipLaunchKernelGGL((k_meshlet_cull<1, decltype(o)::value, decltype(sk)::value, false>), grid, block, 0, s, a); }, ortho, skinned);
	else
		with_flags([&](auto o, auto sk, auto fv) { hipLaunchKernelGGL((k_meshlet_cull<2, decltype(o)::value, decltype(sk)::value, decltype(fv)::value>), grid, block, 0, s, a); },
		           ortho, skinned, force);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
