// TEST INFRASTRUCTURE.  The per-lane decisions of granite_amd/csrc/meshlet_cull.hpp -- what k_meshlet_cull calls -- built for the host
// (g++ -ffp-contract=off) as a stand-alone program, so that it also runs under -fsanitize=address,undefined.
// tests/test_meshlet_cull_core_cpu.py holds it to the golden of the executed shader (tests/golden/meshlet_cull_shader_v1.npz) before a
// device sees the code.
//
//   meshlet_cull_core_host <case file>
// case file, dwords: phase, flags, tasks, aabbs, transforms, chunks, occluder words, output dwords, chain floats, chain width, height,
// levels, dispatches; camera[3]; frustum[56]; dispatches x {offset, count, mdi_count_offset, draw_indirect_offset}; then the arrays in
// that order (tasks, aabbs, transforms, bounds, draws, occluders, output, chain).  stdout: the output buffer, then the occluder words.
// The walk follows k_meshlet_cull: groups of 64 tasks one after the other, the set bits two a turn, the lower task's survivors first.
#include "../../granite_amd/csrc/meshlet_cull.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace gr_cull;

static void get(void *data, size_t bytes, FILE *f)
{
	if (bytes && fread(data, 1, bytes, f) != bytes)
	{
		fprintf(stderr, "meshlet_cull_core_host: short case file\n");
		exit(3);
	}
}
static void put(const void *data, size_t bytes)
{
	if (bytes && fwrite(data, 1, bytes, stdout) != bytes)
		exit(3);
}

template <int PHASE, bool ORTHO, bool SKINNED> static void dispatch(const CullArgs &a, bool force_visible)
{
	for (uint32_t group_base = 0; group_base < a.count; group_base += 64u)
	{
		uint64_t work = 0;
		for (uint32_t lane = 0; lane < 64u; lane++)
			if (task_needs_work<PHASE, ORTHO>(a, group_base + lane))
				work |= uint64_t(1) << lane;
		while (work)
		{
			uint32_t bit[2], halves = 0;
			for (; halves < 2u && work; halves++)
			{
				bit[halves] = uint32_t(__builtin_ctzll(work));
				work &= work - 1u;
			}
			bool alloc[64] = {};
			uint32_t chunk[64] = {}, task_of[64] = {};
			for (uint32_t half = 0; half < halves; half++)
			{
				const uint32_t task_index = a.offset + group_base + bit[half];
				const Task task = a.tasks[task_index];
				const uint32_t old_state = PHASE >= 1 ? occluder_word(a, task.occluder_state_offset) : 0u;
				uint32_t visible = 0;
				for (uint32_t sub = 0; sub < 32u; sub++)
				{
					const uint32_t lane = 32u * half + sub;
					task_of[lane] = task_index;
					alloc[lane] = chunk_visible<PHASE, ORTHO, SKINNED>(a, task, sub, old_state, chunk[lane]);
					visible |= uint32_t(alloc[lane]) << sub;
				}
				if (PHASE == 2)
				{
					set_occluder_word(a, task.occluder_state_offset, visible);
					if (!force_visible)
						for (uint32_t sub = 0; sub < 32u; sub++)
							if ((old_state >> sub) & 1u)
								alloc[32u * half + sub] = false;
				}
			}
			uint32_t total = 0;
			for (bool v : alloc)
				total += v;
			if (!total)
				continue;
			uint32_t slot = a.output[a.mdi_count_offset];
			a.output[a.mdi_count_offset] = slot + total;
			for (uint32_t lane = 0; lane < 64u; lane++)
				if (alloc[lane])
					write_draw(a, slot++, chunk[lane], task_of[lane]);
		}
	}
}

template <int PHASE> static void by_flags(const CullArgs &a, uint32_t flags)
{
	const bool force = (flags & 4u) != 0u;
	switch (flags & 3u)
	{
	case 0: dispatch<PHASE, false, false>(a, force); break;
	case 1: dispatch<PHASE, true, false>(a, force); break;
	case 2: dispatch<PHASE, false, true>(a, force); break;
	default: dispatch<PHASE, true, true>(a, force); break;
	}
}

int main(int argc, char **argv)
{
	if (argc != 2)
	{
		fprintf(stderr, "usage: meshlet_cull_core_host <case file>\n");
		return 2;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	uint32_t h[13];
	get(h, sizeof(h), f);
	const uint32_t phase = h[0], flags = h[1];
	if (phase > 2u || flags > 7u || h[2] > (1u << 20) || h[3] > (1u << 20) || h[4] > (1u << 20) || h[5] > (1u << 20) || h[6] > (1u << 20) || h[7] > (1u << 24) ||
	    h[8] > (1u << 24) || h[12] > 16u)
		return 2;
	CullArgs a = {};
	get(a.camera_position, sizeof(a.camera_position), f);
	get(&a.frustum, 224, f);
	std::vector<uint32_t> dispatches(size_t(h[12]) * 4u);
	get(dispatches.data(), dispatches.size() * 4u, f);
	std::vector<Task> tasks(h[2]);
	std::vector<AABB> aabbs(h[3]);
	std::vector<Affine> transforms(h[4]);
	std::vector<Bound> bounds(h[5]);
	std::vector<Draw> draws(h[5]);
	std::vector<uint32_t> occluders(h[6]), output(h[7]);
	std::vector<float> chain(h[8]);
	get(tasks.data(), tasks.size() * sizeof(Task), f);
	get(aabbs.data(), aabbs.size() * sizeof(AABB), f);
	get(transforms.data(), transforms.size() * sizeof(Affine), f);
	get(bounds.data(), bounds.size() * sizeof(Bound), f);
	get(draws.data(), draws.size() * sizeof(Draw), f);
	get(occluders.data(), occluders.size() * 4u, f);
	get(output.data(), output.size() * 4u, f);
	get(chain.data(), chain.size() * 4u, f);
	fclose(f);

	a.tasks = tasks.data();
	a.aabbs = aabbs.data();
	a.transforms = transforms.data();
	a.bounds = bounds.data();
	a.draws = draws.data();
	a.occluders = occluders.data();
	a.output = output.data();
	a.chain = chain.data();
	a.task_count = h[2];
	a.aabb_count = h[3];
	a.transform_count = h[4];
	a.bound_count = a.draw_count = h[5];
	a.occluder_count = h[6];
	a.output_dwords = h[7];
	a.chain_width = h[9];
	a.chain_height = h[10];
	a.chain_levels = h[11];
	// what the launcher asks of the chain before a launch
	size_t texels = 0;
	for (uint32_t l = 0; l < a.chain_levels; l++)
		texels += size_t((a.chain_width >> l) ? (a.chain_width >> l) : 1u) * ((a.chain_height >> l) ? (a.chain_height >> l) : 1u);
	if (phase == 2u && (a.chain_levels == 0u || texels > chain.size()))
		return 2;
	for (size_t d = 0; d < dispatches.size(); d += 4u)
	{
		a.offset = dispatches[d];
		a.count = dispatches[d + 1];
		a.mdi_count_offset = dispatches[d + 2];
		a.draw_indirect_offset = dispatches[d + 3];
		if (a.mdi_count_offset >= a.output_dwords || a.draw_indirect_offset >= a.output_dwords)
			return 2;
		if (phase == 0u)
			by_flags<0>(a, flags);
		else if (phase == 1u)
			by_flags<1>(a, flags);
		else
			by_flags<2>(a, flags);
	}
	put(output.data(), output.size() * 4u);
	put(occluders.data(), occluders.size() * 4u);
	return 0;
}
