// TEST INFRASTRUCTURE (needs a device).  MESHLET4 files through the culling pass's host layer, as an integrator would use it:
// create_mesh_view and place_mesh_chunks per file, build_task_infos per instance, buffers uploaded, build_mdi_culling_pass for one
// context with two MDICalls, the second with indirect_count_max = 0 and offsets no launch would accept (it must be skipped).
//   meshlet_cull_pass SCENE OUT
// SCENE, dwords: phase (CullingPhase), force_visible, width, height, files, instances, chain width, height, levels, min lod; projection[16],
// view[16], planes[24], camera[3]; per instance {file, material_flags}; instances x AABB (8 floats); instances x transform (12 floats);
// the chain's floats; per file its size in bytes and its bytes padded to whole dwords.  Occluder word i starts as i * 2654435761 ^ 0x5bd1e995,
// every fifth 0.  OUT: counts {tasks, chunks, output dwords}, tasks, bounds, draws, the output buffer, the occluder words.
// tests/test_gpu_meshlet_cull_pass.py feeds the same arrays to tests/meshlet_cull_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../granite_amd/csrc/host/mesh/meshlet_cull.hpp"

using namespace Granite;

#define CHECK(call)                                                            \
	do                                                                         \
	{                                                                          \
		if ((call) != GR_OK)                                                   \
		{                                                                      \
			fprintf(stderr, "%s: %s\n", #call, gr_last_error(ctx));            \
			return 1;                                                          \
		}                                                                      \
	} while (0)

template <typename T> static void *upload(gr_ctx *ctx, const std::vector<T> &v)
{
	void *p = nullptr;
	if (gr_alloc(ctx, v.size() * sizeof(T) + 16, &p) != GR_OK || (!v.empty() && gr_upload(ctx, nullptr, p, v.data(), v.size() * sizeof(T)) != GR_OK))
	{
		fprintf(stderr, "upload: %s\n", gr_last_error(ctx));
		exit(1);
	}
	return p;
}

int main(int argc, char **argv)
{
	if (argc != 3)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 3;
	fseek(f, 0, SEEK_END);
	const size_t size = size_t(ftell(f));
	fseek(f, 0, SEEK_SET);
	std::vector<uint32_t> w(size / 4);
	if (fread(w.data(), 4, w.size(), f) != w.size())
		return 3;
	fclose(f);
	const uint32_t phase = w[0], force = w[1], width = w[2], height = w[3], files = w[4], instances = w[5];
	CullingContext c;
	c.hiz.width = w[6];
	c.hiz.height = w[7];
	c.hiz.levels = w[8];
	c.hiz.min_lod = w[9];
	size_t at = 10;
	memcpy(static_cast<void *>(&c.projection), &w[at], 64);
	memcpy(static_cast<void *>(&c.view), &w[at + 16], 64);
	memcpy(static_cast<void *>(c.planes), &w[at + 32], 96);
	memcpy(static_cast<void *>(&c.camera_position), &w[at + 56], 12);
	at += 59;
	const uint32_t *instance_words = &w[at];
	at += 2 * size_t(instances);
	std::vector<gr_meshlet_aabb> aabbs(instances);
	memcpy(aabbs.data(), &w[at], instances * sizeof(gr_meshlet_aabb));
	at += 8 * size_t(instances);
	std::vector<gr_mat_affine> transforms(instances);
	memcpy(transforms.data(), &w[at], instances * sizeof(gr_mat_affine));
	at += 12 * size_t(instances);
	size_t texels = 0;
	for (uint32_t l = 0; l < c.hiz.levels; l++)
		texels += size_t((c.hiz.width >> l) ? (c.hiz.width >> l) : 1u) * ((c.hiz.height >> l) ? (c.hiz.height >> l) : 1u);
	std::vector<float> chain(texels);
	memcpy(chain.data(), &w[at], texels * 4);
	at += texels;

	std::vector<gr_meshlet_bound> bounds;
	std::vector<gr_meshlet_draw> draws;
	std::vector<MeshletRange> ranges;
	uint32_t prim = 0, vert = 0;
	for (uint32_t i = 0; i < files; i++)
	{
		const uint32_t bytes = w[at++];
		std::string why;
		const Meshlet::MeshView view = Meshlet::create_mesh_view(&w[at], bytes, &why);
		if (!view.format_header)
		{
			fprintf(stderr, "file %u: %s\n", i, why.c_str());
			return 5;
		}
		ranges.push_back(place_mesh_chunks(view, prim, vert, bounds, draws));
		prim += view.total_primitives;
		vert += view.total_vertices;
		at += (bytes + 3) / 4;
	}
	std::vector<gr_meshlet_task> tasks;
	for (uint32_t i = 0; i < instances; i++)
	{
		MeshletInstance instance;
		instance.aabb_instance = i;
		instance.node_instance = i;
		instance.material_flags = instance_words[2 * i + 1];
		instance.occluder_state_offset = uint32_t(tasks.size());
		instance.range = ranges.at(instance_words[2 * i]);
		std::string why;
		if (!build_task_infos(instance, tasks, &why))
		{
			fprintf(stderr, "%s\n", why.c_str());
			return 5;
		}
	}
	std::vector<uint32_t> occluders(tasks.size());
	for (size_t i = 0; i < occluders.size(); i++)
		occluders[i] = i % 5 == 0 ? 0u : (uint32_t(i) * 2654435761u) ^ 0x5bd1e995u;
	uint64_t chunks_in_tasks = 0;
	for (const auto &t : tasks)
		chunks_in_tasks += (t.mesh_index_count & 31u) + 1u;
	std::vector<uint32_t> output(4 + 5 * chunks_in_tasks + 7, 0xcdcdcdcdu);
	output[0] = output[1] = output[2] = output[3] = 0u;

	gr_ctx *ctx = gr_create(0);
	if (!ctx)
		return 1;
	c.tasks = static_cast<const gr_meshlet_task *>(upload(ctx, tasks));
	c.aabbs = static_cast<const gr_meshlet_aabb *>(upload(ctx, aabbs));
	c.transforms = static_cast<const gr_mat_affine *>(upload(ctx, transforms));
	c.bounds = static_cast<const gr_meshlet_bound *>(upload(ctx, bounds));
	c.draws = static_cast<const gr_meshlet_draw *>(upload(ctx, draws));
	c.occluders = static_cast<uint32_t *>(upload(ctx, occluders));
	c.indirect = static_cast<uint32_t *>(upload(ctx, output));
	c.hiz.chain = upload(ctx, chain);
	c.task_count = uint32_t(tasks.size());
	c.aabb_count = c.transform_count = instances;
	c.chunk_count = uint32_t(bounds.size());
	c.occluder_count = uint32_t(occluders.size());
	c.indirect_dwords = output.size();
	CHECK(gr_sync(ctx, nullptr));

	std::vector<MDICall> calls(2);
	calls[0].indirect_count_offset = 0;
	calls[0].indirect_offset = 4 * sizeof(uint32_t);
	calls[0].indirect_count_max = uint32_t(chunks_in_tasks);
	calls[0].task_range = {0u, uint32_t(tasks.size())};
	calls[1].indirect_count_offset = 0xfffffff0u;
	calls[1].indirect_offset = 0xfffffff0u;
	calls[1].indirect_count_max = 0;
	calls[1].task_range = {0u, uint32_t(tasks.size())};
	calls[1].skinned = true;
	if (!build_mdi_culling_pass(ctx, nullptr, c, CullingPhase(phase), force != 0, width, height, calls))
	{
		fprintf(stderr, "build_mdi_culling_pass: %s\n", gr_last_error(ctx));
		return 1;
	}
	CHECK(gr_sync(ctx, nullptr));
	CHECK(gr_download(ctx, nullptr, output.data(), c.indirect, output.size() * 4));
	if (!occluders.empty())
		CHECK(gr_download(ctx, nullptr, occluders.data(), c.occluders, occluders.size() * 4));
	CHECK(gr_sync(ctx, nullptr));

	f = fopen(argv[2], "wb");
	if (!f)
		return 3;
	const uint32_t head[3] = {uint32_t(tasks.size()), uint32_t(bounds.size()), uint32_t(output.size())};
	fwrite(head, 4, 3, f);
	fwrite(tasks.data(), sizeof(gr_meshlet_task), tasks.size(), f);
	fwrite(bounds.data(), sizeof(gr_meshlet_bound), bounds.size(), f);
	fwrite(draws.data(), sizeof(gr_meshlet_draw), draws.size(), f);
	fwrite(output.data(), 4, output.size(), f);
	fwrite(occluders.data(), 4, occluders.size(), f);
	fclose(f);
	gr_destroy(ctx);
	return 0;
}
