// TEST INFRASTRUCTURE.  granite_amd/csrc/host/mesh/meshlet_cull.cpp -- the culling pass's host arithmetic -- with no device:
//   meshlet_cull_host ubo IN OUT          IN: projection[16], view[16], planes[24], viewport {x, y, width, height}, then five dwords
//                                         {cw, hiz present, chain width, height, levels, min lod}; OUT: the 224-byte Frustum block
//   meshlet_cull_host tasks AABB NODE FLAGS OCCLUDER OFFSET COUNT OUT     build_task_infos' records; exit 5 with the reason for a refusal
//   meshlet_cull_host place OUT PRIM VERT FILE...   place_mesh_chunks for every file in turn: per file {offset, count}, then the bounds,
//                                         then the draws
//   meshlet_cull_host describe IN OUT     IN as for ubo, then {phase enum, force_visible, width, height, count_offset, indirect_offset,
//                                         count_max, first task, tasks, skinned}; OUT: {phase, flags, push[4]} and the Frustum block
// tests/test_meshlet_cull_host_cpu.py compares with the reference's arithmetic restated in fp32.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../granite_amd/csrc/host/mesh/meshlet_cull.hpp"

using namespace Granite;

static std::vector<uint32_t> read_words(const char *path)
{
	FILE *f = fopen(path, "rb");
	if (!f)
		exit(3);
	fseek(f, 0, SEEK_END);
	const size_t size = size_t(ftell(f));
	fseek(f, 0, SEEK_SET);
	std::vector<uint32_t> words((size + 3) / 4);
	if (size && fread(words.data(), 1, size, f) != size)
		exit(3);
	fclose(f);
	return words;
}

static void write_all(const char *path, const std::vector<uint8_t> &bytes)
{
	FILE *f = fopen(path, "wb");
	if (!f || (bytes.size() && fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) || fclose(f) != 0)
		exit(3);
}

template <typename T> static void append(std::vector<uint8_t> &out, const T *data, size_t count)
{
	const uint8_t *p = reinterpret_cast<const uint8_t *>(data);
	out.insert(out.end(), p, p + count * sizeof(T));
}

struct CameraInput
{
	mat4 projection, view;
	vec4 planes[6];
	MeshletViewport viewport;
	bool cw;
	SceneHiZ hiz;
};

static CameraInput parse_camera(const std::vector<uint32_t> &w)
{
	if (w.size() < 66)
		exit(2);
	CameraInput c;
	memcpy(static_cast<void *>(&c.projection), &w[0], 64);
	memcpy(static_cast<void *>(&c.view), &w[16], 64);
	memcpy(static_cast<void *>(c.planes), &w[32], 96);
	memcpy(static_cast<void *>(&c.viewport), &w[56], 16);
	c.cw = w[60] != 0;
	static const float marker = 0.0f;
	c.hiz.chain = w[61] ? &marker : nullptr; // only tested for presence
	c.hiz.width = w[62];
	c.hiz.height = w[63];
	c.hiz.levels = w[64];
	c.hiz.min_lod = w[65];
	return c;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	std::vector<uint8_t> out;
	if (mode == "ubo" && argc == 4)
	{
		const CameraInput c = parse_camera(read_words(argv[2]));
		gr_meshlet_frustum ubo;
		fill_meshlet_culling_ubo(ubo, c.projection, c.view, c.planes, c.viewport, c.cw, &c.hiz);
		append(out, &ubo, 1);
		write_all(argv[3], out);
		return 0;
	}
	if (mode == "tasks" && argc == 9)
	{
		MeshletInstance instance;
		instance.aabb_instance = uint32_t(strtoul(argv[2], nullptr, 0));
		instance.node_instance = uint32_t(strtoul(argv[3], nullptr, 0));
		instance.material_flags = uint32_t(strtoul(argv[4], nullptr, 0));
		instance.occluder_state_offset = uint32_t(strtoul(argv[5], nullptr, 0));
		instance.range.offset = uint32_t(strtoul(argv[6], nullptr, 0));
		instance.range.count = uint32_t(strtoul(argv[7], nullptr, 0));
		std::vector<gr_meshlet_task> tasks;
		std::string why;
		if (!build_task_infos(instance, tasks, &why))
		{
			fprintf(stderr, "%s\n", why.c_str());
			return 5;
		}
		append(out, tasks.data(), tasks.size());
		write_all(argv[8], out);
		return 0;
	}
	if (mode == "place" && argc >= 6)
	{
		std::vector<gr_meshlet_bound> bounds;
		std::vector<gr_meshlet_draw> draws;
		std::vector<uint32_t> ranges;
		uint32_t prim = uint32_t(strtoul(argv[3], nullptr, 0)), vert = uint32_t(strtoul(argv[4], nullptr, 0));
		for (int i = 5; i < argc; i++)
		{
			const std::vector<uint32_t> words = read_words(argv[i]);
			FILE *f = fopen(argv[i], "rb");
			fseek(f, 0, SEEK_END);
			const size_t size = size_t(ftell(f));
			fclose(f);
			std::string why;
			const Meshlet::MeshView view = Meshlet::create_mesh_view(words.data(), size, &why);
			if (!view.format_header)
			{
				fprintf(stderr, "%s\n", why.c_str());
				return 5;
			}
			const MeshletRange r = place_mesh_chunks(view, prim, vert, bounds, draws);
			ranges.push_back(r.offset);
			ranges.push_back(r.count);
			prim += view.total_primitives;
			vert += view.total_vertices;
		}
		if (bounds.size() != draws.size())
			return 4;
		append(out, ranges.data(), ranges.size());
		append(out, bounds.data(), bounds.size());
		append(out, draws.data(), draws.size());
		write_all(argv[2], out);
		return 0;
	}
	if (mode == "describe" && argc == 4)
	{
		const std::vector<uint32_t> w = read_words(argv[2]);
		if (w.size() < 76)
			return 2;
		const CameraInput c = parse_camera(w);
		CullingContext ctx;
		ctx.projection = c.projection;
		ctx.view = c.view;
		for (int i = 0; i < 6; i++)
			ctx.planes[i] = c.planes[i];
		ctx.hiz = c.hiz;
		MDICall call;
		call.indirect_count_offset = w[70];
		call.indirect_offset = w[71];
		call.indirect_count_max = w[72];
		call.task_range = {w[73], w[74]};
		call.skinned = w[75] != 0;
		gr_meshlet_cull_args args;
		gr_push_meshlet_cull push;
		describe_mdi_cull(ctx, CullingPhase(w[66]), w[67] != 0, w[68], w[69], call, args, push);
		const uint32_t head[6] = {args.phase, args.flags, push.offset, push.count, push.mdi_count_offset, push.draw_indirect_offset};
		append(out, head, 6);
		append(out, &args.frustum, 1);
		write_all(argv[3], out);
		return 0;
	}
	return 2;
}
