// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Meshlet culling's host arithmetic: no device, no launch (see meshlet_cull.hpp).
#include "meshlet_cull.hpp"
#include <algorithm>
#include <cstring>

namespace Granite
{
void fill_meshlet_culling_ubo(gr_meshlet_frustum &ubo, const mat4 &projection, const mat4 &view, const vec4 planes[6], const MeshletViewport &viewport, bool cw,
                              const SceneHiZ *hiz)
{
	memset(&ubo, 0, sizeof(ubo));
	// renderer.cpp:545-548
	ubo.viewport[0] = viewport.x + 0.5f * viewport.width - 0.5f;
	ubo.viewport[1] = viewport.y + 0.5f * viewport.height - 0.5f;
	ubo.viewport[2] = 0.5f * viewport.width;
	ubo.viewport[3] = 0.5f * viewport.height;
	ubo.winding = cw ? -1.0f : 1.0f;
	static_assert(sizeof(vec4) == 16 && sizeof(mat4) == 64, "tightly packed");
	memcpy(ubo.planes, planes, sizeof(ubo.planes));
	memcpy(ubo.view, &view, sizeof(ubo.view));

	// renderer.cpp:553-563
	const float half_x = 0.5f * viewport.width, half_y = 0.5f * viewport.height;
	float scale_bias[4] = {half_x, half_y, half_x, half_y};
	scale_bias[2] += scale_bias[0] * projection.c[3].x;
	scale_bias[3] += scale_bias[1] * projection.c[3].y;
	scale_bias[0] *= projection.c[0].x;
	scale_bias[1] *= -projection.c[1].y;
	memcpy(ubo.viewport_scale_bias, scale_bias, sizeof(scale_bias));

	// renderer.cpp:565-571
	if (hiz && hiz->chain)
	{
		ubo.hiz_resolution[0] = int32_t(hiz->width << hiz->min_lod);
		ubo.hiz_resolution[1] = int32_t(hiz->height << hiz->min_lod);
		ubo.hiz_min_lod = int32_t(hiz->min_lod);
		ubo.hiz_max_lod = int32_t(hiz->levels - 1u + hiz->min_lod);
	}
}

bool build_task_infos(const MeshletInstance &instance, std::vector<gr_meshlet_task> &tasks, std::string *error)
{
	if (instance.range.count == 0u)
		return true;
	if ((instance.range.offset & 31u) != 0u)
	{
		if (error)
			*error = "build_task_infos: meshlet range offset " + std::to_string(instance.range.offset) + " is not a multiple of 32";
		return false;
	}
	gr_meshlet_task draw = {};
	draw.aabb_instance = instance.aabb_instance;
	draw.node_instance = instance.node_instance;
	draw.material_flags = instance.material_flags;
	draw.occluder_state_offset = instance.occluder_state_offset;
	for (uint32_t j = 0; j < instance.range.count; j += 32u)
	{
		draw.mesh_index_count = instance.range.offset + j + (std::min(instance.range.count - j, 32u) - 1u);
		tasks.push_back(draw);
		draw.occluder_state_offset++;
	}
	return true;
}

MeshletRange place_mesh_chunks(const Meshlet::MeshView &view, uint32_t primitive_offset, uint32_t vertex_offset, std::vector<gr_meshlet_bound> &bounds,
                               std::vector<gr_meshlet_draw> &draws)
{
	static_assert(sizeof(gr_meshlet_bound) == sizeof(Meshlet::Bound) && sizeof(gr_meshlet_draw) == sizeof(Meshlet::RuntimeHeaderDecodedMDI), "the kernel's records are Meshlet's");
	const size_t first = (std::max(bounds.size(), draws.size()) + 31u) & ~size_t(31);
	bounds.resize(first, gr_meshlet_bound{});
	draws.resize(first, gr_meshlet_draw{});
	MeshletRange range;
	range.offset = uint32_t(first);
	range.count = view.num_bounds_256;
	if (range.count == 0u)
		return range;
	bounds.resize(first + range.count);
	draws.resize(first + range.count);
	memcpy(bounds.data() + first, view.bounds_256, size_t(range.count) * sizeof(gr_meshlet_bound));
	const std::vector<uint8_t> records = Meshlet::build_indirect_records(view, Meshlet::RuntimeStyle::MDI, primitive_offset, vertex_offset);
	memcpy(draws.data() + first, records.data(), std::min(records.size(), size_t(range.count) * sizeof(gr_meshlet_draw)));
	return range;
}

int culling_phase_index(CullingPhase phase)
{
	switch (phase)
	{
	case CullingPhase::OneShot:
		return 0;
	case CullingPhase::First:
	case CullingPhase::MotionVector:
		return 1;
	default:
		return 2;
	}
}

void describe_mdi_cull(const CullingContext &ctx, CullingPhase phase, bool force_visible, uint32_t width, uint32_t height, const MDICall &call,
                       gr_meshlet_cull_args &args, gr_push_meshlet_cull &push)
{
	args = {};
	args.tasks = ctx.tasks;
	args.task_count = ctx.task_count;
	args.aabbs = ctx.aabbs;
	args.aabb_count = ctx.aabb_count;
	args.transforms = ctx.transforms;
	args.transform_count = ctx.transform_count;
	args.bounds = ctx.bounds;
	args.bound_count = ctx.chunk_count;
	args.draws = ctx.draws;
	args.draw_count = ctx.chunk_count;
	args.occluders = ctx.occluders;
	args.occluder_count = ctx.occluder_count;
	args.output = ctx.indirect;
	args.output_dwords = ctx.indirect_dwords;
	args.chain = ctx.hiz.chain;
	args.chain_width = ctx.hiz.width;
	args.chain_height = ctx.hiz.height;
	args.chain_levels = ctx.hiz.levels;
	args.phase = uint32_t(culling_phase_index(phase));
	// scene_renderer.cpp:1021-1023, 981
	const bool ortho = ctx.projection.c[3].w == 1.0f;
	args.flags = (ortho ? GR_MESHLET_CULL_ORTHO : 0u) | (call.skinned ? GR_MESHLET_CULL_SKINNED : 0u) | (force_visible ? GR_MESHLET_CULL_FORCE_VISIBLE : 0u);
	args.camera_position[0] = ctx.camera_position.x;
	args.camera_position[1] = ctx.camera_position.y;
	args.camera_position[2] = ctx.camera_position.z;
	// scene_renderer.cpp:996-1000
	MeshletViewport vp;
	vp.width = float(width);
	vp.height = float(height);
	fill_meshlet_culling_ubo(args.frustum, ctx.projection, ctx.view, ctx.planes, vp, false, &ctx.hiz);
	// scene_renderer.cpp:1016-1019
	push.offset = call.task_range.first;
	push.count = call.task_range.second;
	push.mdi_count_offset = call.indirect_count_offset / uint32_t(sizeof(uint32_t));
	push.draw_indirect_offset = call.indirect_offset / uint32_t(sizeof(uint32_t));
}
} // namespace Granite
