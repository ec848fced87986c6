// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The host side of meshlet culling, restated over the C ABI of include/granite_hip.h with Granite's names:
//   fill_meshlet_culling_ubo   Renderer::bind_meshlet_culling_ubo (renderer/renderer.cpp:540-572)
//   build_task_infos           the inner loop of SceneTransformManager::update_task_buffer (renderer/scene_renderer.cpp:800-833)
//   place_mesh_chunks          a mesh's chunk bounds and MDI records at a 32-aligned offset of the shared bounds / draws buffers, as the
//                              reference's indirect allocator hands out sub-blocks of 32
//   build_mdi_culling_pass     renderer/scene_renderer.cpp:954-1035, one gr_meshlet_cull per MDICall
// The first three are host arithmetic that needs no device (meshlet_cull.cpp); the last launches (meshlet_cull_pass.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "../math.hpp"
#include "meshlet.hpp"

namespace Granite
{
struct MeshletViewport // VkViewport's x, y, width, height
{
	float x = 0.0f, y = 0.0f, width = 0.0f, height = 0.0f;
};

struct SceneHiZ // RenderContext::get_scene_hiz_view / get_scene_hiz_min_lod: the chain gr_hiz writes with output_downsample = 1
{
	const void *chain = nullptr; // device memory; null: no HiZ, the block's HiZ fields stay zero
	uint32_t width = 0, height = 0, levels = 0;
	uint32_t min_lod = 0;
};

// viewport, winding, the six planes, view, viewport_scale_bias from the viewport halves and projection[0].x, -projection[1].y,
// projection[3].xy, and the HiZ fields from the chain's size, levels and min LOD.
void fill_meshlet_culling_ubo(gr_meshlet_frustum &ubo, const mat4 &projection, const mat4 &view, const vec4 planes[6], const MeshletViewport &viewport, bool cw,
                              const SceneHiZ *hiz);

struct MeshletRange // ResourceManager::get_mesh_draw_range(...).meshlet: chunks of 256 primitives
{
	uint32_t offset = 0, count = 0;
};

struct MeshletInstance // what update_task_buffer reads of one renderable
{
	uint32_t aabb_instance = 0;
	uint32_t node_instance = 0; // the skin's transform offset for a skinned mesh
	uint32_t material_flags = 0;
	uint32_t occluder_state_offset = 0;
	MeshletRange range;
};

// One task per 32 chunks of the instance's range, appended to `tasks`: mesh_index_count = offset + j + (min(count - j, 32) - 1),
// occluder_state_offset growing by one per task.  Returns the number of tasks appended (0 for an empty range); false with *error for a
// range whose offset is no multiple of 32 (the reference asserts).
bool build_task_infos(const MeshletInstance &instance, std::vector<gr_meshlet_task> &tasks, std::string *error = nullptr);

// Appends the view's bounds_256 and its RuntimeHeaderDecodedMDI records (build_indirect_records with these offsets) to `bounds` and
// `draws`, after padding both with zero records to a multiple of 32.  Returns the range to give MeshletInstance.
MeshletRange place_mesh_chunks(const Meshlet::MeshView &view, uint32_t primitive_offset, uint32_t vertex_offset, std::vector<gr_meshlet_bound> &bounds,
                               std::vector<gr_meshlet_draw> &draws);

enum class CullingPhase // SceneTransformManager::CullingPhase
{
	OneShot,
	First,
	MotionVector,
	Second
};
int culling_phase_index(CullingPhase phase); // 0, 1, 1, 2

struct MDICall // SceneTransformManager::MDICall and the task range of its draw type
{
	uint32_t indirect_count_offset = 0; // bytes into the output buffer
	uint32_t indirect_offset = 0;       // bytes into the output buffer
	uint32_t indirect_count_max = 0;    // 0: nothing of this type, the call is skipped
	std::pair<uint32_t, uint32_t> task_range; // first task, tasks
	bool skinned = false;
};

struct CullingContext // what bind_global_parameters, bind_scene_transform_parameters and the UBO give the shader for one RenderContext
{
	mat4 projection, view;
	vec4 planes[6];
	vec3 camera_position;
	const gr_meshlet_task *tasks = nullptr;
	const gr_meshlet_aabb *aabbs = nullptr;
	const gr_mat_affine *transforms = nullptr;
	const gr_meshlet_bound *bounds = nullptr;
	const gr_meshlet_draw *draws = nullptr;
	uint32_t *occluders = nullptr;
	uint32_t task_count = 0, aabb_count = 0, transform_count = 0, chunk_count = 0, occluder_count = 0;
	uint32_t *indirect = nullptr; // count words and records
	uint64_t indirect_dwords = 0;
	SceneHiZ hiz;
};

// The arguments and push block of one call, as build_mdi_culling_pass issues it (no device).
void describe_mdi_cull(const CullingContext &ctx, CullingPhase phase, bool force_visible, uint32_t width, uint32_t height, const MDICall &call,
                       gr_meshlet_cull_args &args, gr_push_meshlet_cull &push);

// For one context: ORTHO from projection[3].w == 1, calls with indirect_count_max == 0 skipped, one gr_meshlet_cull per call.
// false where a launch is refused (gr_last_error(ctx) says why).
bool build_mdi_culling_pass(gr_ctx *ctx, gr_stream stream, const CullingContext &context, CullingPhase phase, bool force_visible, uint32_t width, uint32_t height,
                            const std::vector<MDICall> &calls);
} // namespace Granite
