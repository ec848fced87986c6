// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The host-only part of Granite::Ocean's LOD update and static geometry (renderer/ocean.cpp:263-407, 826-835, 960-974, 1084-1090,
// 1102-1406): the grid that follows the camera, the push blocks of update_lod_pass, the meshes of build_buffers and the uniform block of
// get_render_info_heightmap.  Nothing here touches the device, so tests/cpp/ocean_lod_host.cpp links this unit and
// ocean_distribution.cpp alone.
//
// What the reference takes from its RenderContext and scene node is explicit state: set_camera stands in for refresh() and for
// get_visibility_frustum().get_planes(), a fixed-position flag with a centre for node / node_center_position.
#pragma once
#include <vector>
#include "../../../include/granite_hip.h"
#include "ocean_distribution.hpp"

namespace Granite
{
struct OceanVertex // ocean.cpp:1186-1190
{
	uint8_t pos[4];
	uint8_t weights[4];
};
struct OceanLodMesh
{
	std::vector<OceanVertex> vertices;
	std::vector<uint16_t> indices; // triangle strips, 0xffff restarts
};
struct OceanBorderMesh
{
	std::vector<vec3> positions;
	std::vector<uint16_t> indices;
};
// ocean.cpp:826-835, std140.
struct OceanData
{
	alignas(16) float world_offset[3];
	alignas(8) float coord_offset[2];
	alignas(8) float inv_heightmap_size[2];
	alignas(8) float inv_ocean_grid_size[2];
	alignas(8) float normal_uv_scale[2];
	alignas(8) float integer_to_world_mod[2];
	alignas(8) float heightmap_range[2];
};
static_assert(sizeof(OceanData) == 64, "OceanData is the reference's uniform block");
// What a rasteriser needs beside the buffers and maps (OceanInfo, ocean.cpp:837-860, 1082-1092).
struct OceanDrawInfo
{
	OceanData data;
	unsigned lods = 0;         // quad_lod.size(): buckets in use, meshes to bind
	unsigned lod_stride = 0;   // bytes between two buckets of ocean-lod-data
	unsigned border_count = 0; // indices of the border mesh; 0 in fixed-position mode with a heightmap
	unsigned index_type = 0;   // VK_INDEX_TYPE_UINT16: the ARM 32-bit workaround is not built
};

class OceanLod
{
public:
	static constexpr unsigned MaxLODIndirect = 8;
	static constexpr int MaxGridCoord = 1 << 20;

	// `config` as derive_ocean_parameters leaves it.  Builds the meshes (build_buffers).
	OceanLod(const OceanConfig &config, bool fixed_position, const vec3 &center_position);
	// What requesting the LOD update refuses (std::invalid_argument): no heightmap, grid_count or grid_resolution that is not a power
	// of two in 4 .. 128.
	static void check_lod_update(const OceanConfig &config);

	// Refuses (std::invalid_argument) non-finite input and, in moving mode, a snapped grid coordinate beyond +-2^20.
	void set_camera(const vec3 &position, const vec4 planes[6]);
	bool is_fixed_position() const { return fixed_position; }

	vec2 get_grid_size() const;
	vec2 get_snapped_grid_center() const;
	ivec2 get_grid_base_coord() const;
	vec3 get_world_offset() const;
	vec2 get_coord_offset() const;

	gr_push_ocean_update_lod update_lod_push() const;
	gr_push_ocean_cull cull_push() const;
	const float *get_frustum() const { return &frustum[0].x; }
	uint32_t get_wrap() const { return fixed_position ? 0u : 1u; } // NearestClamp : NearestWrap (ocean.cpp:388)
	void get_counts(uint32_t counts16[16]) const;

	unsigned get_lod_count() const { return unsigned(quad_lod.size()); }
	const OceanLodMesh &get_lod_mesh(unsigned lod) const { return quad_lod[lod]; }
	const OceanBorderMesh &get_border_mesh() const { return border; }
	OceanDrawInfo get_draw_info() const;

private:
	OceanConfig config;
	bool fixed_position;
	vec3 node_center_position;
	vec3 last_camera_position;
	vec4 frustum[6];
	std::vector<OceanLodMesh> quad_lod;
	OceanBorderMesh border;

	void build_lod(unsigned size, unsigned stride);
	void build_plane_grid(unsigned size, unsigned stride);
	void build_border(ivec2 base, ivec2 dx, ivec2 dy);
	void build_corner(ivec2 base, ivec2 dx, ivec2 dy);
	void build_fill_edge(vec2 base_outer, vec2 end_outer, ivec2 base_inner, ivec2 delta, ivec2 corner_delta);
	void build_buffers();
};
} // namespace Granite
