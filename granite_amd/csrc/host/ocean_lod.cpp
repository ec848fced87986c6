// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "ocean_lod.hpp"
#include <cmath>
#include <stdexcept>

namespace Granite
{
namespace
{
bool power_of_two_4_to_128(unsigned v) { return v >= 4 && v <= 128 && (v & (v - 1u)) == 0; }
ivec2 operator+(ivec2 a, ivec2 b) { return {a.x + b.x, a.y + b.y}; }
ivec2 operator-(ivec2 a, ivec2 b) { return {a.x - b.x, a.y - b.y}; }
ivec2 operator*(int s, ivec2 a) { return {s * a.x, s * a.y}; }
} // namespace

void OceanLod::check_lod_update(const OceanConfig &config)
{
	if (!config.heightmap)
		throw std::invalid_argument("Ocean: the LOD update needs a heightmap (the reference adds no LOD pass without one).");
	if (!power_of_two_4_to_128(config.grid_count))
		throw std::invalid_argument("Ocean: the LOD update needs a grid_count that is a power of two in 4 .. 128.");
	if (!power_of_two_4_to_128(config.grid_resolution))
		throw std::invalid_argument("Ocean: the LOD update needs a grid_resolution that is a power of two in 4 .. 128.");
}

OceanLod::OceanLod(const OceanConfig &config_, bool fixed_position_, const vec3 &center_position)
	: config(config_), fixed_position(fixed_position_), node_center_position(center_position)
{
	for (auto &p : frustum)
		p = vec4(0.0f, 0.0f, 0.0f, 1.0f); // everything is in view until a camera says otherwise
	build_buffers();
}

void OceanLod::set_camera(const vec3 &position, const vec4 planes[6])
{
	bool finite = std::isfinite(position.x) && std::isfinite(position.y) && std::isfinite(position.z);
	for (unsigned i = 0; i < 6; i++)
		for (int c = 0; c < 4; c++)
			finite = finite && std::isfinite(planes[i][c]);
	if (!finite)
		throw std::invalid_argument("Ocean: set_camera with a position or a plane that is not finite.");
	if (!fixed_position)
	{
		const float cx = std::round(position.x * (float(config.grid_count) / config.ocean_size.x));
		const float cz = std::round(position.z * (float(config.grid_count) / config.ocean_size.y));
		const float limit = float(MaxGridCoord - 128);
		if (!(std::fabs(cx) <= limit && std::fabs(cz) <= limit))
			throw std::invalid_argument("Ocean: set_camera puts the grid beyond +-2^20 blocks from the origin.");
	}
	last_camera_position = position;
	for (unsigned i = 0; i < 6; i++)
		frustum[i] = planes[i];
}

vec2 OceanLod::get_grid_size() const
{
	return {config.ocean_size.x / float(config.grid_count), config.ocean_size.y / float(config.grid_count)};
}

vec2 OceanLod::get_snapped_grid_center() const
{
	const vec2 inv_grid_size = {float(config.grid_count) / config.ocean_size.x, float(config.grid_count) / config.ocean_size.y};
	return {std::round(last_camera_position.x * inv_grid_size.x), std::round(last_camera_position.z * inv_grid_size.y)};
}

ivec2 OceanLod::get_grid_base_coord() const
{
	const vec2 center = get_snapped_grid_center();
	return {int(center.x) - int(config.grid_count >> 1), int(center.y) - int(config.grid_count >> 1)};
}

vec3 OceanLod::get_world_offset() const
{
	if (fixed_position)
		return node_center_position - vec3(config.ocean_size.x * 0.5f, 0.0f, config.ocean_size.y * 0.5f);
	return vec3(0.0f);
}

vec2 OceanLod::get_coord_offset() const
{
	if (fixed_position)
		return vec2(0.0f);
	const ivec2 base = get_grid_base_coord();
	return {float(base.x * int(config.grid_resolution)), float(base.y * int(config.grid_resolution))};
}

gr_push_ocean_update_lod OceanLod::update_lod_push() const
{
	gr_push_ocean_update_lod push = {};
	const vec3 shifted = last_camera_position - get_world_offset();
	push.shifted_camera_pos[0] = shifted.x;
	push.shifted_camera_pos[1] = shifted.y;
	push.shifted_camera_pos[2] = shifted.z;
	push.max_lod = float(quad_lod.size()) - 1.0f;
	const vec2 grid_size = get_grid_size();
	if (!fixed_position)
	{
		const ivec2 base = get_grid_base_coord();
		push.image_offset[0] = base.x;
		push.image_offset[1] = base.y;
		push.grid_base[0] = float(base.x) * grid_size.x;
		push.grid_base[1] = float(base.y) * grid_size.y;
	}
	push.num_threads[0] = push.num_threads[1] = int32_t(config.grid_count);
	push.grid_size[0] = grid_size.x;
	push.grid_size[1] = grid_size.y;
	push.lod_bias = config.lod_bias;
	return push;
}

gr_push_ocean_cull OceanLod::cull_push() const
{
	gr_push_ocean_cull push = {};
	const vec3 world_offset = get_world_offset();
	push.world_offset[0] = world_offset.x;
	push.world_offset[1] = world_offset.y;
	push.world_offset[2] = world_offset.z;
	const vec2 grid_size = get_grid_size();
	if (!fixed_position)
	{
		const ivec2 base = get_grid_base_coord();
		push.image_offset[0] = base.x;
		push.image_offset[1] = base.y;
		push.grid_base[0] = float(base.x) * grid_size.x;
		push.grid_base[1] = float(base.y) * grid_size.y;
	}
	push.num_threads[0] = push.num_threads[1] = config.grid_count;
	push.inv_num_threads[0] = push.inv_num_threads[1] = 1.0f / float(config.grid_count);
	push.grid_size[0] = grid_size.x;
	push.grid_size[1] = grid_size.y;
	push.grid_resolution[0] = push.grid_resolution[1] = float(config.grid_resolution);
	push.heightmap_range[0] = -10.0f;
	push.heightmap_range[1] = 10.0f;
	push.guard_band = 5.0f;
	push.lod_stride = config.grid_count * config.grid_count;
	push.max_lod = float(quad_lod.size()) - 1.0f;
	push.handle_edge_lods = fixed_position ? 0 : 1;
	return push;
}

void OceanLod::get_counts(uint32_t counts16[16]) const
{
	for (unsigned i = 0; i < 16; i++)
		counts16[i] = i < quad_lod.size() ? uint32_t(quad_lod[i].indices.size()) : 0u;
}

OceanDrawInfo OceanLod::get_draw_info() const
{
	OceanDrawInfo info = {};
	const vec3 world_offset = get_world_offset();
	const vec2 coord_offset = get_coord_offset(), grid_size = get_grid_size();
	info.data.world_offset[0] = world_offset.x;
	info.data.world_offset[1] = world_offset.y;
	info.data.world_offset[2] = world_offset.z;
	info.data.coord_offset[0] = coord_offset.x;
	info.data.coord_offset[1] = coord_offset.y;
	info.data.inv_heightmap_size[0] = info.data.inv_heightmap_size[1] = 1.0f / float(config.fft_resolution);
	info.data.inv_ocean_grid_size[0] = info.data.inv_ocean_grid_size[1] = 1.0f / float(config.grid_count * config.grid_resolution);
	info.data.normal_uv_scale[0] = info.data.normal_uv_scale[1] = config.normal_mod;
	info.data.integer_to_world_mod[0] = grid_size.x / float(config.grid_resolution);
	info.data.integer_to_world_mod[1] = grid_size.y / float(config.grid_resolution);
	info.data.heightmap_range[0] = -10.0f;
	info.data.heightmap_range[1] = 10.0f;
	info.lods = unsigned(quad_lod.size());
	info.lod_stride = config.grid_count * config.grid_count * unsigned(sizeof(gr_ocean_patch));
	info.border_count = unsigned(border.indices.size());
	info.index_type = 0; // VK_INDEX_TYPE_UINT16
	return info;
}

void OceanLod::build_border(ivec2 base, ivec2 dx, ivec2 dy)
{
	unsigned base_index = unsigned(border.positions.size());
	const unsigned position_count = (config.grid_count * 2 + 1) * 2;
	for (unsigned i = 0; i < position_count; i++)
	{
		const ivec2 p = base + int(i >> 1) * dx + int(i & 1) * dy;
		border.positions.emplace_back(float(p.x), float(p.y), float((i & 1) ^ 1));
		border.indices.push_back(uint16_t(base_index++));
	}
	border.indices.push_back(0xffffu);
}

void OceanLod::build_corner(ivec2 base, ivec2 dx, ivec2 dy)
{
	unsigned base_index = unsigned(border.positions.size());
	for (unsigned i = 0; i < 4; i++)
		border.indices.push_back(uint16_t(base_index++));
	border.indices.push_back(0xffffu);
	const ivec2 a = base + dx, b = base + dy, c = base + dx + dy;
	border.positions.emplace_back(float(base.x), float(base.y), 1.0f);
	border.positions.emplace_back(float(a.x), float(a.y), 0.0f);
	border.positions.emplace_back(float(b.x), float(b.y), 0.0f);
	border.positions.emplace_back(float(c.x), float(c.y), 0.0f);
}

void OceanLod::build_fill_edge(vec2 base_outer, vec2 end_outer, ivec2 base_inner, ivec2 delta, ivec2 corner_delta)
{
	unsigned base_index = unsigned(border.positions.size());
	const unsigned count = config.grid_count * 2 + 3;
	for (unsigned i = 0; i < count; i++)
	{
		ivec2 inner = base_inner;
		if (i == 0)
			inner = base_inner - corner_delta;
		else if (i + 1 == count)
			inner = base_inner + corner_delta;
		border.positions.emplace_back(float(inner.x), float(inner.y), 0.0f);

		const float outer_lerp = float(i) / float(count - 1);
		border.positions.emplace_back(std::round(base_outer.x * (1.0f - outer_lerp) + end_outer.x * outer_lerp),
		                              std::round(base_outer.y * (1.0f - outer_lerp) + end_outer.y * outer_lerp), 0.0f);
		if (i + 2 < count && i != 0)
			base_inner = base_inner + delta;
		border.indices.push_back(uint16_t(base_index++));
		border.indices.push_back(uint16_t(base_index++));
	}
	border.indices.push_back(0xffffu);
}

void OceanLod::build_plane_grid(unsigned size, unsigned stride)
{
	const unsigned size_1 = size + 1;
	const auto base_index = uint16_t(border.positions.size());
	for (unsigned y = 0; y <= size; y++)
		for (unsigned x = 0; x <= size; x++)
			border.positions.emplace_back(float(x * stride), float(y * stride), 1.0f);
	for (unsigned slice = 0; slice < size; slice++)
	{
		const unsigned base = slice * size_1;
		for (unsigned x = 0; x <= size; x++)
		{
			border.indices.push_back(uint16_t(base_index + base + x));
			border.indices.push_back(uint16_t(base_index + base + size_1 + x));
		}
		border.indices.push_back(0xffffu);
	}
}

void OceanLod::build_lod(unsigned size, unsigned stride)
{
	const unsigned size_1 = size + 1;
	OceanLodMesh lod;
	lod.vertices.reserve(size_1 * size_1);
	lod.indices.reserve(size * (2 * size_1 + 1));
	const unsigned half_size = config.grid_resolution >> 1;
	for (unsigned y = 0; y <= config.grid_resolution; y += stride)
	{
		for (unsigned x = 0; x <= config.grid_resolution; x += stride)
		{
			OceanVertex v = {};
			v.pos[0] = uint8_t(x);
			v.pos[1] = uint8_t(y);
			v.pos[2] = uint8_t(x < half_size);
			v.pos[3] = uint8_t(y < half_size);
			if (x == 0)
				v.weights[0] = 255;
			else if (x == config.grid_resolution)
				v.weights[1] = 255;
			else if (y == 0)
				v.weights[2] = 255;
			else if (y == config.grid_resolution)
				v.weights[3] = 255;
			lod.vertices.push_back(v);
		}
	}
	for (unsigned slice = 0; slice < size; slice++)
	{
		const unsigned base = slice * size_1;
		for (unsigned x = 0; x <= size; x++)
		{
			lod.indices.push_back(uint16_t(base + x));
			lod.indices.push_back(uint16_t(base + size_1 + x));
		}
		lod.indices.push_back(0xffffu);
	}
	quad_lod.push_back(std::move(lod));
}

void OceanLod::build_buffers()
{
	const int full = int(config.grid_count * config.grid_resolution);
	if (config.heightmap)
	{
		// uint8 positions and at most MaxLODIndirect LODs: grid_resolution beyond 128 builds no LOD meshes (check_lod_update refuses it).
		if (config.grid_resolution <= 128)
			for (unsigned size = config.grid_resolution, stride = 1; size >= 2; size >>= 1, stride <<= 1)
				build_lod(size, stride);
	}
	// 16-bit indices: a configuration whose plane grid and border have more vertices than they can name gets neither.
	const uint64_t side = uint64_t(config.grid_count) * 2 + 1;
	const uint64_t plane_vertices = config.heightmap ? 0 : side * side, border_vertices = fixed_position ? 0 : 4 * side * 2 + 16 + 4 * (side + 2) * 2;
	if (plane_vertices + border_vertices >= 0xffffu)
		return;
	if (!config.heightmap)
		build_plane_grid(config.grid_count * 2, config.grid_resolution >> 1);

	if (fixed_position)
		return;
	const int outer_delta = full >> 3, inner_delta = int(config.grid_resolution >> 1);
	build_border({full, 0}, {-inner_delta, 0}, {0, -outer_delta});   // top
	build_border({0, 0}, {0, inner_delta}, {-outer_delta, 0});       // left
	build_border({0, full}, {inner_delta, 0}, {0, outer_delta});     // bottom
	build_border({full, full}, {0, -inner_delta}, {outer_delta, 0}); // right
	build_corner({0, 0}, {0, -outer_delta}, {-outer_delta, 0});      // top-left
	build_corner({0, full}, {-outer_delta, 0}, {0, outer_delta});    // bottom-left
	build_corner({full, 0}, {outer_delta, 0}, {0, -outer_delta});    // top-right
	build_corner({full, full}, {0, outer_delta}, {outer_delta, 0});  // bottom-right
	const float neg_edge_size = float(-32 * 1024), pos_edge_size = float(32 * 1024) + float(full);
	build_fill_edge({pos_edge_size, neg_edge_size}, {neg_edge_size, neg_edge_size}, {full, -outer_delta}, {-inner_delta, 0}, {-outer_delta, 0});
	build_fill_edge({neg_edge_size, neg_edge_size}, {neg_edge_size, pos_edge_size}, {-outer_delta, 0}, {0, inner_delta}, {0, outer_delta});
	build_fill_edge({neg_edge_size, pos_edge_size}, {pos_edge_size, pos_edge_size}, {0, outer_delta + full}, {inner_delta, 0}, {outer_delta, 0});
	build_fill_edge({pos_edge_size, pos_edge_size}, {pos_edge_size, neg_edge_size}, {outer_delta + full, full}, {0, -inner_delta}, {0, -outer_delta});
}
} // namespace Granite
