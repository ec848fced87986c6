// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Meshlet culling: what assets/shaders/meshlet_cull.comp decides per lane with inc/meshlet_render.h -- frustum_cull, cluster_cull,
// view_transform_yz_flip, project_sphere_flat, cluster_cull_hiz and hiz_cull.  Plain functions: meshlet_cull.hip calls them from its
// kernel, tests/cpp/meshlet_cull_core_host.cpp builds the same text for the host, where tests/test_meshlet_cull_core_cpu.py holds it to
// the executed shader's outputs (tests/golden/meshlet_cull_shader_v1.npz) before a device sees it.
//
// Floating point: every operation is one IEEE fp32 operation in the order the shader and oracle/ref_build/glsl_cpu.hpp perform it: dot
// sums left to right, matrix x vector sums column by column, vector x matrix is one dot per column, length(a) = sqrtf(dot(a, a)),
// normalize(a) = a / length(a) with one division per component.  Build without contraction and with correctly rounded division and
// square root.  The decisions are comparisons of such values, so they equal the shader's bit for bit.
//
// What the shader leaves to its environment and this text decides:
//   - every index read from device data (task, AABB, transform, bound / draw, occluder word) is held to its buffer's element count; an
//     element outside is not visible and is never dereferenced; an occluder word outside reads 0 and is not written;
//   - ivec2(range) in hiz_cull is undefined in GLSL outside int's range.  Here the float is clamped to [-2^31, 2^31 - 128] first (NaN goes
//     to -2^31); the clamp to [0, hiz_resolution - 1] that follows makes that equal to the shader wherever the shader's is defined;
//   - a HiZ texel index is held to its level, so that no frustum block can address outside the chain (the launcher also refuses a block
//     that does not describe the chain).
#pragma once
#include <cmath>
#include <cstdint>
#include "core_base.hpp"

namespace gr_cull
{
using gr_core::clampi;
using gr_core::dot3;
using Vec3 = gr_core::f3;

struct Task // MeshAssetDrawTaskInfo, inc/meshlet_render_types.h:15-22
{
	uint32_t aabb_instance, occluder_state_offset, node_instance, mesh_index_count, material_flags;
};
struct AABB // inc/meshlet_render_types.h:4-7
{
	float lo[3], pad0, hi[3], pad1;
};
struct Bound // inc/meshlet_render_types.h:9-13
{
	float center_radius[4], cone[4];
};
struct Affine // mat_affine, inc/affine.h:4-7
{
	float rows[3][4];
};
struct Draw // meshlet_cull.comp:16-21
{
	uint32_t index_count, first_index;
	int32_t vertex_offset;
};
struct Frustum // inc/meshlet_ubos.h:4-14, std140
{
	float viewport[4];
	float planes[6][4];
	float view[4][4]; // column major
	float viewport_scale_bias[4];
	int32_t hiz_resolution[2];
	float winding;
	int32_t hiz_min_lod, hiz_max_lod;
	uint32_t pad[3];
};
static_assert(sizeof(Task) == 20 && sizeof(AABB) == 32 && sizeof(Bound) == 32 && sizeof(Affine) == 48 && sizeof(Draw) == 12 && sizeof(Frustum) == 224,
              "records are the shader's");

struct CullArgs
{
	const Task *tasks;
	const AABB *aabbs;
	const Affine *transforms;
	const Bound *bounds;
	const Draw *draws;
	uint32_t *occluders;
	uint32_t *output;
	const float *chain; // R32_SFLOAT levels, tightly packed one after the other
	uint32_t task_count, aabb_count, transform_count, bound_count, draw_count, occluder_count;
	uint64_t output_dwords;
	uint32_t chain_width, chain_height, chain_levels;
	uint32_t offset, count, mdi_count_offset, draw_indirect_offset; // the push block
	float camera_position[3];
	Frustum frustum;
};

// dot(vec4(v, 1.0), p)
GR_HD float dot_point(const Vec3 &v, const float p[4]) { return v.x * p[0] + v.y * p[1] + v.z * p[2] + 1.0f * p[3]; }

GR_HD int glsl_clampi(int v, int lo, int hi) // GLSL's clamp: min(max(v, lo), hi), also where lo > hi
{
	const int m = v > lo ? v : lo;
	return m < hi ? m : hi;
}
// GLSL findMSB(int): -1 for 0 and -1; for a negative value the highest 0 bit.
GR_HD int find_msb(int v)
{
	uint32_t u = uint32_t(v < 0 ? ~v : v);
	int r = -1;
	while (u)
	{
		u >>= 1;
		r++;
	}
	return r;
}
GR_HD int float_to_int(float v)
{
	const float c = fminf(fmaxf(v, -2147483648.0f), 2147483520.0f); // fmaxf(NaN, a) = a
	return int(c);
}

// texelFetch(uHiZDepth, (x, y), level): level `level` of the chain is max(w >> level, 1) x max(h >> level, 1) texels
GR_HD float hiz_texel(const CullArgs &a, int x, int y, int level)
{
	level = clampi(level, 0, int(a.chain_levels) - 1);
	uint32_t offset = 0;
	for (int l = 0; l < level; l++)
	{
		const uint32_t w = a.chain_width >> l, h = a.chain_height >> l;
		offset += (w ? w : 1u) * (h ? h : 1u);
	}
	const uint32_t w0 = a.chain_width >> level, h0 = a.chain_height >> level;
	const int w = int(w0 ? w0 : 1u), h = int(h0 ? h0 : 1u);
	return a.chain[offset + uint32_t(clampi(y, 0, h - 1)) * uint32_t(w) + uint32_t(clampi(x, 0, w - 1))];
}

// meshlet_render.h:41-48
GR_HD Vec3 view_transform_yz_flip(const Frustum &f, const Vec3 &p)
{
	float v[3];
	for (int i = 0; i < 3; i++)
		v[i] = f.view[0][i] * p.x + f.view[1][i] * p.y + f.view[2][i] * p.z + f.view[3][i] * 1.0f;
	return {v[0], -v[1], -v[2]};
}

// meshlet_render.h:51-90
GR_HD bool hiz_cull(const CullArgs &a, float lo_x, float hi_x, float lo_y, float hi_y, float closest_z)
{
	const Frustum &f = a.frustum;
	const float rx0 = lo_x * f.viewport_scale_bias[0] + f.viewport_scale_bias[2], rx1 = hi_x * f.viewport_scale_bias[0] + f.viewport_scale_bias[2];
	const float ry0 = lo_y * f.viewport_scale_bias[1] + f.viewport_scale_bias[3], ry1 = hi_y * f.viewport_scale_bias[1] + f.viewport_scale_bias[3];
	int ix0 = float_to_int(rx0), ix1 = float_to_int(rx1), iy0 = float_to_int(ry0), iy1 = float_to_int(ry1);
	ix0 = glsl_clampi(ix0, 0, f.hiz_resolution[0] - 1);
	ix1 = glsl_clampi(ix1, ix0, f.hiz_resolution[0] - 1);
	iy0 = glsl_clampi(iy0, 0, f.hiz_resolution[1] - 1);
	iy1 = glsl_clampi(iy1, iy0, f.hiz_resolution[1] - 1);

	const int dx = ix1 - ix0, dy = iy1 - iy0;
	const int max_delta = dx > dy ? dx : dy;
	int lod = glsl_clampi(find_msb(max_delta - 1) + 1, f.hiz_min_lod, f.hiz_max_lod);
	lod = clampi(lod, 0, 30); // a shift count, whatever the block holds
	const int mx = (f.hiz_resolution[0] >> lod) > 1 ? (f.hiz_resolution[0] >> lod) - 1 : 0;
	const int my = (f.hiz_resolution[1] >> lod) > 1 ? (f.hiz_resolution[1] >> lod) - 1 : 0;
	ix0 = (ix0 >> lod) < mx ? (ix0 >> lod) : mx;
	ix1 = (ix1 >> lod) < mx ? (ix1 >> lod) : mx;
	iy0 = (iy0 >> lod) < my ? (iy0 >> lod) : my;
	iy1 = (iy1 >> lod) < my ? (iy1 >> lod) : my;

	lod -= f.hiz_min_lod; // the top LOD was not written
	float d = hiz_texel(a, ix0, iy0, lod);
	const bool nx = ix1 != ix0, ny = iy1 != iy0;
	if (nx)
		d = fmaxf(d, hiz_texel(a, ix0 + 1, iy0, lod));
	if (ny)
		d = fmaxf(d, hiz_texel(a, ix0, iy0 + 1, lod));
	if (nx && ny)
		d = fmaxf(d, hiz_texel(a, ix0 + 1, iy0 + 1, lod));
	return closest_z < d;
}

// meshlet_render.h:93-103
GR_HD void project_sphere_flat(float view_xy, float view_z, float radius, float &lo, float &hi)
{
	const float len = sqrtf(view_xy * view_xy + view_z * view_z);
	const float sin_xy = radius / len;
	const float cos_xy = sqrtf(1.0f - sin_xy * sin_xy);
	const float lo_x = cos_xy * view_xy + (-sin_xy) * view_z, lo_y = sin_xy * view_xy + cos_xy * view_z;
	const float hi_x = cos_xy * view_xy + sin_xy * view_z, hi_y = (-sin_xy) * view_xy + cos_xy * view_z;
	lo = lo_x / lo_y;
	hi = hi_x / hi_y;
}

// meshlet_render.h:108-135
template <bool ORTHO> GR_HD bool cluster_cull_hiz(const CullArgs &a, const Vec3 &center, float radius)
{
	const Vec3 view = view_transform_yz_flip(a.frustum, center);
	// no clipping against the near plane: a sphere close enough is accepted; ORTHO has no effective near plane
	if (!(ORTHO || view.z > radius + 0.1f))
		return true;
	float x0, x1, y0, y1;
	if (ORTHO)
	{
		x0 = view.x + (-radius);
		x1 = view.x + radius;
		y0 = view.y + (-radius);
		y1 = view.y + radius;
	}
	else
	{
		project_sphere_flat(view.x, view.z, radius, x0, x1);
		project_sphere_flat(view.y, view.z, radius, y0, y1);
	}
	return hiz_cull(a, x0, x1, y0, y1, view.z - radius);
}

// meshlet_render.h:138-174
template <int PHASE, bool ORTHO> GR_HD bool cluster_cull(const CullArgs &a, const Affine &m, const Bound &b)
{
	const Vec3 c = {b.center_radius[0], b.center_radius[1], b.center_radius[2]};
	const Vec3 center = {dot_point(c, m.rows[0]), dot_point(c, m.rows[1]), dot_point(c, m.rows[2])};
	float s[3];
	for (int j = 0; j < 3; j++)
		s[j] = m.rows[0][j] * m.rows[0][j] + m.rows[1][j] * m.rows[1][j] + m.rows[2][j] * m.rows[2][j];
	const float radius = b.center_radius[3] * sqrtf(fmaxf(fmaxf(s[0], s[1]), s[2]));

	if (b.cone[3] < 1.0f)
	{
		const Vec3 axis = {b.cone[0], b.cone[1], b.cone[2]};
		const Vec3 t = {dot3(axis, {m.rows[0][0], m.rows[0][1], m.rows[0][2]}), dot3(axis, {m.rows[1][0], m.rows[1][1], m.rows[1][2]}),
		                dot3(axis, {m.rows[2][0], m.rows[2][1], m.rows[2][2]})};
		const float len = sqrtf(dot3(t, t));
		const Vec3 n = {t.x / len, t.y / len, t.z / len};
		const Vec3 d = {center.x - a.camera_position[0], center.y - a.camera_position[1], center.z - a.camera_position[2]};
		if (!(dot3(d, n) <= b.cone[3] * sqrtf(dot3(d, d)) + radius))
			return false;
	}
	for (int i = 0; i < 6; i++)
		if (dot_point(center, a.frustum.planes[i]) < -radius)
			return false;
	if (PHASE == 2)
		return cluster_cull_hiz<ORTHO>(a, center, radius);
	return true;
}

// meshlet_render.h:176-195
template <int PHASE, bool ORTHO> GR_HD bool frustum_cull(const CullArgs &a, const AABB &box)
{
	for (int i = 0; i < 6; i++)
	{
		const float *p = a.frustum.planes[i];
		const Vec3 m = {p[0] > 0.0f ? box.hi[0] : box.lo[0], p[1] > 0.0f ? box.hi[1] : box.lo[1], p[2] > 0.0f ? box.hi[2] : box.lo[2]};
		if (dot_point(m, p) < 0.0f)
			return false;
	}
	if (PHASE == 2)
	{
		// very crude, but the only culling a skinned mesh gets
		const Vec3 c = {0.5f * (box.lo[0] + box.hi[0]), 0.5f * (box.lo[1] + box.hi[1]), 0.5f * (box.lo[2] + box.hi[2])};
		const Vec3 e = {box.hi[0] - box.lo[0], box.hi[1] - box.lo[1], box.hi[2] - box.lo[2]};
		return cluster_cull_hiz<ORTHO>(a, c, 0.5f * sqrtf(dot3(e, e)));
	}
	return true;
}

GR_HD uint32_t occluder_word(const CullArgs &a, uint32_t index) { return index < a.occluder_count ? a.occluders[index] : 0u; }
GR_HD void set_occluder_word(const CullArgs &a, uint32_t index, uint32_t value)
{
	if (index < a.occluder_count)
		a.occluders[index] = value;
}

// main() of meshlet_cull.comp up to its ballot, for the task at `flat_index` of the dispatch: does the task need work?  Phase 2 clears
// the occluder word of a task that does not.
template <int PHASE, bool ORTHO> GR_HD bool task_needs_work(const CullArgs &a, uint32_t flat_index)
{
	if (flat_index >= a.count)
		return false;
	const uint64_t task_index = uint64_t(a.offset) + flat_index;
	if (task_index >= a.task_count)
		return false;
	const Task task = a.tasks[task_index];
	const bool visible = task.aabb_instance < a.aabb_count && frustum_cull<PHASE, ORTHO>(a, a.aabbs[task.aabb_instance]);
	if (PHASE == 1)
		return visible && occluder_word(a, task.occluder_state_offset) != 0u;
	if (PHASE == 2 && !visible)
		set_occluder_word(a, task.occluder_state_offset, 0u);
	return visible;
}

// process_task() up to its first ballot, for chunk `lane` (0 .. 31) of a task that needs work: is the chunk visible now?
// old_state: the task's occluder word as it was (phases 1 and 2).
template <int PHASE, bool ORTHO, bool SKINNED> GR_HD bool chunk_visible(const CullArgs &a, const Task &task, uint32_t lane, uint32_t old_state, uint32_t &chunk)
{
	const uint32_t count = (task.mesh_index_count & 31u) + 1u;
	chunk = (task.mesh_index_count & ~31u) + lane;
	if (lane >= count || chunk >= a.draw_count)
		return false;
	if (PHASE == 1 && ((old_state >> lane) & 1u) == 0u)
		return false;
	if (SKINNED)
		return true;
	if (chunk >= a.bound_count || task.node_instance >= a.transform_count)
		return false;
	return cluster_cull<PHASE, ORTHO>(a, a.transforms[task.node_instance], a.bounds[chunk]);
}

// the record of a surviving chunk, five dwords at draw_indirect_offset + 5 * slot; not written where it would end past the buffer
GR_HD void write_draw(const CullArgs &a, uint32_t slot, uint32_t chunk, uint32_t task_index)
{
	const uint64_t at = uint64_t(a.draw_indirect_offset) + uint64_t(slot) * 5u;
	if (at + 5u > a.output_dwords)
		return;
	const Draw d = a.draws[chunk];
	uint32_t *o = a.output + at;
	o[0] = d.index_count;
	o[1] = 1u;
	o[2] = d.first_index;
	o[3] = uint32_t(d.vertex_offset);
	o[4] = task_index;
}
} // namespace gr_cull
