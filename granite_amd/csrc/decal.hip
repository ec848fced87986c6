// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Volumetric decals: assets/shaders/lights/clusterer_bindless_binning_decal.comp and lights/volumetric_decal.h as two gfx950 kernels.
// The per-lane arithmetic is decal_core.hpp's; this file holds the launch shapes, the cross-lane traffic and the launchers' refusals.
// Built with -ffp-contract=off (Makefile: EXACT_SRCS).
//
// k_cluster_binning_decal: one wave64 per (pair of 32-decal chunks, 8 x 8 cell tile).  Lane l computes the screen box of decal
// 64 * pair + l and tests it against the tile; the 64-bit ballot holds both chunks' 32-bit ballots of the shader's SUBGROUPS form.  The
// ballot is walked wave-uniformly: the box of the decal at the walked bit is read from its lane, every lane tests its own cell and sets
// the bit in the word of the chunk the decal belongs to.  The bits are the shader's; a decal's matrix is read once per tile.
//
// k_decal_apply: one wave64 per 8 x 8 pixel tile, lane = (y & 7) * 8 + (x & 7), so lane ^ 1 and lane ^ 8 are the partners of the aligned
// 2 x 2 quad.  Every lane masks its cell's bitmask word with its own slice's range (cluster_mask_range); the wave-wide OR of those words
// is the candidate set, walked as a scalar loop in ascending index order.  The decal's rows and texture record are wave-uniform loads.
// Every lane evaluates uv for every candidate; the quad partners' uv arrive by two cross-lane moves each.  A lane blends when the bit is
// in its OWN word and |uvw| < 0.5: the reference at subgroup size 1, which is what the stored reference results were recorded at (a
// wider subgroupOr can only add decals whose box the pixel is outside of up to the last bits of the binning's arithmetic).  A tile whose
// OR is empty has read depth, ranges and bitmask words only; only lanes that blended store.
#include "ctx.hpp"
#include "decal_core.hpp"
#include "device_common.hpp"

namespace
{
using namespace gr_decal;

__device__ __forceinline__ float lane_read(float v, int lane)
{
	return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

__global__ __launch_bounds__(64) void k_cluster_binning_decal(const float *__restrict__ mvps, uint32_t *__restrict__ bitmask, gr_cluster_params prm)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t chunk0 = blockIdx.x * 2u;
	const uint32_t tile_x = blockIdx.y, tile_y = blockIdx.z;
	const float inv_x = prm.inv_resolution_xy[0], inv_y = prm.inv_resolution_xy[1];
	const uint32_t num_decals = uint32_t(prm.num_decals), n32 = uint32_t(prm.num_decals_32);

	const uint32_t decal_index = 32u * chunk0 + lane;
	Vec4 bb = {1.0f, 1.0f, -1.0f, -1.0f};
	if (decal_index < num_decals)
		bb = compute_decal_screen_bb(mvps + size_t(decal_index) * 16u);
	const bool tile_passed = test_decal(cell_uv(tile_x * 8u, inv_x), cell_uv(tile_y * 8u, inv_y), (2.0f * 8.0f) * inv_x, (2.0f * 8.0f) * inv_y, bb);
	unsigned long long ballot = __ballot(tile_passed);

	const uint32_t px = tile_x * 8u + (lane & 7u), py = tile_y * 8u + (lane >> 3u);
	const float u = cell_uv(px, inv_x), v = cell_uv(py, inv_y);
	const float stride_u = 2.0f * inv_x, stride_v = 2.0f * inv_y;
	uint32_t mask_lo = 0u, mask_hi = 0u;
	while (ballot != 0ull)
	{
		const int bit = __builtin_ctzll(ballot);
		ballot &= ballot - 1ull;
		const Vec4 scalar_bb = {lane_read(bb.x, bit), lane_read(bb.y, bit), lane_read(bb.z, bit), lane_read(bb.w, bit)};
		const bool passed = test_decal(u, v, stride_u, stride_v, scalar_bb);
		// `bit` is wave-uniform: one of the two words, chosen on the scalar unit
		if (bit < 32)
			mask_lo |= passed ? 1u << bit : 0u;
		else
			mask_hi |= passed ? 1u << (bit - 32) : 0u;
	}
	const size_t base_index = (size_t(py) * uint32_t(prm.resolution_xy[0]) + px) * n32 + chunk0;
	bitmask[base_index] = mask_lo;
	if (chunk0 + 1u < n32)
		bitmask[base_index + 1u] = mask_hi;
}

struct ApplyArgs
{
	uint8_t *albedo;
	const uint8_t *depth;
	uint32_t width, height, albedo_pitch, depth_pitch;
	float inv_width, inv_height;
	float inv_vp[16];
	gr_cluster_params cluster;
	const float *decal_rows; // transforms + GR_TRANSFORMS_OFFSET_DECALS
	const uint32_t *bitmask;
	const uint2 *range;
	const Texture *textures;
	uint32_t num_textures;
	const float *srgb_decode;
	const uint2 *srgb_encode;
};

__global__ __launch_bounds__(64) void k_decal_apply(const ApplyArgs a)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t x = blockIdx.x * 8u + (lane & 7u), y = blockIdx.y * 8u + (lane >> 3u);
	const bool inside = x < a.width && y < a.height;
	float depth = 0.0f;
	if (inside)
		depth = *reinterpret_cast<const float *>(a.depth + size_t(y) * a.depth_pitch + size_t(x) * 4u);
	const bool active = inside && depth != 0.0f;
	const unsigned long long active_lanes = __ballot(active);
	if (active_lanes == 0ull)
		return;

	const gr_cluster_params &cl = a.cluster;
	const uint32_t num_decals = uint32_t(cl.num_decals), n32 = uint32_t(cl.num_decals_32);
	// an inactive lane keeps a finite position: its uv is shuffled to its partners, which do not use it
	const Vec3 pos = active ? world_position(a.inv_vp, x, y, a.inv_width, a.inv_height, depth) : Vec3{0.0f, 0.0f, 0.0f};
	uint2 z_range = make_uint2(0xffffffffu, 0u);
	size_t cluster_base = 0;
	if (active)
	{
		const int cx = cluster_cell(x, a.inv_width, cl.xy_scale[0], cl.resolution_xy[0]);
		const int cy = cluster_cell(y, a.inv_height, cl.xy_scale[1], cl.resolution_xy[1]);
		cluster_base = (size_t(cy) * uint32_t(cl.resolution_xy[0]) + uint32_t(cx)) * n32;
		z_range = a.range[z_slice(pos, cl.camera_base, cl.camera_front, cl.z_scale, cl.z_max_index)];
	}
	const uint32_t z_start = wave_min_u32(z_range.x) >> 5u;
	const uint32_t z_end = min(wave_max_u32(z_range.y) >> 5u, n32 - 1u);

	// the quad's two axes: both pixels of an axis inside the image and off the far plane, or the axis contributes 0
	const bool has_dx = active && ((active_lanes >> (lane ^ 1u)) & 1ull) != 0ull;
	const bool has_dy = active && ((active_lanes >> (lane ^ 8u)) & 1ull) != 0ull;
	const float sign_x = (lane & 1u) ? 1.0f : -1.0f, sign_y = (lane & 8u) ? 1.0f : -1.0f; // uv(x | 1) - uv(x & ~1): this lane is one of the two

	Vec3 base = {0.0f, 0.0f, 0.0f};
	uint32_t texel = 0u;
	bool touched = false;

	for (uint32_t i = z_start; i <= z_end && z_start <= z_end; i++)
	{
		uint32_t own = 0u;
		if (active)
			own = cluster_mask_range(a.bitmask[cluster_base + i], z_range.x, z_range.y, 32u * i);
		uint32_t candidates = uint32_t(__builtin_amdgcn_readfirstlane(int(wave_or(own))));
		while (candidates != 0u)
		{
			const uint32_t bit = uint32_t(__builtin_ctz(candidates));
			candidates &= candidates - 1u;
			const uint32_t index = 32u * i + bit;
			const uint32_t texture_index = uint32_t(cl.decals_texture_offset) + index;
			if (index >= num_decals || texture_index >= a.num_textures)
				continue;
			const Vec3 uvw = decal_uvw(a.decal_rows + size_t(index) * 12u, pos);
			const float u = uvw.x + 0.5f, v = uvw.y + 0.5f;
			const float u_dx = __shfl_xor(u, 1, 64), v_dx = __shfl_xor(v, 1, 64);
			const float u_dy = __shfl_xor(u, 8, 64), v_dy = __shfl_xor(v, 8, 64);
			if (!(((own >> bit) & 1u) != 0u && uvw_in_range(uvw)))
				continue;
			const float dudx = has_dx ? sign_x * (u - u_dx) : 0.0f, dvdx = has_dx ? sign_x * (v - v_dx) : 0.0f;
			const float dudy = has_dy ? sign_y * (u - u_dy) : 0.0f, dvdy = has_dy ? sign_y * (v - v_dy) : 0.0f;
			const Texture tex = a.textures[texture_index];
			const float lambda = texture_lod(dudx, dvdx, dudy, dvdy, tex.width, tex.height, tex.num_levels);
			const Vec4 colour = sample_texture(tex, u, v, lambda, a.srgb_decode);
			if (!touched)
			{
				texel = *reinterpret_cast<const uint32_t *>(a.albedo + size_t(y) * a.albedo_pitch + size_t(x) * 4u);
				base = {a.srgb_decode[texel & 255u], a.srgb_decode[(texel >> 8) & 255u], a.srgb_decode[(texel >> 16) & 255u]};
				touched = true;
			}
			base = blend_decal(base, colour);
		}
	}
	if (touched)
	{
		const uint32_t out = encode_srgb8_lut(base.x, a.srgb_encode) | (encode_srgb8_lut(base.y, a.srgb_encode) << 8) |
		                     (encode_srgb8_lut(base.z, a.srgb_encode) << 16) | (texel & 0xff000000u);
		*reinterpret_cast<uint32_t *>(a.albedo + size_t(y) * a.albedo_pitch + size_t(x) * 4u) = out;
	}
}

int check_cluster_block(gr_ctx *ctx, const char *fn, const gr_cluster_params &p)
{
	if (p.resolution_xy[0] <= 0 || p.resolution_xy[1] <= 0 || (p.resolution_xy[0] & 7) != 0 || (p.resolution_xy[1] & 7) != 0)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: resolution_xy %d x %d is not a positive multiple of 8 each way", fn, p.resolution_xy[0],
		                 p.resolution_xy[1]);
	if (p.num_decals < 0 || p.num_decals > GR_MAX_DECALS_BINDLESS)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: num_decals %d is not 0 .. %d", fn, p.num_decals, GR_MAX_DECALS_BINDLESS);
	if (p.num_decals_32 != (p.num_decals + 31) / 32)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: num_decals_32 %d is not ceil(num_decals %d / 32)", fn, p.num_decals_32, p.num_decals);
	return GR_OK;
}
} // namespace

extern "C" {

int gr_cluster_binning_decal(gr_ctx *ctx, gr_stream stream, const float *mvps, uint32_t *bitmask, const gr_cluster_params *params)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, params);
	if (const int status = check_cluster_block(ctx, __func__, *params))
		return status;
	if (params->num_decals == 0)
		return GR_OK;
	GR_CHECK_ARG(ctx, mvps);
	GR_CHECK_ARG(ctx, bitmask);
	const dim3 grid(gr_div_up(unsigned(params->num_decals_32), 2u), unsigned(params->resolution_xy[0]) / 8u, unsigned(params->resolution_xy[1]) / 8u);
	gr_scoped_timing timing{ctx, gr_to_stream(stream), "cluster_binning_decal"};
	hipLaunchKernelGGL(k_cluster_binning_decal, grid, dim3(64), 0, gr_to_stream(stream), mvps, bitmask, *params);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

int gr_decal_apply(gr_ctx *ctx, gr_stream stream, const gr_decal_apply_args *args)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, args);
	GR_CHECK_IMAGE(ctx, &args->albedo, gr_format_set(GR_FORMAT_R8G8B8A8_SRGB));
	GR_CHECK_IMAGE(ctx, &args->depth, gr_format_set(GR_FORMAT_D32_SFLOAT), args->albedo.width, args->albedo.height);
	if (const int status = check_cluster_block(ctx, __func__, args->cluster))
		return status;
	if (args->cluster.z_max_index < 0)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: cluster.z_max_index %d is negative", __func__, args->cluster.z_max_index);
	if (args->cluster.num_decals == 0)
		return GR_OK;
	GR_CHECK_ARG(ctx, args->transforms);
	GR_CHECK_ARG(ctx, args->bitmask_decal);
	GR_CHECK_ARG(ctx, args->range_decal);
	GR_CHECK_ARG(ctx, args->textures);

	ApplyArgs a = {};
	a.albedo = static_cast<uint8_t *>(args->albedo.ptr);
	a.depth = static_cast<const uint8_t *>(args->depth.ptr);
	a.width = args->albedo.width;
	a.height = args->albedo.height;
	a.albedo_pitch = args->albedo.pitch_bytes;
	a.depth_pitch = args->depth.pitch_bytes;
	a.inv_width = 1.0f / float(a.width);
	a.inv_height = 1.0f / float(a.height);
	memcpy(a.inv_vp, args->inv_view_projection, sizeof(a.inv_vp));
	a.cluster = args->cluster;
	a.decal_rows = reinterpret_cast<const float *>(static_cast<const uint8_t *>(args->transforms) + GR_TRANSFORMS_OFFSET_DECALS);
	a.bitmask = args->bitmask_decal;
	a.range = reinterpret_cast<const uint2 *>(args->range_decal);
	static_assert(sizeof(Texture) == sizeof(gr_decal_texture), "decal_core.hpp's Texture is gr_decal_texture");
	a.textures = reinterpret_cast<const Texture *>(args->textures);
	a.num_textures = args->num_textures;
	a.srgb_decode = ctx->srgb_decode_lut;
	a.srgb_encode = ctx->srgb_encode_lut;

	const dim3 grid(gr_div_up(a.width, 8u), gr_div_up(a.height, 8u));
	gr_scoped_timing timing{ctx, gr_to_stream(stream), "decal_apply"};
	hipLaunchKernelGGL(k_decal_apply, grid, dim3(64), 0, gr_to_stream(stream), a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
}
