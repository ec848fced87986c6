// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen; lights/atmospheric_scatter.h also (c) 2019 Dimas Leenman):
// see THIRD_PARTY_NOTICES.md at the repository root.
// The sky pass: skybox.vert / skybox.frag on the pixels the G-buffer left at the far plane, and lights/volumetric_light_setup_sky.comp.
// The per-pixel arithmetic is sky_core.hpp's; this file holds the launch shapes and the launchers' refusals.  Built with
// -ffp-contract=off (Makefile: EXACT_SRCS).
//
// k_sky_apply: a workgroup of four wave64 per 16 x 16 pixel tile.  Every lane reads its pixel's depth; a tile without a far pixel has read
// depth only and leaves.  Otherwise the tile's far pixels are compacted: each wave's ballot is counted, the four counts go through LDS, and
// a far lane writes its pixel's index (0 .. 255) at (far pixels of earlier waves) + (far lanes below it in its own wave).  After the barrier
// thread i takes the i-th far pixel, so the march runs in ceil(far / 64) full waves and one partial one whatever the far pixels' pattern
// is, and the other waves of the workgroup end.  Nothing a pixel computes needs a neighbour (the cube LOD is formed from pixel positions),
// so compaction needs no cross-lane traffic afterwards.  What compaction does not remove: lanes whose ray hits the earth return 0 at once
// and idle while their wave marches (a horizon inside a wave).  The plain form (lane = pixel, no list) was not built.
//
// k_sky_cube: one lane per texel of a face, wave64 workgroups, blockIdx.y the face: a 32-texel cube is 96 waves of 32 x 16 steps a texel,
// and small workgroups spread them over the CUs.
#include "ctx.hpp"
#include "device_common.hpp"
#include "packed_float.hpp"
#include "sky_core.hpp"

namespace
{
using namespace gr_sky;

constexpr uint32_t TILE = 16u, GROUP = TILE * TILE, WAVES = GROUP / 64u;

struct ApplyArgs
{
	uint8_t *emissive;
	const uint8_t *depth;
	uint32_t width, height, emissive_pitch, depth_pitch;
	float inv[16];
	float color[3], camera_height;
	float sun_direction[3];
	gr_env::Cube cube;
};

template <bool PACKED, bool TEXTURED>
__global__ __launch_bounds__(GROUP) void k_sky_apply(const ApplyArgs a)
{
	__shared__ uint32_t wave_far[WAVES];
	__shared__ uint8_t far_list[GROUP];

	const uint32_t tid = threadIdx.x, wave = tid >> 6u;
	const uint32_t tile_x = blockIdx.x * TILE, tile_y = blockIdx.y * TILE;
	{
		const uint32_t x = tile_x + (tid & (TILE - 1u)), y = tile_y + tid / TILE;
		bool is_far = false;
		if (x < a.width && y < a.height)
			is_far = *reinterpret_cast<const float *>(a.depth + size_t(y) * a.depth_pitch + size_t(x) * 4u) == 0.0f;
		const unsigned long long ballot = __ballot(is_far);
		if ((tid & 63u) == 0u)
			wave_far[wave] = uint32_t(__builtin_popcountll(ballot));
		__syncthreads();
		uint32_t before = 0u, total = 0u;
		for (uint32_t w = 0; w < WAVES; w++)
		{
			const uint32_t n = wave_far[w];
			before += w < wave ? n : 0u;
			total += n;
		}
		if (total == 0u)
			return;
		if (is_far)
			far_list[before + __builtin_amdgcn_mbcnt_hi(uint32_t(ballot >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(ballot), 0u))] = uint8_t(tid);
		__syncthreads();
		if (tid >= total)
			return;
	}
	const uint32_t pixel = far_list[tid];
	const uint32_t x = tile_x + (pixel & (TILE - 1u)), y = tile_y + pixel / TILE;

	f3 rgb;
	if constexpr (TEXTURED)
		rgb = sky_textured(a.cube, a.inv, a.width, a.height, x, y, a.color);
	else
		rgb = sky_procedural(pixel_direction(a.inv, a.width, a.height, x, y), a.color, a.sun_direction, a.camera_height);

	if constexpr (PACKED)
		*reinterpret_cast<uint32_t *>(a.emissive + size_t(y) * a.emissive_pitch + size_t(x) * 4u) = pack_b10g11r11(rgb.x, rgb.y, rgb.z);
	else
	{
		// r, g and b: alpha's two bytes are not stored to
		uint8_t *texel = a.emissive + size_t(y) * a.emissive_pitch + size_t(x) * 8u;
		*reinterpret_cast<uint32_t *>(texel) = gr_core::float_to_half(rgb.x) | (gr_core::float_to_half(rgb.y) << 16);
		*reinterpret_cast<uint16_t *>(texel + 4) = uint16_t(gr_core::float_to_half(rgb.z));
	}
}

struct CubeArgs
{
	uint2 *out;
	uint32_t size;
	float inv_resolution;
	float sun_color[3], camera_y;
	float sun_direction[3];
};

__global__ __launch_bounds__(64) void k_sky_cube(const CubeArgs a)
{
	const uint32_t index = blockIdx.x * 64u + threadIdx.x, face = blockIdx.y;
	if (index >= a.size * a.size)
		return;
	const uint32_t x = index % a.size, y = index / a.size;
	const f3 rgb = sky_cube_texel(face, x, y, a.inv_resolution, a.sun_color, a.sun_direction, a.camera_y);
	a.out[size_t(face) * a.size * a.size + index] = gr_env::pack_rgba(rgb, 1.0f);
}

constexpr uint32_t MAX_CUBE_SIZE = 16384u; // as environment.hip: 6 n^2 texel indices stay below 2^32
} // namespace

extern "C" {

int gr_sky_apply(gr_ctx *ctx, gr_stream stream, const gr_sky_args *args)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, args);
	GR_CHECK_IMAGE(ctx, &args->emissive, GR_HDR_FORMATS);
	GR_CHECK_IMAGE(ctx, &args->depth, gr_format_set(GR_FORMAT_D32_SFLOAT), args->emissive.width, args->emissive.height);
	const gr_cube &cube = args->cube;
	const bool textured = cube.ptr || cube.size || cube.levels;
	if (textured)
	{
		if (!cube.ptr)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: cube.ptr is a null pointer (size %u, levels %u)", __func__, cube.size, cube.levels);
		if (cube.size == 0 || cube.size > MAX_CUBE_SIZE)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: cube.size %u is outside 1 .. %u", __func__, cube.size, MAX_CUBE_SIZE);
		if (cube.levels == 0 || cube.levels > gr_env::full_chain_levels(cube.size))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: cube.levels %u are beyond the chain of size %u (1 .. %u)", __func__, cube.levels,
			                 cube.size, gr_env::full_chain_levels(cube.size));
		if (reinterpret_cast<uintptr_t>(cube.ptr) & 15u)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: cube.ptr is not 16-byte aligned", __func__);
	}

	ApplyArgs a = {};
	a.emissive = static_cast<uint8_t *>(args->emissive.ptr);
	a.depth = static_cast<const uint8_t *>(args->depth.ptr);
	a.width = args->emissive.width;
	a.height = args->emissive.height;
	a.emissive_pitch = args->emissive.pitch_bytes;
	a.depth_pitch = args->depth.pitch_bytes;
	memcpy(a.inv, args->inv_local_view_projection, sizeof(a.inv));
	memcpy(a.color, args->color, sizeof(a.color));
	a.camera_height = args->camera_height;
	memcpy(a.sun_direction, args->sun_direction, sizeof(a.sun_direction));
	a.cube = {static_cast<const uint8_t *>(cube.ptr), cube.size, cube.levels};

	const dim3 grid(gr_div_up(a.width, TILE), gr_div_up(a.height, TILE));
	const bool packed = args->emissive.format == GR_FORMAT_B10G11R11_UFLOAT_PACK32;
	gr_scoped_timing timing{ctx, gr_to_stream(stream), "sky_apply"};
	with_flags([&](auto is_packed, auto is_textured) {
		hipLaunchKernelGGL((k_sky_apply<decltype(is_packed)::value, decltype(is_textured)::value>), grid, dim3(GROUP), 0, gr_to_stream(stream), a);
	}, packed, textured);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

int gr_sky_cube(gr_ctx *ctx, gr_stream stream, void *out_chain, uint32_t size, const gr_sky_cube_params *params)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, out_chain);
	GR_CHECK_ARG(ctx, params);
	if (size == 0 || size > MAX_CUBE_SIZE)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: size %u is outside 1 .. %u", __func__, size, MAX_CUBE_SIZE);
	if (reinterpret_cast<uintptr_t>(out_chain) & 15u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: out_chain is not 16-byte aligned", __func__);

	CubeArgs a = {};
	a.out = static_cast<uint2 *>(out_chain);
	a.size = size;
	a.inv_resolution = 1.0f / float(size);
	memcpy(a.sun_color, params->sun_color, sizeof(a.sun_color));
	a.camera_y = params->camera_y;
	memcpy(a.sun_direction, params->sun_direction, sizeof(a.sun_direction));

	gr_scoped_timing timing{ctx, gr_to_stream(stream), "sky_cube"};
	hipLaunchKernelGGL(k_sky_cube, dim3(gr_div_up(size * size, 64u), 6u), dim3(64), 0, gr_to_stream(stream), a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
}
