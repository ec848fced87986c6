// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The compute work of Ocean::update_fft_pass (renderer/ocean.cpp) apart from the FFTs and the single-pass downsampler: the dispatches of
// ocean/generate_fft.comp, ocean/bake_maps.comp and ocean/mipmap.comp, one launch each.  The arithmetic is ocean_core.hpp's; this file
// adds the mapping of bins and texels to lanes and the argument checks.  Built with -ffp-contract=off (Makefile: EXACT_SRCS).
//
//   k_ocean_generate  one lane per bin, rows along x: a wave reads 64 consecutive float2 of its row and the 64 consecutive float2 of
//                     the mirrored row backwards -- whole 128-byte lines either way -- and stores 64 consecutive half2.
//   k_ocean_bake      one lane per texel of the height map, rows along x; the taps at texel centres snap to single texels.
//   k_ocean_mipmap    one lane per output texel, rows along x; four texels a tap.
//
// And that of Ocean::update_lod_pass: ocean/update_lod.comp, ocean/init_counter_buffer.comp and ocean/cull_blocks.comp, one launch each,
// one wave64 per 8 x 8 group of the shaders.
//   k_ocean_update_lod    one lane per block of the grid; one fp16 store each.
//   k_ocean_init_counters one lane per dword of the eight draw records.
//   k_ocean_cull          one lane per block.  The append is aggregated per wave: per LOD present in the wave one ballot, one
//                         agent-scope add of the lane count by the first lane, each lane's slot from its rank in the ballot.
#include "ctx.hpp"
#include "ocean_core.hpp"

namespace
{
using namespace gr_ocean;
constexpr uint32_t GROUP = 256u;

struct GenerateLaunch
{
	const float2 *distribution;
	uint32_t *out;
	uint32_t log2_nx;
	GenerateArgs g;
};

__global__ __launch_bounds__(GROUP) void k_ocean_generate(GenerateLaunch a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x;
	if (index >= a.g.nx * a.g.ny)
		return;
	const uint32_t x = index & (a.g.nx - 1u), y = index >> a.log2_nx;
	const uint32_t wx = (a.g.nx - x) & (a.g.nx - 1u), wy = (a.g.ny - y) & (a.g.ny - 1u);
	const float2 p = a.distribution[index], q = a.distribution[wy * a.g.nx + wx];
	a.out[index] = generate_bin(a.g, x, y, {p.x, p.y}, {q.x, q.y});
}

struct BakeLaunch
{
	BakeArgs b;
	uint8_t *grad_jacobian, *height_displacement; // RGBA16F; height_displacement may be null
	uint32_t grad_pitch, hd_pitch;
	uint32_t width, height;
};

__global__ __launch_bounds__(GROUP) void k_ocean_bake(BakeLaunch a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x;
	if (index >= a.width * a.height)
		return;
	const uint32_t y = index / a.width, x = index - y * a.width;
	uint2_bits hd, gj;
	bake_texel(a.b, x, y, hd, gj);
	*reinterpret_cast<uint2 *>(a.grad_jacobian + size_t(y) * a.grad_pitch + size_t(x) * 8u) = make_uint2(gj.x, gj.y);
	if (a.height_displacement)
		*reinterpret_cast<uint2 *>(a.height_displacement + size_t(y) * a.hd_pitch + size_t(x) * 8u) = make_uint2(hd.x, hd.y);
}

struct MipmapLaunch
{
	MipmapArgs m;
	uint8_t *out;
	uint32_t out_pitch;
};

template <int C> __global__ __launch_bounds__(GROUP) void k_ocean_mipmap(MipmapLaunch a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x;
	if (index >= a.m.count_x * a.m.count_y)
		return;
	const uint32_t y = index / a.m.count_x, x = index - y * a.m.count_x;
	uint16_t texel[C];
	mipmap_texel<C>(a.m, x, y, texel);
	uint8_t *at = a.out + size_t(y) * a.out_pitch + size_t(x) * (2u * C);
	if constexpr (C == 1)
		*reinterpret_cast<uint16_t *>(at) = texel[0];
	else if constexpr (C == 2)
		*reinterpret_cast<uint32_t *>(at) = uint32_t(texel[0]) | (uint32_t(texel[1]) << 16);
	else
		*reinterpret_cast<uint2 *>(at) = make_uint2(uint32_t(texel[0]) | (uint32_t(texel[1]) << 16), uint32_t(texel[2]) | (uint32_t(texel[3]) << 16));
}

bool power_of_two(uint32_t v) { return v != 0 && (v & (v - 1u)) == 0; }
uint32_t log2_of(uint32_t v)
{
	uint32_t l = 0;
	while (v >>= 1)
		l++;
	return l;
}
// What both image entry points ask of an image beyond the contract: texel indices stay below 2^31.
constexpr uint32_t MAX_EXTENT = 32768u;

// ---- the LOD update ------------------------------------------------------------------------------------------------------------
constexpr uint32_t TILE = 8u; // the shaders' 8 x 8 group: one wave64

struct UpdateLodLaunch
{
	UpdateLodArgs u;
	uint8_t *out;
	uint32_t pitch;
};

__global__ __launch_bounds__(TILE * TILE) void k_ocean_update_lod(UpdateLodLaunch a)
{
	const int x = int(blockIdx.x * TILE + (threadIdx.x & (TILE - 1u))), y = int(blockIdx.y * TILE + threadIdx.x / TILE);
	if (x >= a.u.n || y >= a.u.n)
		return;
	int ix, iy;
	const uint16_t bits = update_lod_texel(a.u, x, y, ix, iy); // ix, iy < n: the image is n x n
	*reinterpret_cast<uint16_t *>(a.out + size_t(iy) * a.pitch + size_t(ix) * 2u) = bits;
}

struct InitCountersLaunch
{
	uint32_t *draws;
	uint32_t counts[MAX_LOD_INDIRECT];
};

__global__ __launch_bounds__(64) void k_ocean_init_counters(InitCountersLaunch a)
{
	const uint32_t word = threadIdx.x; // 8 records of 8 dwords
	a.draws[word] = (word & 7u) == 0u ? a.counts[word >> 3] : 0u;
}

struct CullLaunch
{
	CullArgs c;
	Patch *patches;
	uint32_t *draws;
	uint32_t num_lods; // int(max_lod) + 1
};

__global__ __launch_bounds__(TILE * TILE) void k_ocean_cull(CullLaunch a)
{
	const uint32_t lane = threadIdx.x;
	const int x = int(blockIdx.x * TILE + (lane & (TILE - 1u))), y = int(blockIdx.y * TILE + lane / TILE);
	Patch patch = {};
	int lod = -1; // no lane leaves before the ballots
	if (x < a.c.n && y < a.c.n && box_in_frustum(a.c, x, y))
		lod = cull_patch(a.c, x, y, patch);
	for (uint32_t l = 0; l < a.num_lods; l++)
	{
		const unsigned long long mask = __ballot(lod == int(l));
		if (mask == 0ull)
			continue;
		const uint32_t first = uint32_t(__ffsll(mask)) - 1u;
		uint32_t base = 0;
		if (lane == first)
			base = __hip_atomic_fetch_add(&a.draws[l * 8u + 1u], uint32_t(__popcll(mask)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		base = uint32_t(__shfl(int(base), int(first)));
		if (lod == int(l))
		{
			const uint32_t slot = base + uint32_t(__popcll(mask & ((1ull << lane) - 1ull)));
			if (slot < a.c.lod_stride) // holds whenever the counters began at init_counter_buffer's zero
				a.patches[size_t(a.c.lod_stride) * l + slot] = patch;
		}
	}
}

// What the three entry points ask of num_threads and max_lod; the text of the rule broken, or nullptr.
const char *grid_rule(int32_t nx, int32_t ny, float max_lod)
{
	if (nx != ny)
		return "num_threads is not square";
	if (nx < 4 || nx > 128 || !power_of_two(uint32_t(nx)))
		return "num_threads is not a power of two in 4 .. 128";
	if (!(max_lod >= 0.0f && max_lod <= float(MAX_LOD_INDIRECT - 1u)) || max_lod != floorf(max_lod))
		return "max_lod is not an integer in 0 .. 7";
	return nullptr;
}

Texture texture_of(const gr_image *img) { return {static_cast<const uint8_t *>(img->ptr), int(img->width), int(img->height), img->pitch_bytes}; }
} // namespace

extern "C" int gr_ocean_generate_fft(gr_ctx *ctx, gr_stream stream, const void *distribution, void *out, const gr_push_ocean_generate *push,
                                     uint32_t variant, const float *freq_bands)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, distribution);
	GR_CHECK_ARG(ctx, out);
	GR_CHECK_ARG(ctx, push);
	const uint32_t nx = push->N[0], ny = push->N[1];
	if (!power_of_two(nx) || !power_of_two(ny))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: N = %u x %u is not a power of two each way", nx, ny);
	if (nx < 64u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: N.x = %u is below 64 (the shader dispatches N.x / 64 groups a row)", nx);
	if (uint64_t(nx) * ny >= (1ull << 31))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: N = %u x %u has 2^31 bins or more", nx, ny);
	if (!(push->period > 0.0f))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: period %g is not positive", double(push->period));
	if (variant >= VARIANT_COUNT)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: unknown variant %u", variant);
	if ((reinterpret_cast<uintptr_t>(distribution) & 7u) || (reinterpret_cast<uintptr_t>(out) & 3u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: distribution is not 8-byte or out is not 4-byte aligned");
	if (gr_images_overlap(distribution, size_t(nx) * ny * 8u, out, size_t(nx) * ny * 4u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: out overlaps distribution");

	GenerateLaunch a = {};
	a.distribution = static_cast<const float2 *>(distribution);
	a.out = static_cast<uint32_t *>(out);
	a.log2_nx = log2_of(nx);
	a.g.mod_x = push->mod_factor[0];
	a.g.mod_y = push->mod_factor[1];
	a.g.nx = nx;
	a.g.ny = ny;
	a.g.freq_to_band_mod = push->freq_to_band_mod;
	a.g.time = push->time;
	a.g.period = push->period;
	a.g.variant = variant;
	a.g.use_bands = freq_bands ? 1u : 0u;
	if (freq_bands)
		memcpy(a.g.bands, freq_bands, sizeof(a.g.bands));
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_generate_fft"};
	hipLaunchKernelGGL(k_ocean_generate, dim3(gr_div_up(nx * ny, GROUP)), dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_ocean_bake_maps(gr_ctx *ctx, gr_stream stream, const gr_image *height, const gr_image *displacement, const gr_image *grad_jacobian,
                                  const gr_image *height_displacement, const gr_push_ocean_bake *push)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, push);
	GR_CHECK_IMAGE(ctx, height, GR_FORMAT_R16_SFLOAT);
	GR_CHECK_IMAGE(ctx, displacement, GR_FORMAT_R16G16_SFLOAT);
	GR_CHECK_IMAGE(ctx, grad_jacobian, GR_FORMAT_R16G16B16A16_SFLOAT);
	if (height_displacement)
		GR_CHECK_IMAGE(ctx, height_displacement, GR_FORMAT_R16G16B16A16_SFLOAT);
	GR_CHECK_ARG(ctx, height->width <= MAX_EXTENT && height->height <= MAX_EXTENT); // (the outputs have the height map's size, below)
	GR_CHECK_ARG(ctx, displacement->width <= MAX_EXTENT && displacement->height <= MAX_EXTENT);
	if (!power_of_two(displacement->width) || !power_of_two(displacement->height))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_bake_maps: displacement %u x %u is not a power of two each way", displacement->width, displacement->height);
	if (grad_jacobian->width != height->width || grad_jacobian->height != height->height ||
	    (height_displacement && (height_displacement->width != height->width || height_displacement->height != height->height)))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_bake_maps: the outputs do not have the height map's size %u x %u", height->width, height->height);
	for (const gr_image *o : {grad_jacobian, height_displacement})
		if (o && (gr_images_overlap(o, height) || gr_images_overlap(o, displacement) || (o == height_displacement && gr_images_overlap(o, grad_jacobian))))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_bake_maps: %s overlaps an input or the other output", o == grad_jacobian ? "grad_jacobian" : "height_displacement");

	BakeLaunch a = {};
	a.b.height = texture_of(height);
	a.b.displacement = texture_of(displacement);
	memcpy(a.b.inv_size, push->inv_size, sizeof(a.b.inv_size));
	memcpy(a.b.scale, push->scale, sizeof(a.b.scale));
	a.grad_jacobian = static_cast<uint8_t *>(grad_jacobian->ptr);
	a.grad_pitch = grad_jacobian->pitch_bytes;
	a.height_displacement = height_displacement ? static_cast<uint8_t *>(height_displacement->ptr) : nullptr;
	a.hd_pitch = height_displacement ? height_displacement->pitch_bytes : 0u;
	a.width = height->width;
	a.height = height->height;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_bake_maps"};
	hipLaunchKernelGGL(k_ocean_bake, dim3(gr_div_up(a.width * a.height, GROUP)), dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_ocean_mipmap(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, const gr_push_ocean_mipmap *push)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, push);
	constexpr gr_format_set half_floats{GR_FORMAT_R16_SFLOAT, GR_FORMAT_R16G16_SFLOAT, GR_FORMAT_R16G16B16A16_SFLOAT};
	GR_CHECK_IMAGE(ctx, in, half_floats);
	GR_CHECK_IMAGE(ctx, out, in->format);
	const uint32_t channels = gr_format_texel_bytes(in->format) / 2u;
	GR_CHECK_ARG(ctx, in->width <= MAX_EXTENT && in->height <= MAX_EXTENT);
	GR_CHECK_ARG(ctx, out->width <= MAX_EXTENT && out->height <= MAX_EXTENT);
	if (out->width != push->count[0] || out->height != push->count[1])
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_mipmap: out is %u x %u, count says %u x %u", out->width, out->height, push->count[0], push->count[1]);
	if (gr_images_overlap(in, out))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_mipmap: out overlaps in");

	MipmapLaunch a = {};
	a.m.in = texture_of(in);
	memcpy(a.m.result_mod, push->result_mod, sizeof(a.m.result_mod));
	memcpy(a.m.inv_resolution, push->inv_resolution, sizeof(a.m.inv_resolution));
	a.m.count_x = push->count[0];
	a.m.count_y = push->count[1];
	a.out = static_cast<uint8_t *>(out->ptr);
	a.out_pitch = out->pitch_bytes;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_mipmap"};
	const dim3 grid(gr_div_up(a.m.count_x * a.m.count_y, GROUP));
	if (channels == 1)
		hipLaunchKernelGGL(k_ocean_mipmap<1>, grid, dim3(GROUP), 0, s, a);
	else if (channels == 2)
		hipLaunchKernelGGL(k_ocean_mipmap<2>, grid, dim3(GROUP), 0, s, a);
	else
		hipLaunchKernelGGL(k_ocean_mipmap<4>, grid, dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_ocean_update_lod(gr_ctx *ctx, gr_stream stream, const gr_image *lod_image, const gr_push_ocean_update_lod *push)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, push);
	if (const char *rule = grid_rule(push->num_threads[0], push->num_threads[1], push->max_lod))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_update_lod: %s (%d x %d, max_lod %g)", rule, push->num_threads[0], push->num_threads[1], double(push->max_lod));
	const uint32_t n = uint32_t(push->num_threads[0]);
	GR_CHECK_IMAGE(ctx, lod_image, GR_FORMAT_R16_SFLOAT, n, n);

	UpdateLodLaunch a = {};
	memcpy(a.u.camera, push->shifted_camera_pos, sizeof(a.u.camera));
	a.u.max_lod = push->max_lod;
	a.u.offset_x = push->image_offset[0];
	a.u.offset_y = push->image_offset[1];
	a.u.n = int(n);
	a.u.base_x = push->grid_base[0];
	a.u.base_y = push->grid_base[1];
	a.u.size_x = push->grid_size[0];
	a.u.size_y = push->grid_size[1];
	a.u.lod_bias = push->lod_bias;
	a.out = static_cast<uint8_t *>(lod_image->ptr);
	a.pitch = lod_image->pitch_bytes;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_update_lod"};
	hipLaunchKernelGGL(k_ocean_update_lod, dim3(gr_div_up(n, TILE), gr_div_up(n, TILE)), dim3(TILE * TILE), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_ocean_init_counter_buffer(gr_ctx *ctx, gr_stream stream, const gr_ocean_buffer *counters, const uint32_t *counts16)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, counters && counters->ptr);
	GR_CHECK_ARG(ctx, counts16);
	if (counters->size_bytes < MAX_LOD_INDIRECT * sizeof(gr_ocean_indirect_draw) || (reinterpret_cast<uintptr_t>(counters->ptr) & 3u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_init_counter_buffer: counters has %llu bytes, below 8 * 32, or is not 4-byte aligned",
		                 static_cast<unsigned long long>(counters->size_bytes));
	InitCountersLaunch a = {};
	a.draws = static_cast<uint32_t *>(counters->ptr);
	memcpy(a.counts, counts16, sizeof(a.counts)); // NUM_COUNTERS = 8: the shader reads the first eight of the sixteen
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_init_counter_buffer"};
	hipLaunchKernelGGL(k_ocean_init_counters, dim3(1), dim3(64), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_ocean_cull_blocks(gr_ctx *ctx, gr_stream stream, const gr_image *lod_image, uint32_t wrap, const gr_ocean_buffer *patches,
                                    const gr_ocean_buffer *counters, const gr_push_ocean_cull *push, const float *frustum)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, push);
	GR_CHECK_ARG(ctx, frustum);
	GR_CHECK_ARG(ctx, patches && patches->ptr);
	GR_CHECK_ARG(ctx, counters && counters->ptr);
	if (push->num_threads[0] > 128u || push->num_threads[1] > 128u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_cull_blocks: num_threads is not a power of two in 4 .. 128 (%u x %u)", push->num_threads[0], push->num_threads[1]);
	if (const char *rule = grid_rule(int32_t(push->num_threads[0]), int32_t(push->num_threads[1]), push->max_lod))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_cull_blocks: %s (%u x %u, max_lod %g)", rule, push->num_threads[0], push->num_threads[1], double(push->max_lod));
	const uint32_t n = push->num_threads[0], num_lods = uint32_t(push->max_lod) + 1u;
	GR_CHECK_IMAGE(ctx, lod_image, GR_FORMAT_R16_SFLOAT, n, n);
	if (push->lod_stride < n * n)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_cull_blocks: lod_stride %u is below num_threads.x * num_threads.y = %u", push->lod_stride, n * n);
	if (patches->size_bytes < uint64_t(push->lod_stride) * num_lods * sizeof(gr_ocean_patch) || (reinterpret_cast<uintptr_t>(patches->ptr) & 15u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_cull_blocks: patches has %llu bytes, below lod_stride * (max_lod + 1) * 32 = %llu, or is not 16-byte aligned",
		                 static_cast<unsigned long long>(patches->size_bytes), static_cast<unsigned long long>(uint64_t(push->lod_stride) * num_lods * sizeof(gr_ocean_patch)));
	if (counters->size_bytes < MAX_LOD_INDIRECT * sizeof(gr_ocean_indirect_draw) || (reinterpret_cast<uintptr_t>(counters->ptr) & 3u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_cull_blocks: counters has %llu bytes, below 8 * 32, or is not 4-byte aligned",
		                 static_cast<unsigned long long>(counters->size_bytes));
	const size_t image_bytes = size_t(lod_image->pitch_bytes) * lod_image->height;
	if (gr_images_overlap(patches->ptr, size_t(patches->size_bytes), lod_image->ptr, image_bytes) ||
	    gr_images_overlap(counters->ptr, size_t(counters->size_bytes), lod_image->ptr, image_bytes) ||
	    gr_images_overlap(patches->ptr, size_t(patches->size_bytes), counters->ptr, size_t(counters->size_bytes)))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_cull_blocks: patches, counters and the LOD image overlap");

	CullLaunch a = {};
	memcpy(a.c.world_offset, push->world_offset, sizeof(a.c.world_offset));
	a.c.offset_x = push->image_offset[0];
	a.c.offset_y = push->image_offset[1];
	a.c.n = int(n);
	a.c.base_x = push->grid_base[0];
	a.c.base_y = push->grid_base[1];
	a.c.size_x = push->grid_size[0];
	a.c.size_y = push->grid_size[1];
	a.c.resolution_x = push->grid_resolution[0];
	a.c.resolution_y = push->grid_resolution[1];
	a.c.range_lo = push->heightmap_range[0];
	a.c.range_hi = push->heightmap_range[1];
	a.c.guard_band = push->guard_band;
	a.c.lod_stride = push->lod_stride;
	a.c.max_lod = push->max_lod;
	a.c.handle_edge_lods = push->handle_edge_lods != 0 ? 1u : 0u;
	a.c.wrap = wrap != 0u ? 1u : 0u;
	memcpy(a.c.frustum, frustum, sizeof(a.c.frustum));
	a.c.lods = texture_of(lod_image);
	a.patches = static_cast<Patch *>(patches->ptr);
	a.draws = static_cast<uint32_t *>(counters->ptr);
	a.num_lods = num_lods;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_cull_blocks"};
	hipLaunchKernelGGL(k_ocean_cull, dim3(gr_div_up(n, TILE), gr_div_up(n, TILE)), dim3(TILE * TILE), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
