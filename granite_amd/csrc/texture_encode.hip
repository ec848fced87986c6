// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// gr_texture_encode: R8 / RG8 / RGBA8 texels to BC4 / BC5 blocks, what scene-export/texture_compression.cpp's
// enqueue_compression_block_rgtc does with scene-export/rgtc_compressor.cpp, one launch per level and layer.
// gr_texture_generate_mipmap: one level of scene-export/texture_utils.cpp's generate_mipmaps for the UNORM8 formats.
// The rules are texture_encode_core.hpp's; this file is how they are spread over lanes.
//
// k_texture_encode_rgtc: GROUP lanes share one channel block (the 16 values of one component of a 4 x 4 block; a BC5 block is two of
// them side by side).  The reference's code has four ways through a channel block -- flat, range below 16, searched with the 7-weight form
// kept, searched and replaced -- and the searched ones cost some twenty times the others, so a lane that owned a whole block would wait for
// the slowest block among 64.  With a group per channel block every lane of the group takes the same way, and the work inside one way is
// spread:
//   - lanes 0 .. 15 own one texel each: fetch, 7-weight position and error, rank among the sorted values, 5-weight code.  The 48 code bits
//     and the error are combined with xor shuffles over 16 lanes;
//   - the sorted values go through LDS (a lane stores its value at its rank), and so do the 15 below_sum(lo) and 15 above_sum(hi), which
//     depend on one position each: lane l computes both for position l;
//   - the 120 candidates are dealt out GROUP apart, in partition_by_width's order and not the reference's: inside_sum loops over the
//     positions between lo and hi, a wave's loop runs as long as its longest lane's, and widest-first puts partitions of nearly one
//     width into the same turn -- 35 loop turns for the eight candidate turns instead of 120 (the order and each partition's search
//     position are a table in LDS, one entry a thread at the start of a workgroup).  A lane adds the two sums from LDS and keeps the
//     smallest search_key; an xor shuffle minimum over the group gives every lane the winner, which is the reference's first strict
//     minimum because the key orders equal errors by the reference's search position (candidate_index) and the 7-weight form holds
//     position 0;
//   - divider5 and divider7 are tables in LDS too: two integer divisions a thread instead of ten a lane and block;
//   - lane 0 stores the 8 bytes with one store (block pointers and pitches are multiples of the block size).
// Groups past the row's last channel block run on the last one's texels and store nothing: no lane leaves before the barriers.
// GROUP is 16: four channel blocks a wave, so a wave still waits for the slowest of four, against eight candidate turns of which half a
// turn is idle.  GR_RGTC_GROUP=32 or 64 at build time gives the other mappings for an A/B (DESIGN.md 7.16 has the times).
#include "ctx.hpp"
#include "texture_encode_core.hpp"

#ifndef GR_RGTC_GROUP
#define GR_RGTC_GROUP 16
#endif

namespace
{
namespace te = gr_texenc;

struct EncodeArgs
{
	const uint8_t *in;
	uint8_t *blocks;
	uint32_t in_pitch, block_pitch;
	uint32_t width, height, blocks_x;
	uint32_t stride, channels; // bytes a pixel; channel blocks a block (1 BC4, 2 BC5)
};

constexpr int ENCODE_THREADS = 256;

template <int GROUP>
__device__ __forceinline__ uint32_t group_or(uint32_t v)
{
#pragma unroll
	for (int m = 8; m >= 1; m >>= 1) // the texel lanes: 16 wide whatever GROUP is
		v |= uint32_t(__shfl_xor(int(v), m, 16));
	return v;
}

template <int GROUP>
__global__ __launch_bounds__(ENCODE_THREADS) void k_texture_encode_rgtc(EncodeArgs a)
{
	constexpr int GROUPS = ENCODE_THREADS / GROUP;
	__shared__ __attribute__((aligned(16))) uint8_t s_texels[GROUPS][16];
	__shared__ __attribute__((aligned(16))) uint8_t s_sorted[GROUPS][16];
	__shared__ int s_below[GROUPS][16], s_above[GROUPS][16];
	__shared__ int s_divider5[256], s_divider7[256]; // by range
	__shared__ uint16_t s_partition[128];            // by place in partition_by_width's order: lo, hi << 4, (candidate_index + 1) << 8
	static_assert(ENCODE_THREADS == 256, "one table entry a thread");
	s_divider5[threadIdx.x] = te::divider5(int(threadIdx.x));
	s_divider7[threadIdx.x] = threadIdx.x ? te::divider7(int(threadIdx.x)) : 0;
	if (threadIdx.x < te::CANDIDATES)
	{
		int p, q;
		te::partition_by_width(int(threadIdx.x), p, q);
		s_partition[threadIdx.x] = uint16_t(p | (q << 4) | ((te::candidate_index(p, q) + 1) << 8));
	}

	const int lane = int(threadIdx.x) % GROUP, group = int(threadIdx.x) / GROUP;
	const uint32_t channel_blocks = a.blocks_x * a.channels; // of this row of blocks
	const uint32_t wanted = blockIdx.x * uint32_t(GROUPS) + uint32_t(group);
	const bool stores = wanted < channel_blocks;
	const uint32_t index = stores ? wanted : channel_blocks - 1u;
	const uint32_t bx = index / a.channels, channel = index % a.channels, by = blockIdx.y;

	int value = 0;
	if (lane < 16)
	{
		value = a.in[te::block_texel_offset(bx, by, lane, a.width, a.height, a.in_pitch, a.stride) + channel];
		s_texels[group][lane] = uint8_t(value);
	}
	__syncthreads();

	const uint8_t *texels = s_texels[group];
	int lo = 255, hi = 0;
#pragma unroll
	for (int i = 0; i < 16; i++)
	{
		lo = min(lo, int(texels[i]));
		hi = max(hi, int(texels[i]));
	}
	const int range = hi - lo; // the same in every lane of the group, and so is every branch below
	int e0 = hi, e1 = lo;
	uint64_t bits = 0;
	const bool searched = range >= te::RANGE_THRESHOLD;

	int error = 0;
	if (range != 0 && lane < 16)
	{
		const int position = te::quantise(value, lo, s_divider7[range]);
		error = te::error7(value, lo, range, position);
		bits = uint64_t(te::remap7(position)) << (3 * lane);
	}
	if (searched && lane < 16)
		s_sorted[group][te::rank_of(texels, lane)] = uint8_t(value);
	__syncthreads();

	const uint8_t *sorted = s_sorted[group];
	if (searched && lane < 16)
	{
		s_below[group][lane] = lane < 15 ? te::below_sum(sorted, lane) : 0;
		s_above[group][lane] = lane < 15 ? te::above_sum(sorted, lane) : 0;
	}
	__syncthreads();

	if (searched)
	{
#pragma unroll
		for (int m = 8; m >= 1; m >>= 1)
			error += __shfl_xor(error, m, 16);
		uint32_t best = te::search_key(error, 0); // lanes 0 .. 15 hold the whole block's error, the others 0: they enter no incumbent
		if (lane >= 16)
			best = 0xffffffffu;
		for (int k = lane; k < te::CANDIDATES; k += GROUP)
		{
			const int entry = s_partition[k], p = entry & 15, q = (entry >> 4) & 15;
			const int error_k = s_below[group][p] + te::inside_sum(sorted, p, q, s_divider5[sorted[q] - sorted[p]]) + s_above[group][q];
			best = min(best, te::search_key(error_k, entry >> 8));
		}
#pragma unroll
		for (int m = GROUP / 2; m >= 1; m >>= 1)
			best = min(best, uint32_t(__shfl_xor(int(best), m, GROUP)));
		const int slot = te::key_slot(best);
		if (slot)
		{
			int p, q;
			te::candidate_partition(slot - 1, p, q);
			e0 = sorted[p];
			e1 = sorted[q];
			bits = lane < 16 ? uint64_t(te::code5(value, e0, e1, s_divider5[e1 - e0])) << (3 * lane) : 0;
		}
	}

	const uint32_t low = group_or<GROUP>(uint32_t(bits)), high = group_or<GROUP>(uint32_t(bits >> 32));
	if (lane == 0 && stores)
	{
		uint8_t *dst = a.blocks + size_t(by) * a.block_pitch + size_t(index) * 8u;
		*reinterpret_cast<uint2 *>(dst) = make_uint2(uint32_t(e0) | (uint32_t(e1) << 8) | (low << 16), (low >> 16) | (high << 16));
	}
}

struct MipArgs
{
	const uint8_t *src;
	uint8_t *dst;
	uint32_t src_pitch, dst_pitch;
	uint32_t src_width, src_height, dst_width, dst_height;
	float rescale_x, rescale_y;
};

// One destination texel a lane, lanes along x.
template <int CHANNELS>
__global__ __launch_bounds__(256) void k_texture_mip_level(MipArgs a)
{
	const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
	if (x >= a.dst_width || y >= a.dst_height)
		return;
	uint32_t x0, x1, y0, y1;
	float wx, wy;
	te::mip_axis(x, a.rescale_x, a.src_width, x0, x1, wx);
	te::mip_axis(y, a.rescale_y, a.src_height, y0, y1, wy);
	const uint8_t *top = a.src + size_t(y0) * a.src_pitch, *bottom = a.src + size_t(y1) * a.src_pitch;
	uint8_t *dst = a.dst + size_t(y) * a.dst_pitch + size_t(x) * CHANNELS;
#pragma unroll
	for (int c = 0; c < CHANNELS; c++)
		dst[c] = uint8_t(te::mip_filter(top[x0 * CHANNELS + c], top[x1 * CHANNELS + c], bottom[x0 * CHANNELS + c], bottom[x1 * CHANNELS + c], wx, wy));
}

bool is_encode_input(uint32_t f)
{
	return f == GR_FORMAT_R8_UNORM || f == GR_FORMAT_R8G8_UNORM || f == GR_FORMAT_R8G8B8A8_UNORM || f == GR_FORMAT_R8G8B8A8_SRGB;
}
} // namespace

extern "C" int gr_texture_encode_supported(uint32_t block_format, uint32_t input_format)
{
	if (block_format == GR_FORMAT_BC4_UNORM_BLOCK)
		return is_encode_input(input_format) ? 1 : 0;
	if (block_format == GR_FORMAT_BC5_UNORM_BLOCK)
		return is_encode_input(input_format) && input_format != GR_FORMAT_R8_UNORM ? 1 : 0;
	return 0;
}

extern "C" int gr_texture_encode(gr_ctx *ctx, gr_stream stream, uint32_t block_format, const gr_image *in, void *blocks, uint32_t block_row_pitch_bytes)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, in);
	if (block_format != GR_FORMAT_BC4_UNORM_BLOCK && block_format != GR_FORMAT_BC5_UNORM_BLOCK)
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_encode: format %u is not a block format encoded here (BC4_UNORM, BC5_UNORM)", block_format);
	if (!is_encode_input(in->format))
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_encode: input format %u is not R8_UNORM, R8G8_UNORM, R8G8B8A8_UNORM or R8G8B8A8_SRGB", in->format);
	if (!gr_texture_encode_supported(block_format, in->format))
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_encode: input format %u has one component, block format %u takes two", in->format, block_format);
	if (in->width > 65536u || in->height > 65536u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_encode: input extent %u x %u is larger than 65536", in->width, in->height);
	if (in->width == 0 || in->height == 0)
		return GR_OK;
	EncodeArgs a = {};
	a.channels = block_format == GR_FORMAT_BC5_UNORM_BLOCK ? 2u : 1u;
	const uint32_t block_bytes = 8u * a.channels;
	a.blocks_x = gr_div_up(in->width, 4);
	const uint32_t blocks_y = gr_div_up(in->height, 4);
	if (const char *rule = gr_image_layout_rule(in, in->format)) // the kernel loads bytes: any pitch that covers a row, any alignment
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_encode: invalid argument: in%s", rule);
	GR_CHECK_ARG(ctx, in->ptr);
	GR_CHECK_ARG(ctx, blocks);
	if ((reinterpret_cast<uintptr_t>(blocks) | block_row_pitch_bytes) & (block_bytes - 1u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_encode: invalid argument: blocks or block_row_pitch_bytes (%u) is not a multiple of the block size %u",
		                 block_row_pitch_bytes, block_bytes);
	if (block_row_pitch_bytes < a.blocks_x * block_bytes)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_encode: block row pitch %u is smaller than a row of %u blocks", block_row_pitch_bytes, a.blocks_x);
	a.in = static_cast<const uint8_t *>(in->ptr);
	a.blocks = static_cast<uint8_t *>(blocks);
	a.in_pitch = in->pitch_bytes;
	a.block_pitch = block_row_pitch_bytes;
	a.width = in->width;
	a.height = in->height;
	a.stride = gr_format_texel_bytes(in->format);

	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "texture_encode"};
	constexpr int GROUPS = ENCODE_THREADS / GR_RGTC_GROUP;
	const dim3 grid(gr_div_up(a.blocks_x * a.channels, GROUPS), blocks_y), block(ENCODE_THREADS);
	hipLaunchKernelGGL((k_texture_encode_rgtc<GR_RGTC_GROUP>), grid, block, 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_texture_generate_mipmap(gr_ctx *ctx, gr_stream stream, const gr_image *src_level, const gr_image *dst_level)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, src_level);
	GR_CHECK_ARG(ctx, dst_level);
	const uint32_t format = src_level->format;
	if (format == GR_FORMAT_R8G8B8A8_SRGB)
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_generate_mipmap: src_level is R8G8B8A8_SRGB: sRGB-aware filtering is not built");
	if (format != GR_FORMAT_R8_UNORM && format != GR_FORMAT_R8G8_UNORM && format != GR_FORMAT_R8G8B8A8_UNORM)
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_generate_mipmap: src_level format %u is not R8_UNORM, R8G8_UNORM or R8G8B8A8_UNORM", format);
	if (dst_level->format != format)
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_generate_mipmap: dst_level format %u is not src_level's format %u", dst_level->format, format);
	if (src_level->width > 65536u || src_level->height > 65536u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_generate_mipmap: src_level extent %u x %u is larger than 65536", src_level->width, src_level->height);
	if (const char *rule = gr_image_layout_rule(src_level, format)) // the kernel loads and stores bytes: any alignment, as in gr_texture_encode
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_generate_mipmap: invalid argument: src_level%s", rule);
	const uint32_t width = src_level->width >> 1 ? src_level->width >> 1 : 1u, height = src_level->height >> 1 ? src_level->height >> 1 : 1u;
	if (dst_level->width != width || dst_level->height != height)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_generate_mipmap: invalid argument: dst_level is %u x %u, the level below %u x %u is %u x %u",
		                 dst_level->width, dst_level->height, src_level->width, src_level->height, width, height);
	if (const char *rule = gr_image_layout_rule(dst_level, format))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_generate_mipmap: invalid argument: dst_level%s", rule);
	GR_CHECK_ARG(ctx, src_level->ptr);
	GR_CHECK_ARG(ctx, dst_level->ptr);
	if (gr_images_overlap(src_level, dst_level))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_generate_mipmap: invalid argument: dst_level shares bytes with src_level");
	MipArgs a = {};
	a.src = static_cast<const uint8_t *>(src_level->ptr);
	a.dst = static_cast<uint8_t *>(dst_level->ptr);
	a.src_pitch = src_level->pitch_bytes;
	a.dst_pitch = dst_level->pitch_bytes;
	a.src_width = src_level->width;
	a.src_height = src_level->height;
	a.dst_width = width;
	a.dst_height = height;
	a.rescale_x = te::mip_rescale(a.src_width, width);
	a.rescale_y = te::mip_rescale(a.src_height, height);

	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "texture_mip_level"};
	const dim3 grid(gr_div_up(width, 64), gr_div_up(height, 4)), block(64, 4);
	switch (gr_format_texel_bytes(format))
	{
	case 1: hipLaunchKernelGGL((k_texture_mip_level<1>), grid, block, 0, s, a); break;
	case 2: hipLaunchKernelGGL((k_texture_mip_level<2>), grid, block, 0, s, a); break;
	default: hipLaunchKernelGGL((k_texture_mip_level<4>), grid, block, 0, s, a); break;
	}
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
