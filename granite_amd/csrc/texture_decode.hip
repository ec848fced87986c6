// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// gr_texture_decode: BC1-BC7 and ASTC LDR blocks to texels, what vulkan/texture/texture_decoder.cpp's decode_compressed_image does with
// assets/shaders/decode/{s3tc,rgtc,bc7,bc6,astc}.comp, one launch per level and layer.
//
// BC1-BC7: the shaders spend one invocation per texel and parse the block header sixteen times.  Here a lane owns a block (or, LANES > 1, a
// share of its rows): one 8- or 16-byte payload load, the header parsed once (bc_decode.hpp), one store per row -- 16 B for RGBA8,
// 4 B for R8, 8 B for RG8, 32 B for RGBA16F.  Lanes run along x, so the 64 stores of a wave's row are 1 KiB of one image row.
// The shaders' specialization constants (USE_ALPHA, BC_VERSION, DUAL_COMPONENT, SIGNED) are the KIND template parameter.
// Pointers or pitches that are not aligned to the load / store width take a byte-by-byte path, as do the partial blocks at the right
// edge; rows below the image are not written.
//
// ASTC LDR (assets/shaders/decode/astc.comp, DECODE_8BIT) does not fit that layout: a footprint is up to 12 x 12 texels and a block's
// header -- block mode, partitions, up to 18 endpoint integers, up to 64 weights -- is most of the work.  k_astc_decode gives a wave 64
// neighbouring blocks of one block row: every lane parses one block into an LDS record (astc_decode.hpp's block half), then the wave
// walks the 64 * BW x BH texels of those blocks row by row, 64 neighbouring texels of one image row per turn (the texel half), one
// 4-byte store per lane -- 256 B of a row per turn, across block boundaries.  BW * BH turns whatever the image, so the count is
// wave-uniform.  Measured at 4096 x 4096 on the legal blocks of the test suite's case sets (profiles/texture_decode_time.txt): 4 x 4 295 us,
// 6 x 6 256 us, 8 x 8 183 us, 12 x 12 200 us beside BC7's 83 us; void extents only 18 - 28 us.  The other form, every lane parsing the
// header again for its own texel as the shader does, was not built, so there is no A/B to report.
#include "ctx.hpp"
#include "bc_decode.hpp"
#include "astc_decode.hpp"

namespace
{
struct DecodeArgs
{
	const uint8_t *blocks;
	uint8_t *out;
	uint32_t block_pitch, out_pitch;
	uint32_t width, height, blocks_x, blocks_y;
	uint32_t blocks_aligned, out_aligned;
};

constexpr int WAVE_BLOCKS_Y = 4; // a 64 x 4 workgroup: four waves, each one row of blocks

template <int KIND, int LANES>
__global__ __launch_bounds__(64 * WAVE_BLOCKS_Y) void k_texture_decode(DecodeArgs a)
{
	constexpr int ROWS = 4 / LANES;
	constexpr int BLOCK_BYTES = gr_bc::block_bytes(KIND);
	constexpr int ROW_BYTES = 4 * gr_bc::texel_bytes(KIND);
	const uint32_t lane_x = blockIdx.x * 64u + threadIdx.x;
	const uint32_t bx = lane_x / LANES, by = blockIdx.y * WAVE_BLOCKS_Y + threadIdx.y;
	if (bx >= a.blocks_x || by >= a.blocks_y)
		return;
	const int row0 = int(lane_x % LANES) * ROWS;

	const uint8_t *src = a.blocks + size_t(by) * a.block_pitch + size_t(bx) * BLOCK_BYTES;
	gr_bc::Payload p = {0, 0};
	if (a.blocks_aligned)
	{
		if (BLOCK_BYTES == 16)
		{
			const uint4 v = *reinterpret_cast<const uint4 *>(src);
			p.lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
			p.hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
		}
		else
		{
			const uint2 v = *reinterpret_cast<const uint2 *>(src);
			p.lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
		}
	}
	else
	{
		for (int i = 0; i < 8; i++)
			p.lo |= uint64_t(src[i]) << (8 * i);
		if (BLOCK_BYTES == 16)
			for (int i = 0; i < 8; i++)
				p.hi |= uint64_t(src[8 + i]) << (8 * i);
	}

	uint32_t words[ROWS][gr_bc::ROW_WORDS_MAX];
	gr_bc::decode_rows<KIND, ROWS>(p, row0, words);

	const uint32_t x0 = 4u * bx;
	const uint32_t texels = a.width - x0 < 4u ? a.width - x0 : 4u;
#pragma unroll
	for (int r = 0; r < ROWS; r++)
	{
		const uint32_t y = 4u * by + uint32_t(row0 + r);
		if (y >= a.height)
			break;
		uint8_t *dst = a.out + size_t(y) * a.out_pitch + size_t(bx) * ROW_BYTES;
		if (a.out_aligned && texels == 4u)
		{
			if (ROW_BYTES == 4)
				*reinterpret_cast<uint32_t *>(dst) = words[r][0];
			else if (ROW_BYTES == 8)
				*reinterpret_cast<uint2 *>(dst) = make_uint2(words[r][0], words[r][1]);
			else
			{
				*reinterpret_cast<uint4 *>(dst) = make_uint4(words[r][0], words[r][1], words[r][2], words[r][3]);
				if (ROW_BYTES == 32)
					*reinterpret_cast<uint4 *>(dst + 16) = make_uint4(words[r][4], words[r][5], words[r][6], words[r][7]);
			}
		}
		else
		{
			const uint32_t bytes = texels * uint32_t(gr_bc::texel_bytes(KIND));
#pragma unroll
			for (int i = 0; i < ROW_BYTES; i++)
				if (uint32_t(i) < bytes)
					dst[i] = uint8_t(words[r][i / 4] >> (8 * (i % 4)));
		}
	}
}

template <int BW, int BH>
__global__ __launch_bounds__(64) void k_astc_decode(DecodeArgs a)
{
	__shared__ gr_astc::Block records[64];
	const uint32_t bx0 = blockIdx.x * 64u, by = blockIdx.y; // the launch has no block past blocks_x / 64 or blocks_y
	const uint32_t bx = bx0 + threadIdx.x;
	if (bx < a.blocks_x)
	{
		const uint8_t *src = a.blocks + size_t(by) * a.block_pitch + size_t(bx) * 16u;
		gr_astc::Payload p = {0, 0};
		if (a.blocks_aligned)
		{
			const uint4 v = *reinterpret_cast<const uint4 *>(src);
			p.lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
			p.hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
		}
		else
		{
			for (int i = 0; i < 8; i++)
			{
				p.lo |= uint64_t(src[i]) << (8 * i);
				p.hi |= uint64_t(src[8 + i]) << (8 * i);
			}
		}
		gr_astc::decode_block(p, BW, BH, records[threadIdx.x]);
	}
	__syncthreads();

	for (uint32_t turn = 0; turn < uint32_t(BW * BH); turn++)
	{
		const uint32_t ly = turn / BW, lx = (turn % BW) * 64u + threadIdx.x; // inside the 64 * BW x BH texels of this wave
		const uint32_t x = bx0 * BW + lx, y = by * BH + ly;
		if (x >= a.width || y >= a.height)
			continue;
		const uint32_t texel = gr_astc::decode_texel(records[lx / BW], int(lx % BW), int(ly), BW, BH);
		uint8_t *dst = a.out + size_t(y) * a.out_pitch + size_t(x) * 4u;
		if (a.out_aligned)
			*reinterpret_cast<uint32_t *>(dst) = texel;
		else
			for (int i = 0; i < 4; i++)
				dst[i] = uint8_t(texel >> (8 * i));
	}
}

// 0..13 for the ASTC LDR formats (UNORM and SRGB of one footprint share an index), -1 otherwise.
int astc_footprint_of(uint32_t block_format)
{
	return block_format >= GR_FORMAT_ASTC_4x4_UNORM_BLOCK && block_format <= GR_FORMAT_ASTC_12x12_SRGB_BLOCK ? int(block_format - GR_FORMAT_ASTC_4x4_UNORM_BLOCK) / 2 : -1;
}

int kind_of(uint32_t block_format)
{
	switch (block_format)
	{
	case GR_FORMAT_BC1_RGB_UNORM_BLOCK:
	case GR_FORMAT_BC1_RGB_SRGB_BLOCK: return gr_bc::KIND_BC1_RGB;
	case GR_FORMAT_BC1_RGBA_UNORM_BLOCK:
	case GR_FORMAT_BC1_RGBA_SRGB_BLOCK: return gr_bc::KIND_BC1_RGBA;
	case GR_FORMAT_BC2_UNORM_BLOCK:
	case GR_FORMAT_BC2_SRGB_BLOCK: return gr_bc::KIND_BC2;
	case GR_FORMAT_BC3_UNORM_BLOCK:
	case GR_FORMAT_BC3_SRGB_BLOCK: return gr_bc::KIND_BC3;
	case GR_FORMAT_BC4_UNORM_BLOCK: return gr_bc::KIND_BC4;
	case GR_FORMAT_BC5_UNORM_BLOCK: return gr_bc::KIND_BC5;
	case GR_FORMAT_BC6H_UFLOAT_BLOCK: return gr_bc::KIND_BC6H_UFLOAT;
	case GR_FORMAT_BC6H_SFLOAT_BLOCK: return gr_bc::KIND_BC6H_SFLOAT;
	case GR_FORMAT_BC7_UNORM_BLOCK:
	case GR_FORMAT_BC7_SRGB_BLOCK: return gr_bc::KIND_BC7;
	default: return -1;
	}
}

bool is_srgb_block(uint32_t f)
{
	return f == GR_FORMAT_BC1_RGB_SRGB_BLOCK || f == GR_FORMAT_BC1_RGBA_SRGB_BLOCK || f == GR_FORMAT_BC2_SRGB_BLOCK || f == GR_FORMAT_BC3_SRGB_BLOCK ||
	       f == GR_FORMAT_BC7_SRGB_BLOCK;
}

// What gr_texture_decode wants as the output's format: the BC answer of gr_texture_decoded_format, RGBA8 UNORM / SRGB for ASTC LDR.
uint32_t decoded_format_of(uint32_t block_format)
{
	if (astc_footprint_of(block_format) >= 0)
		return (block_format - GR_FORMAT_ASTC_4x4_UNORM_BLOCK) & 1u ? GR_FORMAT_R8G8B8A8_SRGB : GR_FORMAT_R8G8B8A8_UNORM;
	return gr_texture_decoded_format(block_format);
}
} // namespace

extern "C" uint32_t gr_texture_decoded_format(uint32_t block_format)
{
	switch (kind_of(block_format))
	{
	case -1: return GR_FORMAT_UNDEFINED;
	case gr_bc::KIND_BC4: return GR_FORMAT_R8_UNORM;
	case gr_bc::KIND_BC5: return GR_FORMAT_R8G8_UNORM;
	case gr_bc::KIND_BC6H_UFLOAT:
	case gr_bc::KIND_BC6H_SFLOAT: return GR_FORMAT_R16G16B16A16_SFLOAT;
	default: return is_srgb_block(block_format) ? GR_FORMAT_R8G8B8A8_SRGB : GR_FORMAT_R8G8B8A8_UNORM;
	}
}

extern "C" uint32_t gr_texture_block_bytes(uint32_t block_format)
{
	const int kind = kind_of(block_format);
	return kind < 0 ? 0u : uint32_t(gr_bc::block_bytes(kind));
}

extern "C" int gr_texture_block_dim(uint32_t block_format, uint32_t *width, uint32_t *height)
{
	const int astc = astc_footprint_of(block_format);
	if ((astc < 0 && kind_of(block_format) < 0) || !width || !height)
		return !width || !height ? GR_ERR_INVALID_ARGUMENT : GR_ERR_UNSUPPORTED_FORMAT;
	*width = astc < 0 ? 4u : gr_astc::footprint(astc).w;
	*height = astc < 0 ? 4u : gr_astc::footprint(astc).h;
	return GR_OK;
}

extern "C" int gr_texture_block_info(uint32_t block_format, uint32_t *block_bytes, uint32_t *decoded_format)
{
	if (!block_bytes || !decoded_format)
		return GR_ERR_INVALID_ARGUMENT;
	*block_bytes = astc_footprint_of(block_format) >= 0 ? 16u : gr_texture_block_bytes(block_format);
	*decoded_format = decoded_format_of(block_format);
	return *block_bytes ? GR_OK : GR_ERR_UNSUPPORTED_FORMAT;
}

extern "C" int gr_texture_decode(gr_ctx *ctx, gr_stream stream, uint32_t block_format, const void *blocks, uint32_t block_row_pitch_bytes,
                                 const gr_image *out)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, out);
	const int kind = kind_of(block_format), astc = astc_footprint_of(block_format);
	if (kind < 0 && astc < 0)
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_decode: format %u is not a block format handled here (BC1-BC7 without SNORM, ASTC LDR)", block_format);
	if (out->format != decoded_format_of(block_format))
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_decode: output format %u is not the decoded format %u of block format %u", out->format,
		                 decoded_format_of(block_format), block_format);
	if (out->width > 65536u || out->height > 65536u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_decode: output extent %u x %u is larger than 65536", out->width, out->height);
	if (out->width == 0 || out->height == 0)
		return GR_OK;
	DecodeArgs a = {};
	a.width = out->width;
	a.height = out->height;
	const uint32_t block_w = astc < 0 ? 4u : gr_astc::footprint(astc).w, block_h = astc < 0 ? 4u : gr_astc::footprint(astc).h;
	a.blocks_x = gr_div_up(out->width, block_w);
	a.blocks_y = gr_div_up(out->height, block_h);
	const uint32_t block_bytes = astc < 0 ? uint32_t(gr_bc::block_bytes(kind)) : 16u, texel_bytes = astc < 0 ? uint32_t(gr_bc::texel_bytes(kind)) : 4u;
	if (block_row_pitch_bytes < a.blocks_x * block_bytes)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_decode: block row pitch %u is smaller than a row of %u blocks", block_row_pitch_bytes, a.blocks_x);
	if (const char *rule = gr_image_layout_rule(out, out->format)) // the kernel stores bytes where the output is not aligned (out_aligned, below)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_texture_decode: invalid argument: output%s", rule);
	GR_CHECK_ARG(ctx, blocks);
	GR_CHECK_ARG(ctx, out->ptr);
	a.blocks = static_cast<const uint8_t *>(blocks);
	a.out = static_cast<uint8_t *>(out->ptr);
	a.block_pitch = block_row_pitch_bytes;
	a.out_pitch = out->pitch_bytes;
	a.blocks_aligned = ((reinterpret_cast<uintptr_t>(blocks) | block_row_pitch_bytes) & (block_bytes - 1u)) == 0;
	const uint32_t row_bytes = astc < 0 ? 4u * texel_bytes : 4u; // the widest store: a BC block's row, one ASTC texel
	a.out_aligned = is_aligned(out, row_bytes < 16u ? row_bytes : 16u);

	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "texture_decode"};
	if (astc >= 0)
	{
		const dim3 grid(gr_div_up(a.blocks_x, 64), a.blocks_y), block(64);
#define ASTC_DECODE_CASE(index_, w_, h_) \
	case index_: hipLaunchKernelGGL((k_astc_decode<w_, h_>), grid, block, 0, s, a); break;
		switch (astc)
		{
			ASTC_DECODE_CASE(0, 4, 4)
			ASTC_DECODE_CASE(1, 5, 4)
			ASTC_DECODE_CASE(2, 5, 5)
			ASTC_DECODE_CASE(3, 6, 5)
			ASTC_DECODE_CASE(4, 6, 6)
			ASTC_DECODE_CASE(5, 8, 5)
			ASTC_DECODE_CASE(6, 8, 6)
			ASTC_DECODE_CASE(7, 8, 8)
			ASTC_DECODE_CASE(8, 10, 5)
			ASTC_DECODE_CASE(9, 10, 6)
			ASTC_DECODE_CASE(10, 10, 8)
			ASTC_DECODE_CASE(11, 10, 10)
			ASTC_DECODE_CASE(12, 12, 10)
			ASTC_DECODE_CASE(13, 12, 12)
		}
#undef ASTC_DECODE_CASE
		GR_CHECK_LAUNCH(ctx);
		return GR_OK;
	}
	// Measured at 4096 x 4096 (profiles/texture_decode_time.txt): BC6H is faster with four lanes per block (one row each, 32 B stored per
	// lane, every lane parsing the header itself), BC7 with one.  The slower forms are not built.
	const int lanes = kind == gr_bc::KIND_BC6H_UFLOAT || kind == gr_bc::KIND_BC6H_SFLOAT ? 4 : 1;
	const dim3 grid(gr_div_up(a.blocks_x * uint32_t(lanes), 64), gr_div_up(a.blocks_y, WAVE_BLOCKS_Y)), block(64, WAVE_BLOCKS_Y);
#define TEXTURE_DECODE_CASE(kind_, lanes_) \
	case (kind_) * 8 + (lanes_): hipLaunchKernelGGL((k_texture_decode<kind_, lanes_>), grid, block, 0, s, a); break;
	switch (kind * 8 + lanes)
	{
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC1_RGB, 1)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC1_RGBA, 1)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC2, 1)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC3, 1)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC4, 1)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC5, 1)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC7, 1)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC6H_UFLOAT, 4)
		TEXTURE_DECODE_CASE(gr_bc::KIND_BC6H_SFLOAT, 4)
	default: return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_texture_decode: no kernel for format %u", block_format);
	}
#undef TEXTURE_DECODE_CASE
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
