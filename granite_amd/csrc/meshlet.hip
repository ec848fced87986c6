// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Mesh decode: assets/shaders/decode/meshlet_decode.comp as one gfx950 kernel.  The per-lane work is decode_lane() of
// meshlet_decode.hpp; this file holds the launch shape and the launcher's refusals.
//
// Shape: the shader's.  256 threads are eight meshlets of 32 lanes: a wave64 holds two meshlets, its halves diverge only where their
// counts differ.  A lane loads each 16-byte stream header it needs with one dwordx4 load at an address all 32 lanes of its meshlet
// share (one request per half-wave).  Stores are element-sized: bytes, shorts or dwords for indices, dwords for positions, one dwordx4
// per {normal, tangent, uv}, one dwordx2 per skin record; none rounds outward, since the neighbouring bytes belong to other lanes.
#include "ctx.hpp"
#include "meshlet_decode.hpp"

namespace
{
constexpr unsigned MESHLETS_PER_GROUP = 8;
constexpr unsigned GROUP_THREADS = MESHLETS_PER_GROUP * gr_meshlet::MAX_ELEMENTS;

template <int INDEX_BYTES, bool ALIGNED> __global__ __launch_bounds__(GROUP_THREADS) void k_meshlet_decode(const gr_meshlet::DecodeArgs a)
{
	const uint32_t meshlet = MESHLETS_PER_GROUP * (blockIdx.x + a.wg_offset) + (threadIdx.x >> 5);
	gr_meshlet::decode_lane<INDEX_BYTES, ALIGNED>(a, meshlet, threadIdx.x & 31u);
}
} // namespace

extern "C" int gr_meshlet_decode(gr_ctx *ctx, gr_stream stream, const gr_meshlet_decode_args *args, const gr_push_meshlet_decode *push)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, args);
	GR_CHECK_ARG(ctx, push);
	if (args->stream_count != 2u && args->stream_count != 4u && args->stream_count != 6u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_decode: stream_count %u is not 2, 4 or 6", args->stream_count);
	if (args->target_style > GR_MESHLET_STYLE_SKINNED)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_decode: target_style %u is not 0, 1 or 2", args->target_style);
	if (args->stream_count < 2u * args->target_style + 2u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_decode: target_style %u needs %u streams, stream_count is %u", args->target_style,
		                 2u * args->target_style + 2u, args->stream_count);
	if (args->flags & ~(GR_MESHLET_DECODE_UNROLLED_MESH | GR_MESHLET_DECODE_INDEX_16))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_decode: flags 0x%x holds bits that are no decode mode", args->flags);
	if (push->meshlet_count == 0u)
		return GR_OK;
	GR_CHECK_ARG(ctx, args->streams);
	GR_CHECK_ARG(ctx, args->payload);
	GR_CHECK_ARG(ctx, args->offsets);
	GR_CHECK_ARG(ctx, args->indices);
	GR_CHECK_ARG(ctx, args->positions);
	if (args->target_style >= GR_MESHLET_STYLE_TEXTURED)
		GR_CHECK_ARG(ctx, args->attributes);
	if (args->target_style >= GR_MESHLET_STYLE_SKINNED)
		GR_CHECK_ARG(ctx, args->skin);
	if (args->payload_words == 0u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_decode: the payload has zero words");
	const auto misaligned = [](const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) != 0u; };
	if (misaligned(args->streams, 16) || misaligned(args->payload, 4) || misaligned(args->offsets, 4) || misaligned(args->positions, 4) ||
	    misaligned(args->attributes, 16) || misaligned(args->skin, 8))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_meshlet_decode: a pointer is below its alignment (streams and attributes 16, skin 8, payload, offsets and positions 4 bytes)");

	const uint32_t groups = push->meshlet_count / MESHLETS_PER_GROUP + (push->meshlet_count % MESHLETS_PER_GROUP != 0u);
	if (push->wg_offset >= groups)
		return GR_OK;

	gr_meshlet::DecodeArgs a = {};
	a.streams = reinterpret_cast<const gr_meshlet::Stream *>(args->streams);
	a.payload = {args->payload, args->payload_words};
	a.offsets = reinterpret_cast<const gr_meshlet::Offsets *>(args->offsets);
	a.indices = static_cast<uint8_t *>(args->indices);
	a.positions = args->positions;
	a.attributes = static_cast<gr_meshlet::TexturedAttr *>(args->attributes);
	a.skin = static_cast<uint32_t *>(args->skin);
	a.index_capacity = args->index_capacity;
	a.position_capacity = args->position_capacity;
	a.attribute_capacity = args->attribute_capacity;
	a.skin_capacity = args->skin_capacity;
	a.primitive_offset = push->primitive_offset;
	a.vertex_offset = push->vertex_offset;
	a.meshlet_count = push->meshlet_count;
	a.wg_offset = push->wg_offset;
	a.stream_count = args->stream_count;
	a.target_style = args->target_style;

	const int index_bytes = (args->flags & GR_MESHLET_DECODE_UNROLLED_MESH) ? 4 : ((args->flags & GR_MESHLET_DECODE_INDEX_16) ? 2 : 1);
	const bool aligned = !misaligned(args->indices, uintptr_t(index_bytes));
	const dim3 grid(groups - push->wg_offset), block(GROUP_THREADS);
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "meshlet_decode"};
	if (index_bytes == 4)
		with_flags([&](auto al) { hipLaunchKernelGGL((k_meshlet_decode<4, decltype(al)::value>), grid, block, 0, s, a); }, aligned);
	else if (index_bytes == 2)
		with_flags([&](auto al) { hipLaunchKernelGGL((k_meshlet_decode<2, decltype(al)::value>), grid, block, 0, s, a); }, aligned);
	else
		hipLaunchKernelGGL((k_meshlet_decode<1, true>), grid, block, 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
