// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// decode_mesh: the one part of host/mesh that touches the device (meshlet.cpp holds the view and the host arithmetic, and links without one).
#include "meshlet.hpp"
#include <cstring>

namespace Granite
{
namespace Meshlet
{
namespace
{
struct Staging // device and pinned memory of one decode, released together
{
	gr_ctx *ctx;
	gr_stream stream;
	void *device = nullptr, *pinned = nullptr;
	Staging(gr_ctx *ctx_, gr_stream stream_) : ctx(ctx_), stream(stream_) {}
	~Staging()
	{
		gr_sync(ctx, stream); // a launch that was enqueued before a later call failed still reads this memory
		if (device)
			gr_free(ctx, device);
		if (pinned)
			gr_free_host(ctx, pinned);
	}
	Staging(const Staging &) = delete;
	void operator=(const Staging &) = delete;
};
size_t align16(size_t v) { return (v + 15u) & ~size_t(15); }
} // namespace

bool decode_mesh(gr_ctx *ctx, gr_stream stream, const DecodeInfo &info, const MeshView &view, std::string *error)
{
	auto fail = [&](const char *what) {
		if (error)
			*error = what;
		return false;
	};
	if (!ctx || !view.format_header)
		return fail("decode_mesh: no context or no mesh view.");
	if (!info.streams[0].ptr)
		return fail("Decode stream 0 must be set.");
	if (!info.ibo.ptr)
		return fail("Output IBO must be set.");
	const FormatHeader &header = *view.format_header;
	if (header.meshlet_count == 0)
		return true;

	const std::vector<Offsets> decode_offsets = build_decode_offsets(view, info.runtime_style, info.flags);
	const size_t streams_size = size_t(header.meshlet_count) * header.stream_count * sizeof(Stream);
	const size_t payload_size = size_t(header.payload_size_words) * sizeof(PayloadWord);
	const size_t offsets_size = decode_offsets.size() * sizeof(Offsets);
	const size_t payload_at = align16(streams_size), offsets_at = payload_at + align16(payload_size), total = offsets_at + align16(offsets_size);

	Staging staging(ctx, stream);
	auto check = [&](int code) {
		if (code < 0 && error)
			*error = gr_last_error(ctx);
		return code >= 0;
	};
	if (!check(gr_alloc(ctx, total, &staging.device)) || !check(gr_alloc_host(ctx, total, &staging.pinned)))
		return false;
	auto *pinned = static_cast<uint8_t *>(staging.pinned);
	auto *device = static_cast<uint8_t *>(staging.device);
	memcpy(pinned, view.streams, streams_size);
	memcpy(pinned + payload_at, view.payload, payload_size);
	memcpy(pinned + offsets_at, decode_offsets.data(), offsets_size);
	const gr_upload_range ranges[3] = {{device, pinned, streams_size}, {device + payload_at, pinned + payload_at, payload_size},
	                                   {device + offsets_at, pinned + offsets_at, offsets_size}};
	if (!check(gr_upload_batch(ctx, stream, ranges, 3)))
		return false;

	const uint32_t index_bytes = (info.flags & DECODE_MODE_UNROLLED_MESH) ? 4u : ((info.flags & DECODE_MODE_INDEX_16) ? 2u : 1u);
	gr_meshlet_decode_args args = {};
	args.streams = reinterpret_cast<const gr_meshlet_stream *>(device);
	args.payload = reinterpret_cast<const uint32_t *>(device + payload_at);
	args.payload_words = header.payload_size_words;
	args.stream_count = header.stream_count;
	args.offsets = reinterpret_cast<const gr_meshlet_offsets *>(device + offsets_at);
	args.indices = info.ibo.ptr;
	args.index_capacity = info.ibo.size / (3u * index_bytes);
	args.positions = static_cast<float *>(info.streams[0].ptr);
	args.position_capacity = info.streams[0].size / 12u;
	args.attributes = info.streams[1].ptr;
	args.attribute_capacity = info.streams[1].size / 16u;
	args.skin = info.streams[2].ptr;
	args.skin_capacity = info.streams[2].size / 8u;
	args.target_style = uint32_t(info.target_style);
	args.flags = info.flags;
	const gr_push_meshlet_decode push = {info.push.primitive_offset, info.push.vertex_offset, header.meshlet_count, 0};
	if (!check(gr_meshlet_decode(ctx, stream, &args, &push)))
		return false;

	if (info.indirect.ptr)
	{
		const std::vector<uint8_t> records = build_indirect_records(view, info.runtime_style, info.push.primitive_offset, info.push.vertex_offset);
		const uint64_t at = uint64_t(info.indirect_offset) * indirect_stride(info.runtime_style);
		if (at + records.size() > info.indirect.size)
			return fail("decode_mesh: the indirect buffer is smaller than indirect_offset plus the mesh's chunks.");
		if (!check(gr_upload(ctx, stream, static_cast<uint8_t *>(info.indirect.ptr) + at, records.data(), records.size())))
			return false;
	}
	return check(gr_sync(ctx, stream)); // the staging memory is read by the launches above
}
} // namespace Meshlet
} // namespace Granite
