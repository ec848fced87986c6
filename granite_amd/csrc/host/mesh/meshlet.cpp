// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "meshlet.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>

namespace Granite
{
namespace Meshlet
{
static MeshView refuse(std::string *error, const char *fmt, unsigned a = 0, unsigned b = 0, unsigned c = 0, unsigned d = 0, unsigned e = 0)
{
	if (error)
	{
		char buf[256];
		snprintf(buf, sizeof(buf), fmt, a, b, c, d, e);
		*error = buf;
	}
	return {};
}

MeshView create_mesh_view(const void *data, size_t size, std::string *error)
{
	MeshView view = {};
	if (size < sizeof(magic) + sizeof(FormatHeader))
		return refuse(error, "MESHLET4 file too small.");
	if (!data || (reinterpret_cast<uintptr_t>(data) & 3u))
		return refuse(error, "MESHLET4 data is null or not 4-byte aligned.");

	auto *ptr = static_cast<const unsigned char *>(data);
	auto *end_ptr = ptr + size;
	if (memcmp(ptr, magic, sizeof(magic)) != 0)
		return refuse(error, "Invalid MESHLET4 magic.");
	ptr += sizeof(magic);

	view.format_header = reinterpret_cast<const FormatHeader *>(ptr);
	ptr += sizeof(*view.format_header);
	const FormatHeader &header = *view.format_header;
	if (uint32_t(header.style) > uint32_t(MeshStyle::Skinned))
		return refuse(error, "MESHLET4 style %u is not Wireframe, Textured or Skinned.", uint32_t(header.style));
	if (header.stream_count != 2u * uint32_t(header.style) + 2u)
		return refuse(error, "MESHLET4 style %u has %u streams, not %u.", uint32_t(header.style), 2u * uint32_t(header.style) + 2u, header.stream_count);

	// sizes in 64 bits: the counts are the file's
	const uint64_t left = uint64_t(end_ptr - ptr);
	const uint64_t bounds_size = uint64_t(header.meshlet_count) * sizeof(Bound);
	if (left < bounds_size)
		return refuse(error, "MESHLET4 file ends inside the %u meshlet bounds.", header.meshlet_count);
	view.bounds = reinterpret_cast<const Bound *>(ptr);
	ptr += bounds_size;

	const uint64_t num_bounds_256 = (uint64_t(header.meshlet_count) + ChunkFactor - 1) / ChunkFactor;
	if (uint64_t(end_ptr - ptr) < num_bounds_256 * sizeof(Bound))
		return refuse(error, "MESHLET4 file ends inside the %u chunk bounds.", unsigned(num_bounds_256));
	view.bounds_256 = reinterpret_cast<const Bound *>(ptr);
	ptr += num_bounds_256 * sizeof(Bound);
	view.num_bounds = header.meshlet_count;
	view.num_bounds_256 = uint32_t(num_bounds_256);

	const uint64_t streams_size = uint64_t(header.meshlet_count) * header.stream_count * sizeof(Stream);
	if (uint64_t(end_ptr - ptr) < streams_size)
		return refuse(error, "MESHLET4 file ends inside the stream headers (%u meshlets of %u streams).", header.meshlet_count, header.stream_count);
	view.streams = reinterpret_cast<const Stream *>(ptr);
	ptr += streams_size;

	if (!header.payload_size_words)
		return refuse(error, "MESHLET4 payload has zero words.");
	if (uint64_t(end_ptr - ptr) < uint64_t(header.payload_size_words) * sizeof(PayloadWord))
		return refuse(error, "MESHLET4 file ends inside the payload of %u words.", header.payload_size_words);
	view.payload = reinterpret_cast<const PayloadWord *>(ptr);

	static const unsigned components[6] = {3, 3, 4, 2, 4, 4}, width[6] = {5, 16, 8, 16, 8, 8};
	for (uint32_t i = 0, n = header.meshlet_count; i < n; i++)
	{
		const Stream *streams = view.streams + size_t(i) * header.stream_count;
		const auto counts = streams[0].u.counts;
		if (counts.prim_count > MaxElements || counts.vert_count > MaxElements)
			return refuse(error, "MESHLET4 meshlet %u, stream 0: counts %u and %u are above 32.", i, counts.prim_count, counts.vert_count);
		for (uint32_t s = 0; s < header.stream_count; s++)
		{
			const uint32_t bits = s == 0 ? 5u : (streams[s].bits & 0xffu);
			if (bits > width[s])
				return refuse(error, "MESHLET4 meshlet %u, stream %u: %u bits per component, above the stream's %u.", i, s, bits, width[s]);
			const uint32_t count = s == 0 ? counts.prim_count : counts.vert_count;
			const uint64_t words = (uint64_t(count) * components[s] * bits + 31u) / 32u;
			if (uint64_t(streams[s].offset_in_words) + words > header.payload_size_words)
				return refuse(error, "MESHLET4 meshlet %u, stream %u: words %u + %u lie past the payload's %u.", i, s, streams[s].offset_in_words, unsigned(words),
				              header.payload_size_words);
		}
		view.total_primitives += counts.prim_count;
		view.total_vertices += counts.vert_count;
	}
	return view;
}

std::vector<Offsets> build_decode_offsets(const MeshView &view, RuntimeStyle runtime_style, DecodeModeFlags flags)
{
	std::vector<Offsets> decode_offsets;
	Offsets offsets = {};
	const bool meshlet_runtime = runtime_style == RuntimeStyle::Meshlet;
	decode_offsets.reserve(view.format_header->meshlet_count);
	for (uint32_t i = 0; i < view.format_header->meshlet_count; i++)
	{
		if (runtime_style == RuntimeStyle::MDI && (flags & DECODE_MODE_UNROLLED_MESH) == 0 && (i & (ChunkFactor - 1)) == 0)
			offsets.index_offset = 0;
		decode_offsets.push_back(offsets);
		const auto &counts = view.streams[size_t(i) * view.format_header->stream_count].u.counts;
		offsets.primitive_output_offset += counts.prim_count;
		offsets.vertex_output_offset += counts.vert_count;
		if (!meshlet_runtime)
			offsets.index_offset += counts.vert_count;
	}
	return decode_offsets;
}

size_t indirect_stride(RuntimeStyle runtime_style)
{
	return runtime_style == RuntimeStyle::Meshlet ? sizeof(RuntimeHeaderDecoded) * ChunkFactor : sizeof(RuntimeHeaderDecodedMDI);
}

std::vector<uint8_t> build_indirect_records(const MeshView &view, RuntimeStyle runtime_style, uint32_t primitive_offset, uint32_t vertex_offset)
{
	const size_t total_meshlets = view.format_header->meshlet_count;
	const uint32_t stream_count = view.format_header->stream_count;
	std::vector<uint8_t> out(view.num_bounds_256 * indirect_stride(runtime_style), 0); // the last chunk's tail stays zero
	uint32_t prim_offset = primitive_offset, vert_offset = vertex_offset;
	if (runtime_style == RuntimeStyle::Meshlet)
	{
		for (size_t i = 0; i < total_meshlets; i++)
		{
			const auto &counts = view.streams[i * stream_count].u.counts;
			const RuntimeHeaderDecoded header = {prim_offset, vert_offset, counts.prim_count, counts.vert_count};
			memcpy(out.data() + i * sizeof(header), &header, sizeof(header));
			prim_offset += counts.prim_count;
			vert_offset += counts.vert_count;
		}
		return out;
	}
	for (size_t i = 0; i < view.num_bounds_256; i++)
	{
		const size_t chunks = std::min<size_t>(total_meshlets - i * ChunkFactor, ChunkFactor);
		RuntimeHeaderDecodedMDI draw = {};
		draw.firstIndex = 3 * prim_offset;
		draw.vertexOffset = int32_t(vert_offset);
		for (size_t chunk = 0; chunk < chunks; chunk++)
		{
			const auto &counts = view.streams[(i * ChunkFactor + chunk) * stream_count].u.counts;
			draw.indexCount += counts.prim_count;
			vert_offset += counts.vert_count;
			prim_offset += counts.prim_count;
		}
		draw.indexCount *= 3;
		memcpy(out.data() + i * sizeof(draw), &draw, sizeof(draw));
	}
	return out;
}

} // namespace Meshlet
} // namespace Granite
