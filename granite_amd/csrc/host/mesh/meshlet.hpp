// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// vulkan/mesh/meshlet.hpp restated over the C ABI of include/granite_hip.h: the MESHLET4 container, create_mesh_view and decode_mesh.
// A Vulkan::Buffer becomes a device pointer with its size; cmd.dispatch becomes gr_meshlet_decode; the names are Granite's.
// The Offsets array, the index_offset rules and both indirect layouts are host arithmetic in functions of their own
// (build_decode_offsets, build_indirect_records) that need no device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "../../../../include/granite_hip.h"

namespace Granite
{
namespace Meshlet
{
static constexpr unsigned MaxStreams = 8;
static constexpr unsigned MaxElements = 32;
static constexpr unsigned ChunkFactor = 256 / MaxElements;

struct Stream
{
	union
	{
		uint32_t base_value[2];
		struct
		{
			uint32_t prim_count;
			uint32_t vert_count;
		} counts;
	} u;
	uint32_t bits;
	uint32_t offset_in_words;
};
static_assert(sizeof(Stream) == 16 && sizeof(Stream) == sizeof(gr_meshlet_stream), "Unexpected Stream size.");

struct RuntimeHeaderDecoded
{
	uint32_t primitive_offset;
	uint32_t vertex_offset;
	uint32_t primitive_count;
	uint32_t vertex_count;
};

struct RuntimeHeaderDecodedMDI
{
	uint32_t indexCount;
	uint32_t firstIndex;
	int32_t vertexOffset;
};

struct Bound
{
	float center[3];
	float radius;
	float cone_axis_cutoff[4];
};

enum class StreamType
{
	Primitive = 0,     // RGB8_UINT (fixed 5-bit encoding, fixed base value of 0)
	Position,          // RGB16_SINT * 2^aux
	NormalTangentOct8, // octahedron encoding in RG8, BA8 for the tangent; aux selects the tangent's sign
	UV,                // 0.5 * (R16G16_SINT * 2^aux) + 0.5
	BoneIndices,       // RGBA8_UINT
	BoneWeights,       // RGBA8_UNORM
};

enum class MeshStyle : uint32_t
{
	Wireframe = 0, // Primitive + Position
	Textured,      // Wireframe + NormalTangentOct8 + UV
	Skinned        // Textured + Bone*
};

struct FormatHeader
{
	MeshStyle style;
	uint32_t stream_count;
	uint32_t meshlet_count;
	uint32_t payload_size_words;
};

using PayloadWord = uint32_t;

struct MeshView
{
	const FormatHeader *format_header;
	const Bound *bounds;
	const Bound *bounds_256;
	const Stream *streams;
	const PayloadWord *payload;
	uint32_t total_primitives;
	uint32_t total_vertices;
	uint32_t num_bounds;
	uint32_t num_bounds_256;
};

static const char magic[8] = {'M', 'E', 'S', 'H', 'L', 'E', 'T', '4'};

// A view over `size` bytes at `data` (4-byte aligned), which must outlive it.  On refusal format_header is null and *error, where
// given, says why.  The reference's size checks (a missing padding word after the payload is accepted), and what the device path cannot
// do without, each naming the meshlet and the stream: a style or stream count the decoder does not know, counts above 32, bits & 0xff
// above the component width (16 for positions and UV, 8 for the byte streams), a stream whose elements span words past
// payload_size_words.
MeshView create_mesh_view(const void *data, size_t size, std::string *error = nullptr);

enum DecodeModeFlagBits : uint32_t
{
	DECODE_MODE_UNROLLED_MESH = 1 << 0,
	DECODE_MODE_INDEX_16 = 1 << 1,
};
using DecodeModeFlags = uint32_t;

enum class RuntimeStyle
{
	MDI,
	Meshlet
};

struct DeviceBuffer // Vulkan::Buffer: device memory and its size
{
	void *ptr = nullptr;
	uint64_t size = 0;
};

struct DecodeInfo
{
	DeviceBuffer ibo, streams[3]; // streams: positions, {normal, tangent, uv}, skin
	DeviceBuffer indirect;        // optional
	DecodeModeFlags flags = 0;
	MeshStyle target_style = MeshStyle::Wireframe;
	RuntimeStyle runtime_style = RuntimeStyle::MDI;

	struct
	{
		uint32_t primitive_offset = 0;
		uint32_t vertex_offset = 0;
	} push;
	uint32_t indirect_offset = 0; // in chunks
};

struct Offsets
{
	uint32_t primitive_output_offset;
	uint32_t vertex_output_offset;
	uint32_t index_offset;
};
static_assert(sizeof(Offsets) == sizeof(gr_meshlet_offsets), "Offsets is the kernel's record");

// decode_mesh's per-meshlet offsets.  index_offset: the Meshlet runtime never grows it, MDI grows it by vert_count, MDI that is not
// unrolled restarts it at every chunk of ChunkFactor meshlets.
std::vector<Offsets> build_decode_offsets(const MeshView &view, RuntimeStyle runtime_style, DecodeModeFlags flags);
// upload_indirect_buffer's records as bytes: RuntimeHeaderDecoded per meshlet, zero-padded to whole chunks, or one
// RuntimeHeaderDecodedMDI per chunk.
std::vector<uint8_t> build_indirect_records(const MeshView &view, RuntimeStyle runtime_style, uint32_t primitive_offset, uint32_t vertex_offset);
size_t indirect_stride(RuntimeStyle runtime_style); // bytes per chunk

// Uploads the stream headers, the payload and the Offsets array (one gr_upload_batch), launches gr_meshlet_decode once, writes the
// indirect records where info.indirect is set, and waits for `stream`: the staging memory is released on return.  Output capacities are
// the buffers' sizes in whole elements.  false (gr_last_error(ctx) or *error say why) where the reference returns false or a call fails.
bool decode_mesh(gr_ctx *ctx, gr_stream stream, const DecodeInfo &info, const MeshView &view, std::string *error = nullptr);
} // namespace Meshlet
} // namespace Granite
