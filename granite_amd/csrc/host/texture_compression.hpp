// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// scene-export/texture_compression.hpp and texture_utils.hpp restated over the C ABI for the part of them that is the reference's own
// code: BC4 / BC5 (gr_texture_encode), the 8-bit copy, and UNORM8 mip chains (gr_texture_generate_mipmap).  Images travel as GtxImage.
#pragma once
#include <string>
#include "../../../include/granite_hip.h"
#include "gtx.hpp"

namespace Granite
{
// texture_compression.cpp:46-109 for the names this build handles: bc4_unorm, bc5_unorm, r8_unorm, rg8_unorm, rgba8_unorm.  Every other
// name, those of the reference's table that need an encoder library included (bc1 / bc3 / bc6h / bc7 / astc_*, the float and srgb copies),
// gives VK_FORMAT_UNDEFINED.
VkFormat string_to_format(const std::string &s);

// The one field of the reference's CompressorArguments that this build acts on.
struct CompressorArguments
{
	VkFormat format = VK_FORMAT_UNDEFINED;
};

// Levels of a full chain: texture_format.cpp:30-40 for a 2-D image.
uint32_t num_miplevels(uint32_t width, uint32_t height);

// The layout compress_texture gives its output: the input's type, extents, layers, levels and flags with the target format; the payload
// sized for it and zeroed.  No device.
GtxImage compressed_layout(const GtxImage &input, VkFormat format);

// texture_utils.cpp:324-333: level 0 of every layer copied, then the full chain filtered level by level, one
// gr_texture_generate_mipmap per level and layer on `stream`.  A chain the input already has is dropped and made again from level 0.
// R8_UNORM, R8G8_UNORM and R8G8B8A8_UNORM; the mipgen-on-load flag is cleared, the other flags are kept.  Throws std::runtime_error for
// another format ("Unsupported format for generate_mipmaps.") and for 3-D images.
GtxImage generate_mipmaps(gr_ctx *ctx, gr_stream stream, const GtxImage &input);

// compress_texture (texture_compression.cpp:787-930): every layer and level of `input` to args.format, one gr_texture_encode each; where
// args.format is the input's own uncompressed 8-bit format, the copy of enqueue_compression_copy_8bit.  The reference insists on an RGBA8
// input; here R8_UNORM and R8G8_UNORM are taken as well (BC4 from either, BC5 from R8G8), since the compressor reads one or two
// components and the project's own attachments are stored that way.  Throws std::runtime_error for a pair of formats
// gr_texture_encode_supported refuses and for 3-D images.
GtxImage compress_texture(gr_ctx *ctx, gr_stream stream, const CompressorArguments &args, const GtxImage &input);
} // namespace Granite
