// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// vulkan/texture/texture_decoder.hpp restated over the C ABI: block-compressed GTX images expanded on the device (gr_texture_decode).
#pragma once
#include "../../../include/granite_hip.h"
#include "gtx.hpp"

namespace Granite
{
// texture_decoder.cpp:28-129 for the formats handled here: BC1/2/3/7 -> R8G8B8A8_UNORM / _SRGB, BC4 -> R8_UNORM, BC5 -> R8G8_UNORM,
// BC6H -> R16G16B16A16_SFLOAT, ASTC LDR -> R8G8B8A8_UNORM / _SRGB; VK_FORMAT_UNDEFINED for everything else (the SNORM forms, ETC2 / EAC
// and the ASTC SFLOAT forms included).
VkFormat compressed_format_to_decoded_format(VkFormat format);

// decode_compressed_image (texture_decoder.cpp:1290-1424): one upload of the whole payload, one gr_texture_decode per level and layer
// on `stream`, one download.  Same type, extents, layers, levels and flags (component swizzle kept verbatim); the format is the decoded
// one and the payload is in GTX layout.  Throws std::runtime_error for a format that is not block-compressed ("Not a compressed
// format"), for SNORM and for 3-D images.
GtxImage decode_compressed_image(gr_ctx *ctx, gr_stream stream, const GtxImage &compressed);
} // namespace Granite
