// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// renderer/utils/image_utils.hpp restated over the C ABI: the three environment bakes (gr_env_equirect_to_cube, gr_env_specular,
// gr_env_diffuse).  Images travel as GtxImage: a cube is type 2-D, 6 layers, MEMORY_MAPPED_TEXTURE_CUBE_MAP_COMPATIBLE_BIT set in
// flags (what MemoryMappedTexture::set_cube writes), R16G16B16A16_SFLOAT, its payload the chain the kernels read and write.
#pragma once
#include "../../../../include/granite_hip.h"
#include "../gtx.hpp"

namespace Granite
{
constexpr uint32_t MEMORY_MAPPED_TEXTURE_CUBE_MAP_COMPATIBLE_BIT = 1u << 0;

// image_utils.cpp:165-223.  `image`: a 2-D R16G16B16A16_SFLOAT image (level 0 is read).  The cube is
// unsigned(scale * max(width / 3, height / 2)) texels a side with a full mip chain.
GtxImage convert_equirect_to_cube(gr_ctx *ctx, gr_stream stream, const GtxImage &image, float scale);
// image_utils.cpp:37-105: 128 texels a side, 8 levels.
GtxImage convert_cube_to_ibl_specular(gr_ctx *ctx, gr_stream stream, const GtxImage &cube);
// image_utils.cpp:107-163: 32 texels a side, 1 level.
GtxImage convert_cube_to_ibl_diffuse(gr_ctx *ctx, gr_stream stream, const GtxImage &cube);
// Each is one upload, one call and one download, and throws std::runtime_error with the reason where the C ABI refuses.
} // namespace Granite
