// The handful of Vulkan enumerants Granite's RenderGraph declarations mention (renderer/render_graph.hpp:124-251,
// renderer/post/hdr.cpp:313-353, ...), with Vulkan's numeric values, so pass-declaration code reads like the
// reference's without any Vulkan header.  Nothing here talks to a Vulkan driver.
#pragma once
#include <cstdint>

using VkFlags = uint32_t;
using VkFlags64 = uint64_t;
using VkDeviceSize = uint64_t;
using VkImageUsageFlags = VkFlags;
using VkBufferUsageFlags = VkFlags;
using VkPipelineStageFlags2 = VkFlags64;
using VkAccessFlags2 = VkFlags64;

enum VkFormat : uint32_t
{
	VK_FORMAT_UNDEFINED = 0,
	VK_FORMAT_R8_UNORM = 9,
	VK_FORMAT_R8G8_UNORM = 16,
	VK_FORMAT_R8G8B8A8_UNORM = 37,
	VK_FORMAT_R8G8B8A8_SRGB = 43,
	VK_FORMAT_B8G8R8A8_UNORM = 44,
	VK_FORMAT_B8G8R8A8_SRGB = 50,
	VK_FORMAT_A2B10G10R10_UNORM_PACK32 = 64,
	VK_FORMAT_R16_UNORM = 70,
	VK_FORMAT_R16_SFLOAT = 76,
	VK_FORMAT_R16G16_UNORM = 77,
	VK_FORMAT_R16G16_SFLOAT = 83,
	VK_FORMAT_R16G16B16A16_SFLOAT = 97,
	VK_FORMAT_R32_SFLOAT = 100,
	VK_FORMAT_R32G32_SFLOAT = 103,
	VK_FORMAT_B10G11R11_UFLOAT_PACK32 = 122,
	VK_FORMAT_D16_UNORM = 124,
	VK_FORMAT_D32_SFLOAT = 126,
	// Block-compressed: .gtx payloads and inputs of Granite::decode_compressed_image only (BC4 / BC5 SNORM are not handled)
	VK_FORMAT_BC1_RGB_UNORM_BLOCK = 131,
	VK_FORMAT_BC1_RGB_SRGB_BLOCK = 132,
	VK_FORMAT_BC1_RGBA_UNORM_BLOCK = 133,
	VK_FORMAT_BC1_RGBA_SRGB_BLOCK = 134,
	VK_FORMAT_BC2_UNORM_BLOCK = 135,
	VK_FORMAT_BC2_SRGB_BLOCK = 136,
	VK_FORMAT_BC3_UNORM_BLOCK = 137,
	VK_FORMAT_BC3_SRGB_BLOCK = 138,
	VK_FORMAT_BC4_UNORM_BLOCK = 139,
	VK_FORMAT_BC4_SNORM_BLOCK = 140, // named to be refused by name: no size, no decode
	VK_FORMAT_BC5_UNORM_BLOCK = 141,
	VK_FORMAT_BC5_SNORM_BLOCK = 142, // likewise
	VK_FORMAT_BC6H_UFLOAT_BLOCK = 143,
	VK_FORMAT_BC6H_SFLOAT_BLOCK = 144,
	VK_FORMAT_BC7_UNORM_BLOCK = 145,
	VK_FORMAT_BC7_SRGB_BLOCK = 146,
	// ASTC LDR, 2-D footprints: .gtx payloads and inputs of Granite::decode_compressed_image only
	VK_FORMAT_ASTC_4x4_UNORM_BLOCK = 157,
	VK_FORMAT_ASTC_4x4_SRGB_BLOCK = 158,
	VK_FORMAT_ASTC_5x4_UNORM_BLOCK = 159,
	VK_FORMAT_ASTC_5x4_SRGB_BLOCK = 160,
	VK_FORMAT_ASTC_5x5_UNORM_BLOCK = 161,
	VK_FORMAT_ASTC_5x5_SRGB_BLOCK = 162,
	VK_FORMAT_ASTC_6x5_UNORM_BLOCK = 163,
	VK_FORMAT_ASTC_6x5_SRGB_BLOCK = 164,
	VK_FORMAT_ASTC_6x6_UNORM_BLOCK = 165,
	VK_FORMAT_ASTC_6x6_SRGB_BLOCK = 166,
	VK_FORMAT_ASTC_8x5_UNORM_BLOCK = 167,
	VK_FORMAT_ASTC_8x5_SRGB_BLOCK = 168,
	VK_FORMAT_ASTC_8x6_UNORM_BLOCK = 169,
	VK_FORMAT_ASTC_8x6_SRGB_BLOCK = 170,
	VK_FORMAT_ASTC_8x8_UNORM_BLOCK = 171,
	VK_FORMAT_ASTC_8x8_SRGB_BLOCK = 172,
	VK_FORMAT_ASTC_10x5_UNORM_BLOCK = 173,
	VK_FORMAT_ASTC_10x5_SRGB_BLOCK = 174,
	VK_FORMAT_ASTC_10x6_UNORM_BLOCK = 175,
	VK_FORMAT_ASTC_10x6_SRGB_BLOCK = 176,
	VK_FORMAT_ASTC_10x8_UNORM_BLOCK = 177,
	VK_FORMAT_ASTC_10x8_SRGB_BLOCK = 178,
	VK_FORMAT_ASTC_10x10_UNORM_BLOCK = 179,
	VK_FORMAT_ASTC_10x10_SRGB_BLOCK = 180,
	VK_FORMAT_ASTC_12x10_UNORM_BLOCK = 181,
	VK_FORMAT_ASTC_12x10_SRGB_BLOCK = 182,
	VK_FORMAT_ASTC_12x12_UNORM_BLOCK = 183,
	VK_FORMAT_ASTC_12x12_SRGB_BLOCK = 184
};

enum VkImageUsageFlagBits : uint32_t
{
	VK_IMAGE_USAGE_TRANSFER_SRC_BIT = 0x1,
	VK_IMAGE_USAGE_TRANSFER_DST_BIT = 0x2,
	VK_IMAGE_USAGE_SAMPLED_BIT = 0x4,
	VK_IMAGE_USAGE_STORAGE_BIT = 0x8,
	VK_IMAGE_USAGE_COLOR_ATTACHMENT_BIT = 0x10,
	VK_IMAGE_USAGE_DEPTH_STENCIL_ATTACHMENT_BIT = 0x20,
	VK_IMAGE_USAGE_INPUT_ATTACHMENT_BIT = 0x80
};

enum VkBufferUsageFlagBits : uint32_t
{
	VK_BUFFER_USAGE_TRANSFER_SRC_BIT = 0x1,
	VK_BUFFER_USAGE_TRANSFER_DST_BIT = 0x2,
	VK_BUFFER_USAGE_UNIFORM_BUFFER_BIT = 0x10,
	VK_BUFFER_USAGE_STORAGE_BUFFER_BIT = 0x20,
	VK_BUFFER_USAGE_INDEX_BUFFER_BIT = 0x40,
	VK_BUFFER_USAGE_VERTEX_BUFFER_BIT = 0x80,
	VK_BUFFER_USAGE_INDIRECT_BUFFER_BIT = 0x100
};

// Stage/access masks are accepted and recorded for API compatibility; a HIP stream is in-order, so they never
// turn into barriers.
constexpr VkPipelineStageFlags2 VK_PIPELINE_STAGE_COMPUTE_SHADER_BIT = 0x800ull;
constexpr VkPipelineStageFlags2 VK_PIPELINE_STAGE_FRAGMENT_SHADER_BIT = 0x80ull;
constexpr VkPipelineStageFlags2 VK_PIPELINE_STAGE_2_COPY_BIT = 0x100000000ull;
constexpr VkAccessFlags2 VK_ACCESS_2_SHADER_STORAGE_WRITE_BIT = 0x400000000ull;
constexpr VkAccessFlags2 VK_ACCESS_2_SHADER_STORAGE_READ_BIT = 0x200000000ull;
constexpr VkAccessFlags2 VK_ACCESS_2_SHADER_SAMPLED_READ_BIT = 0x100000000ull;
constexpr VkAccessFlags2 VK_ACCESS_UNIFORM_READ_BIT = 0x8ull;
constexpr VkAccessFlags2 VK_ACCESS_TRANSFER_WRITE_BIT = 0x1000ull;

union VkClearColorValue
{
	float float32[4];
	int32_t int32[4];
	uint32_t uint32[4];
};

struct VkClearDepthStencilValue
{
	float depth;
	uint32_t stencil;
};

static inline unsigned vk_format_block_size(VkFormat format)
{
	switch (format)
	{
	case VK_FORMAT_R8_UNORM: return 1;
	case VK_FORMAT_R8G8_UNORM: return 2;
	case VK_FORMAT_D16_UNORM: return 2;
	case VK_FORMAT_R16_SFLOAT:
	case VK_FORMAT_R16_UNORM: return 2;
	case VK_FORMAT_R8G8B8A8_UNORM:
	case VK_FORMAT_R8G8B8A8_SRGB:
	case VK_FORMAT_B8G8R8A8_UNORM:
	case VK_FORMAT_B8G8R8A8_SRGB:
	case VK_FORMAT_R16G16_UNORM:
	case VK_FORMAT_A2B10G10R10_UNORM_PACK32:
	case VK_FORMAT_R16G16_SFLOAT:
	case VK_FORMAT_B10G11R11_UFLOAT_PACK32:
	case VK_FORMAT_R32_SFLOAT:
	case VK_FORMAT_D32_SFLOAT: return 4;
	case VK_FORMAT_R32G32_SFLOAT:
	case VK_FORMAT_R16G16B16A16_SFLOAT: return 8;
	case VK_FORMAT_BC1_RGB_UNORM_BLOCK:
	case VK_FORMAT_BC1_RGB_SRGB_BLOCK:
	case VK_FORMAT_BC1_RGBA_UNORM_BLOCK:
	case VK_FORMAT_BC1_RGBA_SRGB_BLOCK:
	case VK_FORMAT_BC4_UNORM_BLOCK: return 8;
	case VK_FORMAT_BC2_UNORM_BLOCK:
	case VK_FORMAT_BC2_SRGB_BLOCK:
	case VK_FORMAT_BC3_UNORM_BLOCK:
	case VK_FORMAT_BC3_SRGB_BLOCK:
	case VK_FORMAT_BC5_UNORM_BLOCK:
	case VK_FORMAT_BC6H_UFLOAT_BLOCK:
	case VK_FORMAT_BC6H_SFLOAT_BLOCK:
	case VK_FORMAT_BC7_UNORM_BLOCK:
	case VK_FORMAT_BC7_SRGB_BLOCK: return 16;
	default: return 0;
	}
}

static inline bool vk_format_is_astc_ldr(VkFormat format) { return format >= VK_FORMAT_ASTC_4x4_UNORM_BLOCK && format <= VK_FORMAT_ASTC_12x12_SRGB_BLOCK; }

// Bytes per block of a .gtx payload: vk_format_block_size, and 16 for the ASTC LDR formats.  vk_format_block_size itself keeps 0 for
// ASTC: it is also the texel size the image-argument contract knows a format by, and no image argument takes an ASTC format.
static inline unsigned vk_format_payload_block_size(VkFormat format) { return vk_format_is_astc_ldr(format) ? 16u : vk_format_block_size(format); }

// Texels per block: 4 x 4 for the BC formats above, the footprint for ASTC, 1 x 1 for everything else (vulkan/texture/texture_format.cpp
// format_block_dim).
static inline void vk_format_block_dim(VkFormat format, unsigned &width, unsigned &height)
{
	if (vk_format_is_astc_ldr(format))
	{
		static const unsigned char dims[14][2] = {{4, 4}, {5, 4}, {5, 5}, {6, 5}, {6, 6}, {8, 5}, {8, 6}, {8, 8}, {10, 5}, {10, 6}, {10, 8}, {10, 10}, {12, 10}, {12, 12}};
		const unsigned index = (unsigned(format) - unsigned(VK_FORMAT_ASTC_4x4_UNORM_BLOCK)) / 2;
		width = dims[index][0];
		height = dims[index][1];
		return;
	}
	const bool block = format >= VK_FORMAT_BC1_RGB_UNORM_BLOCK && format <= VK_FORMAT_BC7_SRGB_BLOCK && vk_format_block_size(format) != 0; // not SNORM
	width = height = block ? 4u : 1u;
}

static inline bool vk_format_is_srgb(VkFormat format) { return format == VK_FORMAT_R8G8B8A8_SRGB || format == VK_FORMAT_B8G8R8A8_SRGB; }
static inline bool vk_format_has_depth(VkFormat format) { return format == VK_FORMAT_D32_SFLOAT || format == VK_FORMAT_D16_UNORM; }
