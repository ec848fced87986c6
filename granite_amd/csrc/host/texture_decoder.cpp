// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "texture_decoder.hpp"
#include <stdexcept>
#include <string>

namespace Granite
{
VkFormat compressed_format_to_decoded_format(VkFormat format)
{
	uint32_t block_bytes = 0, decoded = 0;
	return gr_texture_block_info(uint32_t(format), &block_bytes, &decoded) < 0 ? VK_FORMAT_UNDEFINED : VkFormat(decoded);
}

namespace
{
struct DeviceMemory
{
	gr_ctx *ctx;
	void *ptr = nullptr;
	DeviceMemory(gr_ctx *ctx_, size_t size) : ctx(ctx_)
	{
		if (gr_alloc(ctx, size, &ptr) < 0)
			throw std::runtime_error(gr_last_error(ctx));
	}
	~DeviceMemory() { gr_free(ctx, ptr); }
	DeviceMemory(const DeviceMemory &) = delete;
	void operator=(const DeviceMemory &) = delete;
};
} // namespace

GtxImage decode_compressed_image(gr_ctx *ctx, gr_stream stream, const GtxImage &compressed)
{
	if (compressed.format == VK_FORMAT_BC4_SNORM_BLOCK || compressed.format == VK_FORMAT_BC5_SNORM_BLOCK)
		throw std::runtime_error("SNORM formats are not supported.");
	const VkFormat decoded = compressed_format_to_decoded_format(compressed.format);
	if (decoded == VK_FORMAT_UNDEFINED)
		throw std::runtime_error("Not a compressed format (format " + std::to_string(unsigned(compressed.format)) + ").");
	if (compressed.type == 2 || compressed.depth != 1)
		throw std::runtime_error("3-D images cannot be decoded.");
	if (compressed.payload.size() != compressed.required_payload_size())
		throw std::runtime_error("The compressed payload does not match the image's layout.");

	GtxImage out = compressed;
	out.format = decoded;
	out.payload.assign(out.required_payload_size(), 0);

	DeviceMemory blocks(ctx, compressed.payload.size()), texels(ctx, out.payload.size());
	auto check = [&](int code) {
		if (code < 0)
			throw std::runtime_error(gr_last_error(ctx));
	};
	check(gr_upload(ctx, stream, blocks.ptr, compressed.payload.data(), compressed.payload.size()));
	uint32_t block_bytes = 0, decoded_again = 0;
	check(gr_texture_block_info(uint32_t(compressed.format), &block_bytes, &decoded_again));
	const uint32_t texel_bytes = vk_format_block_size(decoded);
	for (uint32_t level = 0; level < compressed.levels; level++)
	{
		const uint32_t width = compressed.level_width(level), height = compressed.level_height(level);
		const uint32_t block_pitch = compressed.level_blocks_x(level) * block_bytes;
		const size_t block_layer = size_t(block_pitch) * compressed.level_blocks_y(level), texel_layer = size_t(width) * height * texel_bytes;
		for (uint32_t layer = 0; layer < compressed.layers; layer++)
		{
			gr_image view = {};
			view.ptr = static_cast<uint8_t *>(texels.ptr) + out.level_offset(level) + layer * texel_layer;
			view.width = width;
			view.height = height;
			view.pitch_bytes = width * texel_bytes;
			view.format = uint32_t(decoded);
			check(gr_texture_decode(ctx, stream, uint32_t(compressed.format),
			                        static_cast<const uint8_t *>(blocks.ptr) + compressed.level_offset(level) + layer * block_layer, block_pitch, &view));
		}
	}
	check(gr_download(ctx, stream, out.payload.data(), texels.ptr, out.payload.size())); // waits for the stream
	return out;
}
} // namespace Granite
