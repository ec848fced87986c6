// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "texture_compression.hpp"
#include <cstring>
#include <stdexcept>

namespace Granite
{
VkFormat string_to_format(const std::string &s)
{
	if (s == "bc4_unorm")
		return VK_FORMAT_BC4_UNORM_BLOCK;
	if (s == "bc5_unorm")
		return VK_FORMAT_BC5_UNORM_BLOCK;
	if (s == "rgba8_unorm")
		return VK_FORMAT_R8G8B8A8_UNORM;
	if (s == "rg8_unorm")
		return VK_FORMAT_R8G8_UNORM;
	if (s == "r8_unorm")
		return VK_FORMAT_R8_UNORM;
	return VK_FORMAT_UNDEFINED;
}

uint32_t num_miplevels(uint32_t width, uint32_t height)
{
	uint32_t size = width > height ? width : height, levels = 0;
	while (size)
	{
		levels++;
		size >>= 1;
	}
	return levels;
}

GtxImage compressed_layout(const GtxImage &input, VkFormat format)
{
	GtxImage out = input;
	out.format = format;
	out.payload.assign(out.required_payload_size(), 0);
	return out;
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

void check(gr_ctx *ctx, int code)
{
	if (code < 0)
		throw std::runtime_error(gr_last_error(ctx));
}

bool is_unorm8(VkFormat f) { return f == VK_FORMAT_R8_UNORM || f == VK_FORMAT_R8G8_UNORM || f == VK_FORMAT_R8G8B8A8_UNORM; }

// One layer of one level of an uncompressed image inside a device copy of its payload.
gr_image level_view(const GtxImage &img, void *payload, uint32_t level, uint32_t layer)
{
	const uint32_t texel = vk_format_block_size(img.format), width = img.level_width(level), height = img.level_height(level);
	gr_image view = {};
	view.ptr = static_cast<uint8_t *>(payload) + img.level_offset(level) + size_t(layer) * width * height * texel;
	view.width = width;
	view.height = height;
	view.pitch_bytes = width * texel;
	view.format = uint32_t(img.format);
	return view;
}
} // namespace

GtxImage generate_mipmaps(gr_ctx *ctx, gr_stream stream, const GtxImage &input)
{
	if (input.type == 2 || input.depth != 1)
		throw std::runtime_error("3D is not supported for generate_mipmaps.");
	if (!is_unorm8(input.format))
		throw std::runtime_error("Unsupported format for generate_mipmaps.");
	if (input.payload.size() != input.required_payload_size())
		throw std::runtime_error("The payload does not match the image's layout.");

	GtxImage out = input;
	out.levels = num_miplevels(input.width, input.height);
	out.flags = input.flags & ~2u; // MEMORY_MAPPED_TEXTURE_GENERATE_MIPMAP_ON_LOAD_BIT
	out.payload.assign(out.required_payload_size(), 0);

	DeviceMemory chain(ctx, out.payload.size());
	memcpy(out.payload.data(), input.payload.data(), input.level_size(0)); // level 0 of both starts at offset 0
	check(ctx, gr_upload(ctx, stream, chain.ptr, out.payload.data(), out.payload.size())); // with the zeros between the levels, which no launch writes
	for (uint32_t level = 1; level < out.levels; level++)
	{
		for (uint32_t layer = 0; layer < out.layers; layer++)
		{
			const gr_image src = level_view(out, chain.ptr, level - 1, layer), dst = level_view(out, chain.ptr, level, layer);
			check(ctx, gr_texture_generate_mipmap(ctx, stream, &src, &dst));
		}
	}
	check(ctx, gr_download(ctx, stream, out.payload.data(), chain.ptr, out.payload.size())); // waits for the stream
	return out;
}

GtxImage compress_texture(gr_ctx *ctx, gr_stream stream, const CompressorArguments &args, const GtxImage &input)
{
	if (input.type == 2 || input.depth != 1)
		throw std::runtime_error("3-D images cannot be compressed.");
	if (input.payload.size() != input.required_payload_size())
		throw std::runtime_error("The payload does not match the image's layout.");
	if (args.format == input.format && vk_format_block_size(input.format) <= 4 && gr_texture_encode_supported(VK_FORMAT_BC4_UNORM_BLOCK, uint32_t(input.format)))
	{
		// enqueue_compression_copy_8bit with equal strides: texel by texel the same bytes
		GtxImage out = compressed_layout(input, args.format);
		for (uint32_t level = 0; level < input.levels; level++)
			memcpy(out.payload.data() + out.level_offset(level), input.payload.data() + input.level_offset(level), input.level_size(level));
		return out;
	}
	if (!gr_texture_encode_supported(uint32_t(args.format), uint32_t(input.format)))
		throw std::runtime_error("compress_texture: format " + std::to_string(unsigned(input.format)) + " cannot be compressed to format " +
		                         std::to_string(unsigned(args.format)) + " (BC4 from R8 / RG8 / RGBA8, BC5 from RG8 / RGBA8).");

	GtxImage out = compressed_layout(input, args.format);
	DeviceMemory texels(ctx, input.payload.size()), blocks(ctx, out.payload.size());
	check(ctx, gr_upload(ctx, stream, texels.ptr, input.payload.data(), input.payload.size()));
	check(ctx, gr_upload(ctx, stream, blocks.ptr, out.payload.data(), out.payload.size())); // zeros: the bytes between levels are never written
	const uint32_t block_bytes = vk_format_payload_block_size(args.format);
	for (uint32_t level = 0; level < input.levels; level++)
	{
		const uint32_t block_pitch = out.level_blocks_x(level) * block_bytes;
		const size_t block_layer = size_t(block_pitch) * out.level_blocks_y(level);
		for (uint32_t layer = 0; layer < input.layers; layer++)
		{
			const gr_image view = level_view(input, texels.ptr, level, layer);
			check(ctx, gr_texture_encode(ctx, stream, uint32_t(args.format), &view,
			                             static_cast<uint8_t *>(blocks.ptr) + out.level_offset(level) + layer * block_layer, block_pitch));
		}
	}
	check(ctx, gr_download(ctx, stream, out.payload.data(), blocks.ptr, out.payload.size())); // waits for the stream
	return out;
}
} // namespace Granite
