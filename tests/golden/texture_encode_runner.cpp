// Drives the reference's own texture-compression code for tests/golden/make_texture_encode_golden.py.  Compiled only by that script,
// in a temporary directory, against the reference's sources: scene-export/rgtc_compressor.cpp as it is (its header included here) and
// the mip filter of scene-export/texture_utils.cpp.  That file cannot be compiled whole without the Vulkan headers its layout classes
// need, so the script copies the part of it that is the filter -- the TextureFormat* sample / write structs and the generate_mipmaps<Ops>
// template -- into mip_template.inc beside this file's object, and this file gives it the one class it asks for: a layout with the
// accessors the template calls, over a GTX payload (levels 16-byte aligned, layers inside a level).  The arithmetic is the reference's
// text through the reference's muglm; only where a texel lies in memory is answered here.
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <stdexcept>
#include <vector>
#include "muglm/muglm_impl.hpp"
#include "rgtc_compressor.hpp"

namespace Vulkan
{
class TextureFormatLayout
{
public:
	struct MipInfo
	{
		size_t offset = 0;
		uint32_t block_image_height = 0;
		uint32_t block_row_length = 0;
	};

	TextureFormatLayout(uint8_t *buffer_, uint32_t texel_bytes_, uint32_t width, uint32_t height, uint32_t layers_, uint32_t levels)
	    : buffer(buffer_), texel_bytes(texel_bytes_), layers(layers_)
	{
		size_t offset = 0;
		for (uint32_t l = 0; l < levels; l++)
		{
			offset = (offset + 15) & ~size_t(15);
			MipInfo info;
			info.offset = offset;
			info.block_row_length = std::max(width >> l, 1u);
			info.block_image_height = std::max(height >> l, 1u);
			mips.push_back(info);
			offset += size_t(info.block_row_length) * info.block_image_height * texel_bytes * layers;
		}
	}

	template <typename T>
	T *data_generic(uint32_t x, uint32_t y, uint32_t slice_index, uint32_t mip = 0) const
	{
		const MipInfo &info = mips[mip];
		T *slice = reinterpret_cast<T *>(buffer + info.offset);
		slice += size_t(slice_index) * info.block_row_length * info.block_image_height;
		return slice + size_t(y) * info.block_row_length + x;
	}

	void *data(uint32_t layer = 0, uint32_t mip = 0) const
	{
		const MipInfo &info = mips[mip];
		return buffer + info.offset + size_t(layer) * info.block_row_length * info.block_image_height * texel_bytes;
	}

	size_t get_layer_size(uint32_t mip) const { return size_t(mips[mip].block_row_length) * mips[mip].block_image_height * texel_bytes; }
	const MipInfo &get_mip_info(uint32_t mip) const { return mips[mip]; }
	uint32_t get_levels() const { return uint32_t(mips.size()); }
	uint32_t get_layers() const { return layers; }

private:
	uint8_t *buffer;
	uint32_t texel_bytes, layers;
	std::vector<MipInfo> mips;
};
} // namespace Vulkan

namespace Granite
{
using namespace muglm;
namespace SceneFormats
{
#include "mip_template.inc"
}
} // namespace Granite

extern "C" {
void ref_rgtc_compress_block(const uint8_t *texels16, uint8_t *out8) { Granite::compress_rgtc_red_block(out8, texels16); }
void ref_rgtc_decompress_block(const uint8_t *block8, uint8_t *out16) { Granite::decompress_rgtc_red_block(out16, block8); }

// What enqueue_compression_block_rgtc feeds the compressor: tightly packed pixels of `stride` bytes, coordinates clamped to the image.
// channels 1: BC4, 8 bytes a block; 2: BC5, red block then green block.
void ref_rgtc_compress_image(const uint8_t *pixels, int width, int height, int stride, int channels, uint8_t *blocks)
{
	for (int y = 0; y < height; y += 4)
	{
		for (int x = 0; x < width; x += 4)
		{
			uint8_t padded[2][16];
			for (int sy = 0; sy < 4; sy++)
				for (int sx = 0; sx < 4; sx++)
					for (int c = 0; c < channels; c++)
						padded[c][sy * 4 + sx] = pixels[size_t(stride) * (size_t(std::min(y + sy, height - 1)) * width + std::min(x + sx, width - 1)) + c];
			if (channels == 2)
				Granite::compress_rgtc_red_green_block(blocks, padded[0], padded[1]);
			else
				Granite::compress_rgtc_red_block(blocks, padded[0]);
			blocks += 8 * channels;
		}
	}
}

// `level0`: every layer of level 0, tightly packed.  `payload`: a GTX payload of `levels` levels, all of it written.
int ref_generate_mipmaps(uint8_t *payload, uint8_t *level0, int texel_bytes, int width, int height, int layers, int levels)
{
	Vulkan::TextureFormatLayout dst(payload, uint32_t(texel_bytes), uint32_t(width), uint32_t(height), uint32_t(layers), uint32_t(levels));
	Vulkan::TextureFormatLayout layout(level0, uint32_t(texel_bytes), uint32_t(width), uint32_t(height), uint32_t(layers), 1);
	switch (texel_bytes)
	{
	case 1: Granite::SceneFormats::generate_mipmaps(dst, layout, Granite::SceneFormats::TextureFormatUnorm8()); return 0;
	case 2: Granite::SceneFormats::generate_mipmaps(dst, layout, Granite::SceneFormats::TextureFormatRG8Unorm()); return 0;
	case 4: Granite::SceneFormats::generate_mipmaps(dst, layout, Granite::SceneFormats::TextureFormatRGBA8Unorm()); return 0;
	default: return -1;
	}
}
}
