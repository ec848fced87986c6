// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "image_utils.hpp"
#include <algorithm>
#include <stdexcept>
#include <string>

namespace Granite
{
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

GtxImage make_cube(uint32_t size, uint32_t levels)
{
	GtxImage cube;
	cube.format = VK_FORMAT_R16G16B16A16_SFLOAT;
	cube.width = cube.height = size;
	cube.layers = 6;
	cube.levels = levels;
	cube.flags = MEMORY_MAPPED_TEXTURE_CUBE_MAP_COMPATIBLE_BIT;
	cube.payload.assign(size_t(gr_cube_chain_bytes(size, levels)), 0);
	if (cube.payload.size() != cube.required_payload_size())
		throw std::logic_error("a cube chain is not the GTX payload of its image");
	return cube;
}

void require_cube(const GtxImage &cube, const char *who)
{
	if (cube.format != VK_FORMAT_R16G16B16A16_SFLOAT)
		throw std::runtime_error(std::string(who) + ": the cube is not R16G16B16A16_SFLOAT (format " + std::to_string(unsigned(cube.format)) + ").");
	if (cube.type != 1 || cube.depth != 1 || cube.layers != 6 || cube.width != cube.height || cube.width == 0)
		throw std::runtime_error(std::string(who) + ": not a cube (2-D, square, 6 layers).");
	if (cube.payload.size() != cube.required_payload_size() || cube.payload.size() != gr_cube_chain_bytes(cube.width, cube.levels))
		throw std::runtime_error(std::string(who) + ": the cube's payload does not match its layout.");
}

// One upload of `src`, fn(device source, device output), one download of an out_size / out_levels cube.
template <typename Fn> GtxImage bake(gr_ctx *ctx, gr_stream stream, const GtxImage &src, uint32_t out_size, uint32_t out_levels, Fn &&fn)
{
	GtxImage out = make_cube(out_size, out_levels);
	DeviceMemory in(ctx, src.payload.size()), result(ctx, out.payload.size());
	check(ctx, gr_upload(ctx, stream, in.ptr, src.payload.data(), src.payload.size()));
	check(ctx, fn(in.ptr, result.ptr));
	check(ctx, gr_download(ctx, stream, out.payload.data(), result.ptr, out.payload.size())); // waits for the stream
	return out;
}
} // namespace

GtxImage convert_equirect_to_cube(gr_ctx *ctx, gr_stream stream, const GtxImage &image, float scale)
{
	if (image.format != VK_FORMAT_R16G16B16A16_SFLOAT)
		throw std::runtime_error("convert_equirect_to_cube: the equirect image is not R16G16B16A16_SFLOAT (format " + std::to_string(unsigned(image.format)) + ").");
	if (image.type != 1 || image.depth != 1 || image.layers != 1)
		throw std::runtime_error("convert_equirect_to_cube: the equirect image is not a single 2-D image.");
	if (image.payload.size() != image.required_payload_size())
		throw std::runtime_error("convert_equirect_to_cube: the image's payload does not match its layout.");
	const unsigned size = unsigned(scale * float(std::max(image.width / 3, image.height / 2)));
	if (size == 0)
		throw std::runtime_error("convert_equirect_to_cube: scale " + std::to_string(scale) + " of a " + std::to_string(image.width) + " x " +
		                         std::to_string(image.height) + " image gives an empty cube.");
	unsigned levels = 0; // info.levels = 0: the full chain
	for (unsigned s = size; s; s >>= 1)
		levels++;
	return bake(ctx, stream, image, size, levels, [&](void *in, void *out) {
		gr_image view = {};
		view.ptr = in; // level 0 is at the start of the payload
		view.width = image.width;
		view.height = image.height;
		view.pitch_bytes = image.width * 8u;
		view.format = uint32_t(image.format);
		return gr_env_equirect_to_cube(ctx, stream, &view, out, size, levels);
	});
}

GtxImage convert_cube_to_ibl_specular(gr_ctx *ctx, gr_stream stream, const GtxImage &cube)
{
	require_cube(cube, "convert_cube_to_ibl_specular");
	return bake(ctx, stream, cube, 128, 8, [&](void *in, void *out) {
		const gr_cube src = {in, cube.width, cube.levels};
		return gr_env_specular(ctx, stream, &src, out, 128, 8);
	});
}

GtxImage convert_cube_to_ibl_diffuse(gr_ctx *ctx, gr_stream stream, const GtxImage &cube)
{
	require_cube(cube, "convert_cube_to_ibl_diffuse");
	return bake(ctx, stream, cube, 32, 1, [&](void *in, void *out) {
		const gr_cube src = {in, cube.width, cube.levels};
		return gr_env_diffuse(ctx, stream, &src, out, 32);
	});
}
} // namespace Granite
