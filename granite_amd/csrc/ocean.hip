// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The compute work of Ocean::update_fft_pass (renderer/ocean.cpp) apart from the FFTs and the single-pass downsampler: the dispatches of
// ocean/generate_fft.comp, ocean/bake_maps.comp and ocean/mipmap.comp, one launch each.  The arithmetic is ocean_core.hpp's; this file
// adds the mapping of bins and texels to lanes and the argument checks.  Built with -ffp-contract=off (Makefile: EXACT_SRCS).
//
//   k_ocean_generate  one lane per bin, rows along x: a wave reads 64 consecutive float2 of its row and the 64 consecutive float2 of
//                     the mirrored row backwards -- whole 128-byte lines either way -- and stores 64 consecutive half2.
//   k_ocean_bake      one lane per texel of the height map, rows along x; the taps at texel centres snap to single texels.
//   k_ocean_mipmap    one lane per output texel, rows along x; four texels a tap.
#include "ctx.hpp"
#include "ocean_core.hpp"

namespace
{
using namespace gr_ocean;
constexpr uint32_t GROUP = 256u;

struct GenerateLaunch
{
	const float2 *distribution;
	uint32_t *out;
	uint32_t log2_nx;
	GenerateArgs g;
};

__global__ __launch_bounds__(GROUP) void k_ocean_generate(GenerateLaunch a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x;
	if (index >= a.g.nx * a.g.ny)
		return;
	const uint32_t x = index & (a.g.nx - 1u), y = index >> a.log2_nx;
	const uint32_t wx = (a.g.nx - x) & (a.g.nx - 1u), wy = (a.g.ny - y) & (a.g.ny - 1u);
	const float2 p = a.distribution[index], q = a.distribution[wy * a.g.nx + wx];
	a.out[index] = generate_bin(a.g, x, y, {p.x, p.y}, {q.x, q.y});
}

struct BakeLaunch
{
	BakeArgs b;
	uint8_t *grad_jacobian, *height_displacement; // RGBA16F; height_displacement may be null
	uint32_t grad_pitch, hd_pitch;
	uint32_t width, height;
};

__global__ __launch_bounds__(GROUP) void k_ocean_bake(BakeLaunch a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x;
	if (index >= a.width * a.height)
		return;
	const uint32_t y = index / a.width, x = index - y * a.width;
	uint2_bits hd, gj;
	bake_texel(a.b, x, y, hd, gj);
	*reinterpret_cast<uint2 *>(a.grad_jacobian + size_t(y) * a.grad_pitch + size_t(x) * 8u) = make_uint2(gj.x, gj.y);
	if (a.height_displacement)
		*reinterpret_cast<uint2 *>(a.height_displacement + size_t(y) * a.hd_pitch + size_t(x) * 8u) = make_uint2(hd.x, hd.y);
}

struct MipmapLaunch
{
	MipmapArgs m;
	uint8_t *out;
	uint32_t out_pitch;
};

template <int C> __global__ __launch_bounds__(GROUP) void k_ocean_mipmap(MipmapLaunch a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x;
	if (index >= a.m.count_x * a.m.count_y)
		return;
	const uint32_t y = index / a.m.count_x, x = index - y * a.m.count_x;
	uint16_t texel[C];
	mipmap_texel<C>(a.m, x, y, texel);
	uint8_t *at = a.out + size_t(y) * a.out_pitch + size_t(x) * (2u * C);
	if constexpr (C == 1)
		*reinterpret_cast<uint16_t *>(at) = texel[0];
	else if constexpr (C == 2)
		*reinterpret_cast<uint32_t *>(at) = uint32_t(texel[0]) | (uint32_t(texel[1]) << 16);
	else
		*reinterpret_cast<uint2 *>(at) = make_uint2(uint32_t(texel[0]) | (uint32_t(texel[1]) << 16), uint32_t(texel[2]) | (uint32_t(texel[3]) << 16));
}

bool power_of_two(uint32_t v) { return v != 0 && (v & (v - 1u)) == 0; }
uint32_t log2_of(uint32_t v)
{
	uint32_t l = 0;
	while (v >>= 1)
		l++;
	return l;
}
// What both image entry points ask of an image beyond the contract: texel indices stay below 2^31.
constexpr uint32_t MAX_EXTENT = 32768u;

Texture texture_of(const gr_image *img) { return {static_cast<const uint8_t *>(img->ptr), int(img->width), int(img->height), img->pitch_bytes}; }
} // namespace

extern "C" int gr_ocean_generate_fft(gr_ctx *ctx, gr_stream stream, const void *distribution, void *out, const gr_push_ocean_generate *push,
                                     uint32_t variant, const float *freq_bands)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, distribution);
	GR_CHECK_ARG(ctx, out);
	GR_CHECK_ARG(ctx, push);
	const uint32_t nx = push->N[0], ny = push->N[1];
	if (!power_of_two(nx) || !power_of_two(ny))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: N = %u x %u is not a power of two each way", nx, ny);
	if (nx < 64u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: N.x = %u is below 64 (the shader dispatches N.x / 64 groups a row)", nx);
	if (uint64_t(nx) * ny >= (1ull << 31))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: N = %u x %u has 2^31 bins or more", nx, ny);
	if (!(push->period > 0.0f))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: period %g is not positive", double(push->period));
	if (variant >= VARIANT_COUNT)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: unknown variant %u", variant);
	if ((reinterpret_cast<uintptr_t>(distribution) & 7u) || (reinterpret_cast<uintptr_t>(out) & 3u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: distribution is not 8-byte or out is not 4-byte aligned");
	if (gr_images_overlap(distribution, size_t(nx) * ny * 8u, out, size_t(nx) * ny * 4u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_generate_fft: out overlaps distribution");

	GenerateLaunch a = {};
	a.distribution = static_cast<const float2 *>(distribution);
	a.out = static_cast<uint32_t *>(out);
	a.log2_nx = log2_of(nx);
	a.g.mod_x = push->mod_factor[0];
	a.g.mod_y = push->mod_factor[1];
	a.g.nx = nx;
	a.g.ny = ny;
	a.g.freq_to_band_mod = push->freq_to_band_mod;
	a.g.time = push->time;
	a.g.period = push->period;
	a.g.variant = variant;
	a.g.use_bands = freq_bands ? 1u : 0u;
	if (freq_bands)
		memcpy(a.g.bands, freq_bands, sizeof(a.g.bands));
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_generate_fft"};
	hipLaunchKernelGGL(k_ocean_generate, dim3(gr_div_up(nx * ny, GROUP)), dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_ocean_bake_maps(gr_ctx *ctx, gr_stream stream, const gr_image *height, const gr_image *displacement, const gr_image *grad_jacobian,
                                  const gr_image *height_displacement, const gr_push_ocean_bake *push)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, push);
	GR_CHECK_IMAGE(ctx, height, GR_FORMAT_R16_SFLOAT);
	GR_CHECK_IMAGE(ctx, displacement, GR_FORMAT_R16G16_SFLOAT);
	GR_CHECK_IMAGE(ctx, grad_jacobian, GR_FORMAT_R16G16B16A16_SFLOAT);
	if (height_displacement)
		GR_CHECK_IMAGE(ctx, height_displacement, GR_FORMAT_R16G16B16A16_SFLOAT);
	GR_CHECK_ARG(ctx, height->width <= MAX_EXTENT && height->height <= MAX_EXTENT); // (the outputs have the height map's size, below)
	GR_CHECK_ARG(ctx, displacement->width <= MAX_EXTENT && displacement->height <= MAX_EXTENT);
	if (!power_of_two(displacement->width) || !power_of_two(displacement->height))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_bake_maps: displacement %u x %u is not a power of two each way", displacement->width, displacement->height);
	if (grad_jacobian->width != height->width || grad_jacobian->height != height->height ||
	    (height_displacement && (height_displacement->width != height->width || height_displacement->height != height->height)))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_bake_maps: the outputs do not have the height map's size %u x %u", height->width, height->height);
	for (const gr_image *o : {grad_jacobian, height_displacement})
		if (o && (gr_images_overlap(o, height) || gr_images_overlap(o, displacement) || (o == height_displacement && gr_images_overlap(o, grad_jacobian))))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_bake_maps: %s overlaps an input or the other output", o == grad_jacobian ? "grad_jacobian" : "height_displacement");

	BakeLaunch a = {};
	a.b.height = texture_of(height);
	a.b.displacement = texture_of(displacement);
	memcpy(a.b.inv_size, push->inv_size, sizeof(a.b.inv_size));
	memcpy(a.b.scale, push->scale, sizeof(a.b.scale));
	a.grad_jacobian = static_cast<uint8_t *>(grad_jacobian->ptr);
	a.grad_pitch = grad_jacobian->pitch_bytes;
	a.height_displacement = height_displacement ? static_cast<uint8_t *>(height_displacement->ptr) : nullptr;
	a.hd_pitch = height_displacement ? height_displacement->pitch_bytes : 0u;
	a.width = height->width;
	a.height = height->height;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_bake_maps"};
	hipLaunchKernelGGL(k_ocean_bake, dim3(gr_div_up(a.width * a.height, GROUP)), dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_ocean_mipmap(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, const gr_push_ocean_mipmap *push)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, push);
	constexpr gr_format_set half_floats{GR_FORMAT_R16_SFLOAT, GR_FORMAT_R16G16_SFLOAT, GR_FORMAT_R16G16B16A16_SFLOAT};
	GR_CHECK_IMAGE(ctx, in, half_floats);
	GR_CHECK_IMAGE(ctx, out, in->format);
	const uint32_t channels = gr_format_texel_bytes(in->format) / 2u;
	GR_CHECK_ARG(ctx, in->width <= MAX_EXTENT && in->height <= MAX_EXTENT);
	GR_CHECK_ARG(ctx, out->width <= MAX_EXTENT && out->height <= MAX_EXTENT);
	if (out->width != push->count[0] || out->height != push->count[1])
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_mipmap: out is %u x %u, count says %u x %u", out->width, out->height, push->count[0], push->count[1]);
	if (gr_images_overlap(in, out))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_ocean_mipmap: out overlaps in");

	MipmapLaunch a = {};
	a.m.in = texture_of(in);
	memcpy(a.m.result_mod, push->result_mod, sizeof(a.m.result_mod));
	memcpy(a.m.inv_resolution, push->inv_resolution, sizeof(a.m.inv_resolution));
	a.m.count_x = push->count[0];
	a.m.count_y = push->count[1];
	a.out = static_cast<uint8_t *>(out->ptr);
	a.out_pitch = out->pitch_bytes;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "ocean_mipmap"};
	const dim3 grid(gr_div_up(a.m.count_x * a.m.count_y, GROUP));
	if (channels == 1)
		hipLaunchKernelGGL(k_ocean_mipmap<1>, grid, dim3(GROUP), 0, s, a);
	else if (channels == 2)
		hipLaunchKernelGGL(k_ocean_mipmap<2>, grid, dim3(GROUP), 0, s, a);
	else
		hipLaunchKernelGGL(k_ocean_mipmap<4>, grid, dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
