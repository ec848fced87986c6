// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Directional-light shadows: lights/directional.frag with SHADOWS (PCF, the wide PCF kernel, VSM; plain and cascaded), lights/resolve_vsm.frag
// and post/vsm_{down,up}_blur.frag as gfx950 kernels.  The per-lane arithmetic is shadow_core.hpp's; this file holds the launch shapes, the
// wave-uniform cascade loop and the launchers' refusals.  Built with -ffp-contract=off (Makefile: EXACT_SRCS).
//
// k_directional_light: one pixel per lane, 64 x 4 pixel tiles -- a workgroup of four waves, each wave one row of 64 pixels.  The kernel
// is a read-mostly stream over six attachments of 2 .. 8 bytes a pixel, and a wave-instruction is served at full rate when it covers
// contiguous bytes of one row (256 B of a 4-byte attachment here); a 16 x 16 tile would cut every such access into four 64-byte pieces
// of four rows.  Mode, the cascaded form and the depth format are template parameters: a PCF launch carries no VSM code.
// The cascade loop is the shader's: i runs from the wave's smallest layer_near to its largest layer_far, layer i's matrix and map
// descriptor are scalar loads from the kernel arguments, and a lane takes the lookup of the turns that are its own (shadow_core.hpp:
// cascade_turn).  Shadow-map taps are plain cached loads, clamped to the map; there is no LDS.
//
// k_vsm_moments, k_vsm_blur: one texel per lane, 64 x 4 tiles for the same reason.
#include "ctx.hpp"
#include "device_common.hpp"
#include "shadow_core.hpp"

namespace
{
using namespace gr_shadow;

constexpr unsigned TILE_W = 64, TILE_H = 4;

struct DirectionalArgs
{
	const uint8_t *albedo, *normal, *pbr, *depth, *emissive, *ambient_occlusion;
	uint8_t *hdr;
	const float *srgb_decode;
	uint32_t albedo_pitch, normal_pitch, pbr_pitch, depth_pitch, emissive_pitch, hdr_pitch, ao_pitch;
	uint32_t width, height, flags;
	int ao_width, ao_height;
	float inv_width, inv_height;
	float inv_vp[16], col2[4];
	float color[3], camera_pos[3], direction[3], camera_front[3];
	float cascade_log_bias;
	Maps maps;
	float transforms[NUM_CASCADES * 16];
};

template <int MODE, bool CASCADED, bool D16>
__global__ __launch_bounds__(TILE_W *TILE_H) void k_directional_light(const DirectionalArgs a)
{
	const uint32_t x = blockIdx.x * TILE_W + threadIdx.x, y = blockIdx.y * TILE_H + threadIdx.y;
	const bool inside = x < a.width && y < a.height;
	float depth = 0.0f;
	uint2 texel = make_uint2(0u, 0u);
	if (inside)
	{
		depth = *reinterpret_cast<const float *>(a.depth + (y * a.depth_pitch + x * 4u));
		texel = *reinterpret_cast<const uint2 *>(a.emissive + (y * a.emissive_pitch + x * 8u));
	}
	const bool active = inside && depth != 0.0f;
	// far-plane pixels are copied through; in place there is nothing to copy
	if (inside && !active && a.hdr != a.emissive)
		*reinterpret_cast<uint2 *>(a.hdr + (y * a.hdr_pitch + x * 8u)) = texel;
	if (__ballot(active) == 0ull)
		return;

	const f3 camera_pos = {a.camera_pos[0], a.camera_pos[1], a.camera_pos[2]};
	// an inactive lane keeps a finite position and takes no turn of the loop
	const f3 pos = active ? world_position(a.inv_vp, a.col2, a.inv_width, a.inv_height, x, y, depth) : f3{0.0f, 0.0f, 0.0f};
	float shadow_term = 1.0f;
	if (CASCADED)
	{
		Cascade c = compute_shadow_cascade(pos, camera_pos, {a.camera_front[0], a.camera_front[1], a.camera_front[2]}, a.cascade_log_bias);
		if (!active)
			c.layer_near = c.layer_far = -1;
		const int first = __builtin_amdgcn_readfirstlane(int(wave_min_u32(active ? uint32_t(c.layer_near) : uint32_t(NUM_CASCADES))));
		const int last = __builtin_amdgcn_readfirstlane(int(wave_max_u32(active ? uint32_t(c.layer_far) : 0u)));
		float term_near = 1.0f, term_far = 1.0f;
		for (int i = first; i <= last; i++) // 0 <= first, last <= NUM_CASCADES - 1: compute_shadow_cascade clamps both layers
			cascade_turn<MODE, D16>(a.maps, a.transforms, i, c, pos, term_near, term_far);
		shadow_term = blend_cascade(c, term_near, term_far);
	}
	else if (active)
		shadow_term = layer_term<MODE, D16>(a.maps.layer[0], a.maps.width, a.maps.height, light_clip(a.transforms, pos));
	if (!active)
		return;

	const uint32_t albedo = *reinterpret_cast<const uint32_t *>(a.albedo + (y * a.albedo_pitch + x * 4u));
	const uint32_t normal = *reinterpret_cast<const uint32_t *>(a.normal + (y * a.normal_pitch + x * 4u));
	const uint32_t pbr = *reinterpret_cast<const uint16_t *>(a.pbr + (y * a.pbr_pitch + x * 2u));
	const Material m = decode_material(albedo, normal, pbr, a.srgb_decode);
	f3 colour = compute_lighting(m, shadow_term, pos, camera_pos, {a.direction[0], a.direction[1], a.direction[2]}, {a.color[0], a.color[1], a.color[2]});
	if (a.flags & GR_LIGHTING_AMBIENT_FALLBACK_BIT)
	{
		float base_ambient = 1.0f;
		if (a.flags & GR_LIGHTING_AMBIENT_OCCLUSION_BIT)
			base_ambient = sample_ambient_occlusion(a.ambient_occlusion, a.ao_pitch, a.ao_width, a.ao_height, (float(x) + 0.5f) * a.inv_width, (float(y) + 0.5f) * a.inv_height);
		colour = add_ambient_fallback(colour, m.base, base_ambient);
	}
	// blend ONE / ONE: the attachment's store rounds the sum to fp16; alpha keeps its bits
	const uint32_t r = gr_core::float_to_half_pinned(gr_core::half_to_float(texel.x & 0xffffu) + colour.x);
	const uint32_t g = gr_core::float_to_half_pinned(gr_core::half_to_float(texel.x >> 16) + colour.y);
	const uint32_t b = gr_core::float_to_half_pinned(gr_core::half_to_float(texel.y & 0xffffu) + colour.z);
	*reinterpret_cast<uint2 *>(a.hdr + (y * a.hdr_pitch + x * 8u)) = make_uint2(r | (g << 16), b | (texel.y & 0xffff0000u));
}

struct PlaneArgs
{
	const uint8_t *in;
	uint8_t *out;
	uint32_t in_pitch, out_pitch;
	int in_width, in_height;
	uint32_t out_width, out_height;
	float spread;
};

template <bool D16> __global__ __launch_bounds__(TILE_W *TILE_H) void k_vsm_moments(const PlaneArgs a)
{
	const uint32_t x = blockIdx.x * TILE_W + threadIdx.x, y = blockIdx.y * TILE_H + threadIdx.y;
	if (x >= a.out_width || y >= a.out_height)
		return;
	const float z = depth_texel<D16>(Layer{a.in, a.in_pitch}, int(x), int(y));
	*reinterpret_cast<float2 *>(a.out + size_t(y) * a.out_pitch + size_t(x) * 8u) = make_float2(z, z * z);
}

__global__ __launch_bounds__(TILE_W *TILE_H) void k_vsm_blur(const PlaneArgs a)
{
	const uint32_t x = blockIdx.x * TILE_W + threadIdx.x, y = blockIdx.y * TILE_H + threadIdx.y;
	if (x >= a.out_width || y >= a.out_height)
		return;
	float mx, my;
	vsm_blur(Layer{a.in, a.in_pitch}, a.in_width, a.in_height, (float(x) + 0.5f) / float(a.out_width), (float(y) + 0.5f) / float(a.out_height), a.spread, mx, my);
	*reinterpret_cast<float2 *>(a.out + size_t(y) * a.out_pitch + size_t(x) * 8u) = make_float2(mx, my);
}

template <int MODE, bool CASCADED, bool D16> void launch_directional(const dim3 grid, hipStream_t stream, const DirectionalArgs &a)
{
	hipLaunchKernelGGL((k_directional_light<MODE, CASCADED, D16>), grid, dim3(TILE_W, TILE_H), 0, stream, a);
}
} // namespace

extern "C" {

int gr_directional_light(gr_ctx *ctx, gr_stream stream, const gr_directional_light_args *args)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, args != nullptr);
	if (args->hdr.format == GR_FORMAT_B10G11R11_UFLOAT_PACK32)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: hdr is a B10G11R11_UFLOAT_PACK32 target: the shadowed directional light is built for "
		                                          "R16G16B16A16_SFLOAT targets only", __func__);
	GR_CHECK_IMAGE(ctx, &args->hdr, GR_FORMAT_R16G16B16A16_SFLOAT);
	const uint32_t W = args->hdr.width, H = args->hdr.height;
	GR_CHECK_IMAGE(ctx, &args->emissive, GR_FORMAT_R16G16B16A16_SFLOAT, W, H);
	GR_CHECK_IMAGE(ctx, &args->albedo, GR_FORMAT_R8G8B8A8_SRGB, W, H);
	GR_CHECK_IMAGE(ctx, &args->normal, GR_FORMAT_A2B10G10R10_UNORM_PACK32, W, H);
	GR_CHECK_IMAGE(ctx, &args->pbr, GR_FORMAT_R8G8_UNORM, W, H);
	GR_CHECK_IMAGE(ctx, &args->depth, GR_FORMAT_D32_SFLOAT, W, H);
	if (args->flags & ~(GR_LIGHTING_AMBIENT_FALLBACK_BIT | GR_LIGHTING_AMBIENT_OCCLUSION_BIT))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: flags 0x%x has a bit other than the ambient fallback and ambient occlusion bits", __func__, args->flags);
	const bool ao = (args->flags & GR_LIGHTING_AMBIENT_OCCLUSION_BIT) != 0;
	if (ao)
	{
		GR_CHECK_ARG(ctx, (args->flags & GR_LIGHTING_AMBIENT_FALLBACK_BIT) != 0);
		GR_CHECK_IMAGE(ctx, &args->ambient_occlusion, GR_FORMAT_R8_UNORM);
	}
	if (args->mode != GR_SHADOW_PCF && args->mode != GR_SHADOW_PCF_WIDE && args->mode != GR_SHADOW_VSM)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: mode %u is not GR_SHADOW_PCF, GR_SHADOW_PCF_WIDE or GR_SHADOW_VSM", __func__, args->mode);
	if (args->layers != 1u && args->layers != uint32_t(GR_SHADOW_NUM_CASCADES))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: layers %u is not 1 or %d", __func__, args->layers, GR_SHADOW_NUM_CASCADES);
	const gr_format_set map_formats = args->mode == GR_SHADOW_VSM ? gr_format_set(GR_FORMAT_R32G32_SFLOAT) : gr_format_set(GR_FORMAT_D16_UNORM, GR_FORMAT_D32_SFLOAT);
	for (uint32_t i = 0; i < args->layers; i++)
	{
		// every layer has the first one's format and size
		const gr_image *map = &args->shadow_maps[i];
		const char *rule = i == 0 ? gr_image_rule(map, map_formats) : gr_image_rule(map, args->shadow_maps[0].format, args->shadow_maps[0].width, args->shadow_maps[0].height);
		if (!rule && (map->width > GR_SHADOW_MAX_EXTENT || map->height > GR_SHADOW_MAX_EXTENT))
			rule = " is wider or higher than 16384 texels";
		if (rule)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: shadow_maps[%u]%s", __func__, i, rule);
	}
	// 32-bit byte offsets inside the kernel for each of the six frame attachments at its own pitch
	GR_CHECK_IMAGE_OFFSETS(ctx, &args->hdr);
	GR_CHECK_IMAGE_OFFSETS(ctx, &args->emissive);
	GR_CHECK_IMAGE_OFFSETS(ctx, &args->albedo);
	GR_CHECK_IMAGE_OFFSETS(ctx, &args->normal);
	GR_CHECK_IMAGE_OFFSETS(ctx, &args->pbr);
	GR_CHECK_IMAGE_OFFSETS(ctx, &args->depth);
	// lanes read texels that other lanes of the launch write when the output shares bytes with an input
	if (args->hdr.ptr != args->emissive.ptr && gr_images_overlap(&args->hdr, &args->emissive))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: hdr shares bytes with emissive other than by an equal pointer", __func__);
	const struct { const gr_image *image; const char *name; } inputs[] = {{&args->albedo, "albedo"}, {&args->normal, "normal"}, {&args->pbr, "pbr"}, {&args->depth, "depth"}};
	for (const auto &input : inputs)
		if (gr_images_overlap(&args->hdr, input.image))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: hdr shares bytes with %s", __func__, input.name);
	if (ao && gr_images_overlap(&args->hdr, &args->ambient_occlusion))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: hdr shares bytes with ambient_occlusion", __func__);
	for (uint32_t i = 0; i < args->layers; i++)
		if (gr_images_overlap(&args->hdr, &args->shadow_maps[i]))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: hdr shares bytes with shadow_maps[%u]", __func__, i);

	DirectionalArgs a = {};
	a.albedo = static_cast<const uint8_t *>(args->albedo.ptr), a.albedo_pitch = args->albedo.pitch_bytes;
	a.normal = static_cast<const uint8_t *>(args->normal.ptr), a.normal_pitch = args->normal.pitch_bytes;
	a.pbr = static_cast<const uint8_t *>(args->pbr.ptr), a.pbr_pitch = args->pbr.pitch_bytes;
	a.depth = static_cast<const uint8_t *>(args->depth.ptr), a.depth_pitch = args->depth.pitch_bytes;
	a.emissive = static_cast<const uint8_t *>(args->emissive.ptr), a.emissive_pitch = args->emissive.pitch_bytes;
	a.hdr = static_cast<uint8_t *>(args->hdr.ptr), a.hdr_pitch = args->hdr.pitch_bytes;
	if (ao)
	{
		a.ambient_occlusion = static_cast<const uint8_t *>(args->ambient_occlusion.ptr), a.ao_pitch = args->ambient_occlusion.pitch_bytes;
		a.ao_width = int(args->ambient_occlusion.width), a.ao_height = int(args->ambient_occlusion.height);
	}
	a.srgb_decode = ctx->srgb_decode_lut;
	a.width = W, a.height = H, a.flags = args->flags;
	a.inv_width = args->directional.inv_resolution[0], a.inv_height = args->directional.inv_resolution[1];
	memcpy(a.inv_vp, args->inv_view_projection, sizeof(a.inv_vp));
	memcpy(a.col2, args->directional.inv_view_proj_col2, sizeof(a.col2));
	memcpy(a.color, args->directional.color, sizeof(a.color));
	memcpy(a.camera_pos, args->directional.camera_pos, sizeof(a.camera_pos));
	memcpy(a.direction, args->directional.direction, sizeof(a.direction));
	memcpy(a.camera_front, args->directional.camera_front, sizeof(a.camera_front));
	a.cascade_log_bias = args->directional.cascade_log_bias;
	a.maps.width = int(args->shadow_maps[0].width), a.maps.height = int(args->shadow_maps[0].height);
	for (uint32_t i = 0; i < uint32_t(NUM_CASCADES); i++)
	{
		// the plain variant reads layer 0 alone; its other descriptors repeat it, so that no descriptor is left dangling
		const gr_image &map = args->shadow_maps[i < args->layers ? i : 0u];
		a.maps.layer[i] = {static_cast<const uint8_t *>(map.ptr), map.pitch_bytes};
	}
	memcpy(a.transforms, args->transforms, sizeof(a.transforms));

	const dim3 grid(gr_div_up(W, TILE_W), gr_div_up(H, TILE_H));
	const bool cascaded = args->layers != 1u, d16 = args->shadow_maps[0].format == GR_FORMAT_D16_UNORM;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "directional_light"};
	if (args->mode == GR_SHADOW_VSM)
		with_flags([&](auto c) { launch_directional<MODE_VSM, decltype(c)::value, false>(grid, s, a); }, cascaded);
	else if (args->mode == GR_SHADOW_PCF_WIDE)
		with_flags([&](auto c, auto d) { launch_directional<MODE_PCF_WIDE, decltype(c)::value, decltype(d)::value>(grid, s, a); }, cascaded, d16);
	else
		with_flags([&](auto c, auto d) { launch_directional<MODE_PCF, decltype(c)::value, decltype(d)::value>(grid, s, a); }, cascaded, d16);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

int gr_vsm_moments(gr_ctx *ctx, gr_stream stream, const gr_image *depth, const gr_image *moments)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_IMAGE(ctx, depth, gr_format_set(GR_FORMAT_D16_UNORM, GR_FORMAT_D32_SFLOAT));
	GR_CHECK_IMAGE(ctx, moments, GR_FORMAT_R32G32_SFLOAT, depth->width, depth->height);
	if (gr_images_overlap(depth, moments))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: moments shares bytes with depth", __func__);
	PlaneArgs a = {};
	a.in = static_cast<const uint8_t *>(depth->ptr), a.in_pitch = depth->pitch_bytes;
	a.out = static_cast<uint8_t *>(moments->ptr), a.out_pitch = moments->pitch_bytes;
	a.in_width = int(depth->width), a.in_height = int(depth->height);
	a.out_width = moments->width, a.out_height = moments->height;
	const dim3 grid(gr_div_up(a.out_width, TILE_W), gr_div_up(a.out_height, TILE_H));
	gr_scoped_timing timing{ctx, gr_to_stream(stream), "vsm_moments"};
	if (depth->format == GR_FORMAT_D16_UNORM)
		hipLaunchKernelGGL(k_vsm_moments<true>, grid, dim3(TILE_W, TILE_H), 0, gr_to_stream(stream), a);
	else
		hipLaunchKernelGGL(k_vsm_moments<false>, grid, dim3(TILE_W, TILE_H), 0, gr_to_stream(stream), a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

int gr_vsm_blur(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, int up)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_IMAGE(ctx, in, GR_FORMAT_R32G32_SFLOAT);
	GR_CHECK_IMAGE(ctx, out, GR_FORMAT_R32G32_SFLOAT);
	if (in->width > GR_SHADOW_MAX_EXTENT || in->height > GR_SHADOW_MAX_EXTENT)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: in is wider or higher than 16384 texels", __func__);
	if (gr_images_overlap(in, out))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: out shares bytes with in", __func__);
	PlaneArgs a = {};
	a.in = static_cast<const uint8_t *>(in->ptr), a.in_pitch = in->pitch_bytes;
	a.out = static_cast<uint8_t *>(out->ptr), a.out_pitch = out->pitch_bytes;
	a.in_width = int(in->width), a.in_height = int(in->height);
	a.out_width = out->width, a.out_height = out->height;
	a.spread = up ? 0.875f : 1.75f;
	const dim3 grid(gr_div_up(a.out_width, TILE_W), gr_div_up(a.out_height, TILE_H));
	gr_scoped_timing timing{ctx, gr_to_stream(stream), up ? "vsm_up_blur" : "vsm_down_blur"};
	hipLaunchKernelGGL(k_vsm_blur, grid, dim3(TILE_W, TILE_H), 0, gr_to_stream(stream), a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
}
