// Follows MIT-licensed work (FidelityFX CACAO, (c) 2016 Intel Corporation, modifications (c) 2021 Advanced Micro Devices, Inc.; Granite
// integration (c) 2022-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The dispatches of FFX_CACAO_GraniteDraw (renderer/post/ffx-cacao/src/ffx_cacao_impl.cpp:767-1026) for the configuration
// setup_ffx_cacao runs and its non-adaptive sibling, one entry point a shader.  The arithmetic and the kernels are cacao_core.hpp's; this
// file adds the argument checks, the host-only queries and the launches.  Built with -ffp-contract=off (Makefile: EXACT_SRCS).
//
//   k_cacao_prepare_depths           one lane per half-resolution texel, 8 x 8 groups: a 2 x 2 gather, four R16F layers, mips 1-3 via LDS
//   k_cacao_prepare_normals          one lane per half-resolution texel: four RGBA8_SNORM layers
//   k_cacao_generate<level, base>    one lane per half-resolution texel, the pass in blockIdx.z: up to 64 depth taps
//   k_cacao_importance_*             one lane per quarter-resolution texel
//   k_cacao_blur                     16 x 16 lanes of 4 x 3 texels, the pass in blockIdx.z
//   k_cacao_apply                    one lane per output texel
#include <algorithm>
#include "ctx.hpp"
#include "cacao_core.hpp"

namespace
{
using namespace gr_cacao;

bool extent_ok(uint32_t width, uint32_t height) { return width && height && width <= GR_CACAO_MAX_EXTENT && height <= GR_CACAO_MAX_EXTENT; }

// What every launcher asks of (workspace, width, height, constants); the rule broken, or nullptr.
const char *common_rule(const void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *c)
{
	if (!workspace)
		return "workspace is a null pointer";
	if (!c)
		return "constants is a null pointer";
	if (reinterpret_cast<uintptr_t>(workspace) % WORKSPACE_ALIGN)
		return "workspace is not 256-byte aligned";
	if (!extent_ok(width, height))
		return "width or height is 0 or above GR_CACAO_MAX_EXTENT";
	gr_cacao_buffer_sizes b;
	update_buffer_sizes(width, height, b);
	if (c->InputOutputBufferDimensions[0] != float(width) || c->InputOutputBufferDimensions[1] != float(height) || c->DepthBufferDimensions[0] != float(width) ||
	    c->DepthBufferDimensions[1] != float(height) || c->SSAOBufferDimensions[0] != float(b.ssaoBufferWidth) || c->SSAOBufferDimensions[1] != float(b.ssaoBufferHeight) ||
	    c->DeinterleavedDepthBufferDimensions[0] != float(b.deinterleavedDepthBufferWidth) ||
	    c->DeinterleavedDepthBufferDimensions[1] != float(b.deinterleavedDepthBufferHeight) || c->ImportanceMapDimensions[0] != float(b.importanceMapWidth) ||
	    c->ImportanceMapDimensions[1] != float(b.importanceMapHeight))
		return "constants were not made for this width and height (gr_cacao_update_constants)";
	return nullptr;
}
#define CACAO_CHECK_COMMON(ctx, workspace, width, height, c)                                  \
	do                                                                                        \
	{                                                                                         \
		if (const char *rule__ = common_rule(workspace, width, height, c))                    \
			return (ctx)->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: %s", __func__, rule__); \
	} while (0)

// A wrong format alone is GR_ERR_UNSUPPORTED_FORMAT; everything else about an image is image_args.hpp's.
#define CACAO_CHECK_IMAGE(ctx, img, format_)                                                                                             \
	do                                                                                                                                   \
	{                                                                                                                                    \
		if ((img) && (img)->ptr && (img)->format != uint32_t(format_))                                                                   \
			return (ctx)->fail(GR_ERR_UNSUPPORTED_FORMAT, "%s: unsupported format: %s has format %u, this argument takes " #format_, __func__, #img, (img)->format); \
		GR_CHECK_IMAGE(ctx, img, format_);                                                                                               \
	} while (0)

dim3 grid_for(uint32_t w, uint32_t h, uint32_t depth = 1) { return dim3(gr_div_up(w, GROUP), gr_div_up(h, GROUP), depth); }

int launch_importance(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *c, int which, const char *name)
{
	const Workspace ws = workspace_layout(width, height);
	ImportanceLaunch a = {};
	a.c = *c;
	a.im = images_of(workspace, ws);
	uint8_t *base = static_cast<uint8_t *>(workspace);
	a.out = base + ws.importance[which == 1 ? 1 : 0];
	a.load_counter = reinterpret_cast<uint32_t *>(base + ws.load_counter);
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, name};
	const dim3 grid = grid_for(ws.imp_w, ws.imp_h), block(GROUP, GROUP);
	const dim3 groups(grid.x * grid.y), walked(std::min(groups.x, IMPORTANCE_MAX_GROUPS)); // k_cacao_importance_postprocess walks the groups
	if (which == 0)
		hipLaunchKernelGGL(k_cacao_importance_generate, grid, block, 0, s, a);
	else if (which == 1)
		hipLaunchKernelGGL(k_cacao_importance_postprocess<false>, groups, block, 0, s, a);
	else
		hipLaunchKernelGGL(k_cacao_importance_postprocess<true>, walked, block, 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

GenerateLaunch generate_launch(void *workspace, const Workspace &ws, const gr_cacao_constants constants[4], uint32_t target)
{
	GenerateLaunch a = {};
	a.c = constants[0];
	a.pp = per_pass_of(constants);
	a.im = images_of(workspace, ws);
	for (uint32_t p = 0; p < PASSES; p++)
		a.out[p] = static_cast<uint8_t *>(workspace) + ws.ssao[target] + uint64_t(p) * ws.half_w * ws.half_h * 2u;
	return a;
}
} // namespace

extern "C" void gr_cacao_reference_settings(gr_cacao_settings *settings)
{
	if (settings)
		reference_settings(*settings);
}

extern "C" int gr_cacao_update_buffer_sizes(uint32_t width, uint32_t height, gr_cacao_buffer_sizes *sizes)
{
	if (!sizes || !extent_ok(width, height))
		return GR_ERR_INVALID_ARGUMENT;
	update_buffer_sizes(width, height, *sizes);
	return GR_OK;
}

extern "C" int gr_cacao_update_constants(gr_ctx *ctx, gr_cacao_constants constants[4], const gr_cacao_settings *settings, const gr_cacao_buffer_sizes *sizes,
                                         const float proj[16], const float normals_to_view[16])
{
	const auto refuse = [ctx](const char *rule) { return ctx ? ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_cacao_update_constants: invalid argument: %s", rule) : int(GR_ERR_INVALID_ARGUMENT); };
	if (!constants || !settings || !sizes || !proj || !normals_to_view)
		return refuse("a null pointer");
	if (settings->generate_normals)
		return refuse("generate_normals is set: normals come from the G-buffer");
	if (settings->quality_level != GR_CACAO_QUALITY_HIGH && settings->quality_level != GR_CACAO_QUALITY_HIGHEST)
		return refuse("quality_level is neither GR_CACAO_QUALITY_HIGH nor GR_CACAO_QUALITY_HIGHEST");
	if (settings->blur_pass_count > GR_CACAO_MAX_BLUR_PASSES)
		return refuse("blur_pass_count is above 8");
	gr_cacao_buffer_sizes expected;
	if (!extent_ok(sizes->inputOutputBufferWidth, sizes->inputOutputBufferHeight))
		return refuse("sizes: width or height is 0 or above GR_CACAO_MAX_EXTENT");
	update_buffer_sizes(sizes->inputOutputBufferWidth, sizes->inputOutputBufferHeight, expected);
	if (memcmp(&expected, sizes, sizeof(expected)))
		return refuse("sizes are not those of gr_cacao_update_buffer_sizes (native resolution only)");
	for (int pass = 0; pass < 4; pass++)
	{
		constants[pass] = {};
		update_constants(constants[pass], *settings, *sizes, proj, normals_to_view);
		update_per_pass_constants(constants[pass], *sizes, pass);
	}
	return GR_OK;
}

extern "C" size_t gr_cacao_workspace_bytes(uint32_t width, uint32_t height) { return extent_ok(width, height) ? size_t(workspace_layout(width, height).bytes) : 0; }

extern "C" int gr_cacao_workspace_describe(uint32_t width, uint32_t height, gr_cacao_intermediate *out, uint32_t capacity)
{
	if (!out || capacity < GR_CACAO_INTERMEDIATE_COUNT || !extent_ok(width, height))
		return GR_ERR_INVALID_ARGUMENT;
	const Workspace ws = workspace_layout(width, height);
	const auto fill = [](gr_cacao_intermediate &d, const char *name, uint32_t format, uint32_t w, uint32_t h, uint32_t layers, uint64_t offset, uint32_t texel) {
		d = {};
		snprintf(d.name, sizeof(d.name), "%s", name);
		d.format = format;
		d.width = w;
		d.height = h;
		d.layers = layers;
		d.mips = 1;
		d.mip_offset[0] = offset;
		d.bytes = uint64_t(w) * h * texel * layers;
	};
	fill(out[0], "FFX_CACAO_DEINTERLEAVED_DEPTHS", GR_FORMAT_R16_SFLOAT, ws.half_w, ws.half_h, PASSES, ws.depth_mip[0], 2);
	out[0].mips = DEPTH_MIPS;
	out[0].bytes = 0;
	for (uint32_t k = 0; k < DEPTH_MIPS; k++)
	{
		out[0].mip_offset[k] = ws.depth_mip[k];
		out[0].bytes += uint64_t(mip_extent(ws.half_w, k)) * mip_extent(ws.half_h, k) * 2u * PASSES;
	}
	fill(out[1], "FFX_CACAO_DEINTERLEAVED_NORMALS", GR_CACAO_FORMAT_R8G8B8A8_SNORM, ws.half_w, ws.half_h, PASSES, ws.normals, 4);
	fill(out[2], "FFX_CACAO_SSAO_BUFFER_PING", GR_FORMAT_R8G8_UNORM, ws.half_w, ws.half_h, PASSES, ws.ssao[0], 2);
	fill(out[3], "FFX_CACAO_SSAO_BUFFER_PONG", GR_FORMAT_R8G8_UNORM, ws.half_w, ws.half_h, PASSES, ws.ssao[1], 2);
	fill(out[4], "FFX_CACAO_IMPORTANCE_MAP", GR_FORMAT_R8_UNORM, ws.imp_w, ws.imp_h, 1, ws.importance[0], 1);
	fill(out[5], "FFX_CACAO_IMPORTANCE_MAP_PONG", GR_FORMAT_R8_UNORM, ws.imp_w, ws.imp_h, 1, ws.importance[1], 1);
	fill(out[6], "FFX_CACAO_LOAD_COUNTER", GR_CACAO_FORMAT_R32_UINT, 1, 1, 1, ws.load_counter, 4);
	return GR_OK;
}

extern "C" int gr_cacao_prepare_depths(gr_ctx *ctx, gr_stream stream, const gr_image *depth, void *workspace, const gr_cacao_constants *constants)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_IMAGE(ctx, depth, GR_FORMAT_D32_SFLOAT);
	CACAO_CHECK_COMMON(ctx, workspace, depth->width, depth->height, constants);
	const Workspace ws = workspace_layout(depth->width, depth->height);
	if (gr_images_overlap(depth->ptr, size_t(depth->pitch_bytes) * depth->height, workspace, size_t(ws.bytes)))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_cacao_prepare_depths: invalid argument: workspace overlaps depth");
	PrepareDepthsLaunch a = {};
	a.c = *constants;
	a.depth = static_cast<const uint8_t *>(depth->ptr);
	a.depth_pitch = depth->pitch_bytes;
	a.width = int(depth->width);
	a.height = int(depth->height);
	a.workspace = static_cast<uint8_t *>(workspace);
	a.ws = ws;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "cacao_prepare_depths"};
	hipLaunchKernelGGL(k_cacao_prepare_depths, grid_for(ws.half_w, ws.half_h), dim3(GROUP, GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_cacao_prepare_normals(gr_ctx *ctx, gr_stream stream, const gr_image *normal, void *workspace, const gr_cacao_constants *constants)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_IMAGE(ctx, normal, GR_FORMAT_A2B10G10R10_UNORM_PACK32);
	CACAO_CHECK_COMMON(ctx, workspace, normal->width, normal->height, constants);
	const Workspace ws = workspace_layout(normal->width, normal->height);
	if (gr_images_overlap(normal->ptr, size_t(normal->pitch_bytes) * normal->height, workspace, size_t(ws.bytes)))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_cacao_prepare_normals: invalid argument: workspace overlaps normal");
	PrepareNormalsLaunch a = {};
	a.c = *constants;
	a.normal = static_cast<const uint8_t *>(normal->ptr);
	a.normal_pitch = normal->pitch_bytes;
	a.width = int(normal->width);
	a.height = int(normal->height);
	a.workspace = static_cast<uint8_t *>(workspace);
	a.ws = ws;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "cacao_prepare_normals"};
	hipLaunchKernelGGL(k_cacao_prepare_normals, grid_for(ws.half_w, ws.half_h), dim3(GROUP, GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_cacao_generate_base(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants constants[4])
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_COMMON(ctx, workspace, width, height, constants);
	const Workspace ws = workspace_layout(width, height);
	const GenerateLaunch a = generate_launch(workspace, ws, constants, 1);
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "cacao_generate_base"};
	hipLaunchKernelGGL((k_cacao_generate<3, true>), grid_for(ws.half_w, ws.half_h, PASSES), dim3(GROUP, GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_cacao_importance_generate(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_COMMON(ctx, workspace, width, height, constants);
	return launch_importance(ctx, stream, workspace, width, height, constants, 0, "cacao_importance_generate");
}

extern "C" int gr_cacao_importance_postprocess_a(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_COMMON(ctx, workspace, width, height, constants);
	return launch_importance(ctx, stream, workspace, width, height, constants, 1, "cacao_importance_postprocess_a");
}

extern "C" int gr_cacao_importance_postprocess_b(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_COMMON(ctx, workspace, width, height, constants);
	return launch_importance(ctx, stream, workspace, width, height, constants, 2, "cacao_importance_postprocess_b");
}

extern "C" int gr_cacao_generate(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants constants[4], uint32_t quality)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_COMMON(ctx, workspace, width, height, constants);
	if (quality != GR_CACAO_QUALITY_HIGH && quality != GR_CACAO_QUALITY_HIGHEST)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_cacao_generate: invalid argument: quality %u is neither GR_CACAO_QUALITY_HIGH nor GR_CACAO_QUALITY_HIGHEST", quality);
	const Workspace ws = workspace_layout(width, height);
	const GenerateLaunch a = generate_launch(workspace, ws, constants, 0);
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, quality == GR_CACAO_QUALITY_HIGHEST ? "cacao_generate_q3" : "cacao_generate_q2"};
	const dim3 grid = grid_for(ws.half_w, ws.half_h, PASSES), block(GROUP, GROUP);
	if (quality == GR_CACAO_QUALITY_HIGHEST)
		hipLaunchKernelGGL((k_cacao_generate<3, false>), grid, block, 0, s, a);
	else
		hipLaunchKernelGGL((k_cacao_generate<2, false>), grid, block, 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_cacao_blur(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants, uint32_t blur_passes)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_COMMON(ctx, workspace, width, height, constants);
	if (blur_passes < 1 || blur_passes > GR_CACAO_MAX_BLUR_PASSES)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_cacao_blur: invalid argument: blur_passes %u is not 1 .. 8", blur_passes);
	const Workspace ws = workspace_layout(width, height);
	BlurLaunch a = {};
	a.c = *constants;
	for (uint32_t p = 0; p < PASSES; p++)
	{
		a.in[p] = static_cast<const uint8_t *>(workspace) + ws.ssao[0] + uint64_t(p) * ws.half_w * ws.half_h * 2u;
		a.out[p] = static_cast<uint8_t *>(workspace) + ws.ssao[1] + uint64_t(p) * ws.half_w * ws.half_h * 2u;
	}
	a.half_w = int(ws.half_w);
	a.half_h = int(ws.half_h);
	a.blur_passes = blur_passes;
	// ffx_cacao_impl.cpp:945-948: a group covers 4 * 16 - 2 N by 3 * 16 - 2 N texels
	const uint32_t tile_w = uint32_t(BLUR_TILE_W) * BLUR_GROUP - 2u * blur_passes, tile_h = uint32_t(BLUR_TILE_H) * BLUR_GROUP - 2u * blur_passes;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "cacao_blur"};
	hipLaunchKernelGGL(k_cacao_blur, dim3(gr_div_up(ws.half_w, tile_w), gr_div_up(ws.half_h, tile_h), PASSES), dim3(BLUR_GROUP, BLUR_GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_cacao_apply(gr_ctx *ctx, gr_stream stream, const void *workspace, const gr_image *out, const gr_cacao_constants *constants, uint32_t from_pong)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	CACAO_CHECK_IMAGE(ctx, out, GR_FORMAT_R8_UNORM);
	CACAO_CHECK_COMMON(ctx, workspace, out->width, out->height, constants);
	const Workspace ws = workspace_layout(out->width, out->height);
	if (gr_images_overlap(out->ptr, size_t(out->pitch_bytes) * out->height, workspace, size_t(ws.bytes)))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_cacao_apply: invalid argument: out overlaps workspace");
	ApplyLaunch a = {};
	a.c = *constants;
	a.im = images_of(workspace, ws);
	a.out = static_cast<uint8_t *>(out->ptr);
	a.out_pitch = out->pitch_bytes;
	a.width = int(out->width);
	a.height = int(out->height);
	a.from_pong = from_pong ? 1u : 0u;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "cacao_apply"};
	hipLaunchKernelGGL(k_cacao_apply, grid_for(out->width, out->height), dim3(GROUP, GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
