// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen; FidelityFX CACAO (c) 2016 Intel Corporation, modifications
// (c) 2021 Advanced Micro Devices, Inc.): see THIRD_PARTY_NOTICES.md at the repository root.
#include "ssao.hpp"
#include <memory>
#include <stdexcept>

namespace Granite
{
namespace
{
// CACAOState (ssao.cpp:35-43) and the body of the build callback (ssao.cpp:96-121)
struct CACAOState
{
	RenderGraph *graph = nullptr;
	const RenderContext *context = nullptr;
	RenderTextureResource *output = nullptr, *depth = nullptr, *normal = nullptr;
	gr_cacao_settings settings = {};
	// FFX_CACAO_GraniteScreenSizeInfo: the views the screen-size dependent resources were made for
	const HIP::Image *depth_view = nullptr, *normal_view = nullptr, *output_view = nullptr;
	uint32_t width = 0, height = 0;
	HIP::BufferHandle workspace;

	void record(HIP::CommandBuffer &cmd)
	{
		auto &depth_image = graph->get_physical_texture_resource(*depth);
		auto &normal_image = graph->get_physical_texture_resource(*normal);
		auto &output_image = graph->get_physical_texture_resource(*output);
		gr_ctx *ctx = cmd.get_context();
		if (&depth_image != depth_view || &normal_image != normal_view || &output_image != output_view || !workspace)
		{
			depth_view = &depth_image;
			normal_view = &normal_image;
			output_view = &output_image;
			width = depth_image.get_width();
			height = depth_image.get_height();
			const size_t bytes = gr_cacao_workspace_bytes(width, height);
			if (!bytes)
				throw std::logic_error("setup_ffx_cacao: the depth input has a size the SSAO pass does not take.");
			workspace.reset(); // FFX_CACAO_GraniteDestroyScreenSizeDependentResources, then ...InitScreenSizeDependentResources
			workspace = cmd.get_device().create_buffer(bytes, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, "ffx-cacao-workspace");
		}

		auto &rp = context->get_render_parameters();
		gr_cacao_buffer_sizes sizes;
		gr_cacao_constants constants[4];
		cmd.check(gr_cacao_update_buffer_sizes(width, height, &sizes), "cacao buffer sizes");
		cmd.check(gr_cacao_update_constants(ctx, constants, &settings, &sizes, rp.projection.data(), rp.view.data()), "cacao constants");

		// FFX_CACAO_GraniteDraw (ffx_cacao_impl.cpp:767-1026)
		void *ws = workspace->get_device_pointer();
		gr_stream stream = cmd.get_stream();
		cmd.check(gr_cacao_prepare_depths(ctx, stream, &depth_image.get_view(), ws, constants), "cacao prepare depths");
		cmd.check(gr_cacao_prepare_normals(ctx, stream, &normal_image.get_view(), ws, constants), "cacao prepare normals");
		if (settings.quality_level == GR_CACAO_QUALITY_HIGHEST)
		{
			cmd.check(gr_cacao_generate_base(ctx, stream, ws, width, height, constants), "cacao generate base");
			cmd.check(gr_cacao_importance_generate(ctx, stream, ws, width, height, constants), "cacao importance map");
			cmd.check(gr_cacao_importance_postprocess_a(ctx, stream, ws, width, height, constants), "cacao importance map A");
			cmd.check(gr_cacao_importance_postprocess_b(ctx, stream, ws, width, height, constants), "cacao importance map B");
		}
		cmd.check(gr_cacao_generate(ctx, stream, ws, width, height, constants, settings.quality_level), "cacao generate");
		if (settings.blur_pass_count)
			cmd.check(gr_cacao_blur(ctx, stream, ws, width, height, constants, settings.blur_pass_count), "cacao blur");
		cmd.check(gr_cacao_apply(ctx, stream, ws, &output_image.get_view(), constants, settings.blur_pass_count ? 1u : 0u), "cacao apply");
	}
};
} // namespace

void setup_ffx_cacao(RenderGraph &graph, const RenderContext &context, const std::string &output, const std::string &input_depth,
                     const std::string &input_normal, const gr_cacao_settings *settings, const std::string &pass_name)
{
	if (input_normal.empty())
		throw std::logic_error("setup_ffx_cacao: normals generated from depth are not built (generateNormals); name the G-buffer's normal attachment.");

	AttachmentInfo info;
	info.format = VK_FORMAT_R8_UNORM;
	info.size_class = SizeClass::InputRelative;
	info.size_relative_name = input_depth;
	info.size_x = 1.0f;
	info.size_y = 1.0f;

	auto state = std::make_shared<CACAOState>();
	state->graph = &graph;
	state->context = &context;
	if (settings)
		state->settings = *settings;
	else
		gr_cacao_reference_settings(&state->settings);

	auto &ffx = graph.add_pass(pass_name.empty() ? output : pass_name, RENDER_GRAPH_QUEUE_COMPUTE_BIT);
	state->output = &ffx.add_storage_texture_output(output, info);
	state->depth = &ffx.add_texture_input(input_depth);
	state->normal = &ffx.add_texture_input(input_normal);
	ffx.set_build_render_pass([state](HIP::CommandBuffer &cmd) { state->record(cmd); });
}
} // namespace Granite
