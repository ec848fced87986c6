// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "sky.hpp"
#include <cstring>

namespace Granite
{
void Skybox::set_image(HIP::BufferHandle chain, uint32_t size, uint32_t levels)
{
	cube = std::move(chain);
	cube_size = size;
	cube_levels = levels;
}

void Skybox::reset_image()
{
	cube.reset();
	cube_size = cube_levels = 0;
}

Skybox::RenderInfo Skybox::get_render_info(const RenderContext &context) const
{
	RenderInfo info;
	if (cube)
	{
		info.color = color;
		info.camera_height = 0.0f;
		info.direction = vec3(0.0f);
	}
	else
	{
		info.color = context.get_lighting_parameters()->directional.color;
		info.camera_height = context.get_render_parameters().camera_position.y;
		info.direction = context.get_lighting_parameters()->directional.direction;
	}
	return info;
}

void Skybox::render(HIP::CommandBuffer &cmd, const RenderContext &context, HIP::Image &emissive, HIP::Image &depth) const
{
	const RenderInfo info = get_render_info(context);
	gr_sky_args args = {};
	args.emissive = emissive.get_view();
	args.depth = depth.get_view();
	memcpy(args.inv_local_view_projection, context.get_render_parameters().inv_local_view_projection.data(), sizeof(args.inv_local_view_projection));
	for (int i = 0; i < 3; i++)
	{
		args.color[i] = info.color[i];
		args.sun_direction[i] = info.direction[i];
	}
	args.camera_height = info.camera_height;
	if (cube)
		args.cube = {cube->get_device_pointer(), cube_size, cube_levels};
	cmd.check(gr_sky_apply(cmd.get_context(), cmd.get_stream(), &args), "sky_apply");
}
} // namespace Granite
