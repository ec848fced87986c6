// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Skybox (renderer/mesh_util.{hpp,cpp}:1046-1142): the background every scene of the viewer has.  Without an image it is the
// procedural atmosphere lit by the directional light; with a cube it is that cube times a colour.  The reference queues a full-screen
// quad at z = 0 into the G-buffer pass; here render() runs gr_sky_apply on the emissive and depth the pass has just filled.
#pragma once
#include "hip_device.hpp"
#include "math.hpp"
#include "render_context.hpp"

namespace Granite
{
class Skybox
{
public:
	// An R16G16B16A16_SFLOAT cube chain in the gr_env_* layout (what gr_env_equirect_to_cube and gra_environment_bake produce), or none.
	void set_image(HIP::BufferHandle chain, uint32_t size, uint32_t levels);
	void reset_image();
	bool has_image() const { return bool(cube); }
	void set_color(const vec3 &color_) { color = color_; }

	// SkyboxRenderInfo's push values (mesh_util.cpp:1118-1129)
	struct RenderInfo
	{
		vec3 color;
		float camera_height;
		vec3 direction;
	};
	RenderInfo get_render_info(const RenderContext &context) const;

	void render(HIP::CommandBuffer &cmd, const RenderContext &context, HIP::Image &emissive, HIP::Image &depth) const;

private:
	HIP::BufferHandle cube;
	uint32_t cube_size = 0, cube_levels = 0;
	vec3 color = vec3(1.0f);
};
} // namespace Granite
