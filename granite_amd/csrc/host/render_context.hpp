// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen; FidelityFX parts (c) 2021 Advanced Micro Devices, Inc.): see
// THIRD_PARTY_NOTICES.md at the repository root.
// FrameParameters / RenderParameters / RenderContext / LightingParameters — the slices of
// renderer/render_context.{hpp,cpp} and math/render_parameters.hpp:37-59,155-162 the image-space passes read.
#pragma once
#include "hip_device.hpp"
#include "math.hpp"

namespace Granite
{
class LightClusterer;

struct FrameParameters
{
	double frame_time = 0.0;
	double elapsed_time = 0.0;
	bool discontinuous_camera = false;
};

struct RenderParameters
{
	mat4 projection;
	mat4 view;
	mat4 view_projection;
	mat4 inv_projection;
	mat4 inv_view;
	mat4 inv_view_projection;
	mat4 unjittered_view_projection;
	mat4 unjittered_inv_view_projection;
	mat4 unjittered_prev_view_projection;
	// projection * (view with its translation zeroed) and its inverse: what skybox.vert turns a clip-space position into a direction with
	mat4 local_view_projection;
	mat4 inv_local_view_projection;
	vec3 camera_position;
	vec3 camera_front;
	vec3 camera_right;
	vec3 camera_up;
	float z_near = 0.0f;
	float z_far = 0.0f;
};

struct DirectionalParameters
{
	vec3 color = vec3(0.0f);
	vec3 direction = vec3(0.0f, 1.0f, 0.0f);
};

struct FogParameters
{
	vec3 color = vec3(0.0f);
	float falloff = 0.0f;
};

constexpr unsigned NumShadowCascades = 4;

// LightingParameters::shadow (renderer/lights/lights.hpp): world -> (u, v, z) of each cascade, and the bias of log2(view_z).
struct ShadowParameters
{
	mat4 transforms[NumShadowCascades];
	float cascade_log_bias = 0.0f;
};

// LightingParameters::shadows: the directional light's shadow map.  The reference binds one (array) image view and chooses the lookup by
// shader defines; here the view's layers, their count (1, or NumShadowCascades for SHADOW_CASCADES) and the lookup (GR_SHADOW_*; 0 = no
// shadows, which is render_light's unshadowed path).
struct DirectionalShadows
{
	const HIP::ImageView *layers[NumShadowCascades] = {};
	unsigned num_layers = 0;
	uint32_t mode = 0;
};

struct LightingParameters
{
	FogParameters fog;
	DirectionalParameters directional;
	ShadowParameters shadow;
	DirectionalShadows shadows;
	LightClusterer *cluster = nullptr;
	// LightingParameters::ambient_occlusion (renderer/lights/lights.hpp): the SSAO result the deferred lighting pass
	// samples, or null.  Set every frame from the graph's physical resource (scene_viewer_application.cpp:1571).
	const HIP::ImageView *ambient_occlusion = nullptr;
};

class RenderContext
{
public:
	// RenderContext::set_camera (render_context.cpp:53-86): inverses, camera basis, z_near / z_far from inv_projection.
	void set_camera(const mat4 &projection, const mat4 &view);
	// Harness hook: install precomputed parameters verbatim (keeps CPU oracle and device bit-identical inputs); the local view projection
	// is formed from their projection and view, as set_camera forms it.
	void set_render_parameters(const RenderParameters &params)
	{
		camera = params;
		set_local_view_projection();
	}
	const RenderParameters &get_render_parameters() const { return camera; }

	void set_frame_parameters(const FrameParameters &frame_) { frame = frame_; }
	const FrameParameters &get_frame_parameters() const { return frame; }

	void set_lighting_parameters(const LightingParameters *lighting_) { lighting = lighting_; }
	const LightingParameters *get_lighting_parameters() const { return lighting; }

private:
	// render_context.cpp:62-67
	void set_local_view_projection();
	RenderParameters camera;
	FrameParameters frame;
	const LightingParameters *lighting = nullptr;
};
} // namespace Granite
