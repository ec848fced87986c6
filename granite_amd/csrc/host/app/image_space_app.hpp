// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen; FidelityFX parts (c) 2021 Advanced Micro Devices, Inc.): see
// THIRD_PARTY_NOTICES.md at the repository root.
// ImageSpaceApplication — headless composition + frame loop of the image-space chain on the HIP executor.
// Graph composition follows SceneViewerApplication::bake_render_graph / add_main_pass_deferred
// (application/scene_viewer_application.cpp:876-991,1167-1318); the frame loop follows render_frame (:1540-1611) and the
// headless platform's external 4-image swapchain (application/platforms/application_headless.cpp:145-148,207-229).
#pragma once
#include <functional>
#include <memory>
#include <unordered_map>
#include <unordered_set>
#include <string>
#include <vector>
#include "../../../../include/granite_app.h"
#include "../collective.hpp"
#include "../lights/clusterer.hpp"
#include "../post/aa.hpp"
#include "../post/hdr.hpp"
#include "../render_context.hpp"
#include "../render_graph.hpp"
#include "../renderer.hpp"
#include "../sky.hpp"
#include "../video/scaler.hpp"
#include "../video/yuv_to_rgb.hpp"
#include "video_ring.hpp"

namespace Granite
{
class ImageSpaceApplication
{
public:
	explicit ImageSpaceApplication(const gra_config &config, const gra_config_ext &ext = {});
	~ImageSpaceApplication();

	void set_lights(const gra_light_desc *descs, uint32_t count);
	void set_decals(const gra_decal_desc *descs, uint32_t count);
	void set_sky_cube(uint32_t size, uint32_t levels, const void *rgba16f_chain, const float *color);
	const Skybox &get_skybox() const { return skybox; }
	void set_decal_texture(uint32_t index, uint32_t width, uint32_t height, uint32_t levels, uint32_t format, const void *texels);
	void upload_gbuffer(const void *emissive, const void *albedo, const void *normal, const void *pbr, const void *depth, const void *mv);
	void render_frame();
	void wait_idle()
	{
		if (device_holder)
			device_holder->wait_idle();
		if (video)
			video->ring.wait();
		if (playback)
			playback->ring.wait();
		check_taa_history_reach();
	}
	// Row bands with a bounded TAA history reach: throws once a resolve has reported a fetch outside the rows this rank holds.
	void check_taa_history_reach();
	// Composes and bakes the graph without touching a GPU (config.device < 0 creates no device): used by CPU tests.
	void bake_only() { bake_render_graph(); }

	HIP::Device &get_device()
	{
		if (!device_holder)
			throw std::logic_error("Application was created without a device (dry mode).");
		return *device_holder;
	}
	// DirectionalLightComponent of the scene (read_lights, scene_viewer_application.cpp:58-77); direction need not be normalised.
	void set_directional_light(const float direction[3], const float color[3]);
	void set_fog(const float color[3], float falloff);
	// gra_set_directional_shadows: nullptr or mode 0 switches shadows off
	void set_directional_shadows(const gra_directional_shadows *desc);
	// checkpoint / replay (include/granite_app.h: gra_write_resource, gra_frame_state)
	void prepare_resources_for_write();
	void get_frame_state(gra_frame_state &state) const;
	void set_frame_state(const gra_frame_state &state);
	RenderGraph &get_graph() { return graph; }
	RenderContext &get_context() { return context; }
	TemporalJitter &get_jitter() { return jitter; }
	HIP::Collective &get_collective() { return collective; }
	// Camera as the application sees it (un-jittered); with a temporal AA active each frame renders with
	// jitter.get_jittered_projection() like SceneViewerApplication::update_scene (scene_viewer_application.cpp:1431-1433).
	void set_base_camera(const mat4 &projection, const mat4 &view);
	mat4 get_taa_reprojection() const;
	LightClusterer &get_clusterer() { return cluster; }
	HIP::Image *get_last_backbuffer() { return last_backbuffer; }
	const gra_config &get_config() const { return config; }
	unsigned get_render_width() const { return render_width; }
	unsigned get_render_height() const { return render_height; }
	const StripPlan &get_strip_plan() const { return strip_plan; }
	void set_exchange_callback(gra_exchange_fn fn, void *user);
	void init_collective(const uint8_t *id128, int rank, int ranks);
	// Second communicator: the all-gather of the tonemapped bands moves to the device's collective stream and overlaps the
	// next frame ("overlap B with the next frame's lighting").
	void init_output_collective(const uint8_t *id128, int rank, int ranks);
	// Host-side cost of the frame loop: frames rendered, wall seconds inside render_frame(), of which blocked on the GPU.
	size_t get_allocated_bytes() const { return device_holder ? device_holder->get_allocated_bytes() : 0; }
	void get_host_stats(double out[3]) const
	{
		out[0] = double(host_frames);
		out[1] = host_seconds;
		out[2] = device_holder ? device_holder->get_blocked_seconds() : 0.0;
	}
	// The output gather beside the frame (init_output_collective): out[0] = times a pass was about to overwrite an output image, out[1] =
	// of those, how often the gather that last read the image was still in flight (the pass then waits: the gather was NOT hidden).
	void get_output_gather_stats(uint64_t out[2]) const
	{
		out[0] = output_acquires;
		out[1] = output_acquire_waits;
	}
	// G-buffer attachments from .gtx files (any may be null); the frame written back as .gtx.
	void upload_gbuffer_gtx(const char *const paths[6]);
	void set_camera_motion(const vec3 &translation_per_frame);
	void upload_ambient_occlusion(const void *ao_r8);
	void upload_aa_bench_images(const void *first, const void *second, uint32_t width, uint32_t height);
	void save_image_gtx(HIP::Image &image, const std::string &path);
	// Frame recording (include/granite_app.h: gra_video_*; video_recording.cpp)
	void video_begin(const gra_video_options &options);
	void video_end();
	const gra_video_layout &video_layout() const;
	bool video_read(void *dst, uint64_t size, int64_t *frame_number); // false: nothing pending
	// Frame playback (include/granite_app.h: gra_video_play_*; video_playback.cpp)
	void video_play_begin(const gra_video_play_options &options);
	void video_play_end();
	const gra_video_layout &video_play_layout() const;
	void video_play_frame(const void *frame, uint64_t size);
	bool video_play_read(void *dst, uint64_t size, int64_t *frame_number); // false: nothing pending
	std::string last_error;

private:
	gra_config config;
	gra_config_ext ext; // settings that came after gra_config's layout was fixed (gra_create_ext)
	unsigned render_width = 0, render_height = 0; // backbuffer size x resolution_scale
	bool scaled() const { return config.resolution_scale > 0.0f && config.resolution_scale < 1.0f; }
	VkFormat backbuffer_format() const { return config.hdr10 ? VK_FORMAT_A2B10G10R10_UNORM_PACK32 : VK_FORMAT_R8G8B8A8_SRGB; }
	std::unique_ptr<HIP::Device> device_holder;
	RenderGraph graph;
	RenderContext context;
	FrameParameters frame;
	LightingParameters lighting;
	LightClusterer cluster;
	TaskComposer composer;
	HDROptions hdr_options;
	StripPlan strip_plan;
	HIP::Collective collective, output_collective;
	// per output image: the event its last beside-the-frame gather records on the collective stream
	std::unordered_map<const void *, void *> output_gather_done;
	void *last_output_gather_event = nullptr; // hipEvent_t of the newest output gather (one of output_gather_done)
	// 24-bit transport form of the output bands (one buffer per output image, rank_count * chunk_rows rows of width * 3 bytes)
	std::unordered_map<const void *, HIP::BufferHandle> packed_output;
	using BandTransport = std::function<void(void *base, size_t chunk_bytes, void *stream)>;
	bool output_packs(const HIP::Image &image, const char *tag) const;
	void pack_output_band(HIP::CommandBuffer &cmd, HIP::Image &image, uint32_t chunk_rows);
	void gather_packed_output(HIP::Image &image, uint32_t chunk_rows, void *stream, const BandTransport &transport);
	void *output_ready_event = nullptr;
	uint32_t *taa_reach_flag = nullptr; // pinned host word the band resolve writes (strip_plan.taa_reach_flag)
	TemporalJitter jitter;
	mat4 base_projection, base_view;
	bool has_base_camera = false;

	// "Scene": light objects + node transforms, and the synthetic G-buffer sources.
	std::vector<std::unique_ptr<PositionalLight>> light_objects;
	std::vector<mat_affine> light_transforms;
	PositionalLightList light_list;
	// Volumetric decals (config.volumetric_decals): node transforms, the texture each one names, and the textures' mip chains.
	struct DecalTexture
	{
		HIP::BufferHandle levels;
		uint32_t width = 0, height = 0, num_levels = 0, format = 0;
	};
	std::vector<mat_affine> decal_transforms;
	std::vector<uint32_t> decal_texture_index;
	VolumetricDecalList decal_list;
	std::vector<DecalTexture> decal_textures;
	std::vector<gr_decal_texture> decal_table; // this frame's table, in the clusterer's sorted order
	void apply_volumetric_decals(HIP::CommandBuffer &cmd, HIP::Image &albedo, HIP::Image &depth);
	// The scene's background (ext.sky): the atmosphere lit by the directional light, or the cube of set_sky_cube.
	Skybox skybox;
	HIP::ImageHandle src_emissive, src_albedo, src_normal, src_pbr, src_depth, src_mv, src_ao;
	// the directional light's shadow map as the lighting pass reads it (lighting.shadows points at these), one image per layer
	HIP::ImageHandle shadow_layers[NumShadowCascades];
	// scene_viewer_application.cpp:881-883: renderTargetFp16 ? R16G16B16A16_SFLOAT : B10G11R11_UFLOAT_PACK32
	VkFormat hdr_target_format() const { return config.hdr_packed_float ? VK_FORMAT_B10G11R11_UFLOAT_PACK32 : VK_FORMAT_R16G16B16A16_SFLOAT; }
	vec3 camera_motion = vec3(0.0f); // eye translation per frame (world units)
	bool camera_moves = false;
	HIP::ImageHandle bench_images[2]; // aa_bench: the two input images, alternating per frame
	unsigned bench_input_index = 0;
	void add_aa_bench_main_pass(const std::string &tag);
	RenderTextureResource *ssao_output = nullptr;
	bool gbuffer_dirty = true;
	// Physical targets that already hold the current synthetic upload (an attachment the executor double-buffers has two).
	std::unordered_set<const void *> filled_targets;
	bool needs_fill(const HIP::Image &target) { return filled_targets.insert(target.get_device_pointer()).second; }
	bool is_filled(const HIP::Image &target) const { return filled_targets.count(target.get_device_pointer()) != 0; }

	std::vector<HIP::ImageHandle> swapchain;
	unsigned swapchain_index = 0;
	HIP::Image *last_backbuffer = nullptr;
	bool need_bake = true;
	bool resources_prepared = false; // prepare_resources_for_write() ran before the first frame
	double elapsed = 0.0;
	uint64_t host_frames = 0;
	uint64_t output_acquires = 0, output_acquire_waits = 0;
	double host_seconds = 0.0;

	// Recording state: one device copy of the planes (conversion and copy are in order on the ring's stream), a ring of pinned frames.
	struct VideoRecording
	{
		gra_video_options options = {};
		gra_video_layout layout = {};
		uint32_t plane_format[3] = {};
		void *planes = nullptr;        // device
		VideoScaler scaler;
		VideoRing ring;                // one buffer per slot: the packed frame
		// per swapchain image: hipEvent_t after the conversion that read it (the image's next writer waits for it)
		std::unordered_map<const void *, void *> read_done;
	};
	std::unique_ptr<VideoRecording> video;
	void video_check_ring() const;
	void video_before_frame(HIP::Image &backbuffer);
	void video_after_frame(HIP::Image &backbuffer, uint64_t device_frame);
	void video_release();
	// The packed-frame layout and the plane formats of a gra_video_format at w x h; false for an unknown format.
	static bool video_format_layout(uint32_t format, uint32_t w, uint32_t h, gra_video_layout &layout, uint32_t (&plane_format)[3]);

	// Playback state: one device copy of the planes and one of the RGB image (upload, conversion and read-back are in order on the
	// ring's stream), a ring of pinned frame / image pairs.
	struct VideoPlayback
	{
		gra_video_play_options options = {};
		gra_video_layout layout = {};
		uint32_t plane_format[3] = {};
		uint32_t rgb_pitch = 0;
		uint64_t rgb_bytes = 0;
		void *planes = nullptr;        // device
		void *rgb = nullptr;           // device
		VideoYuvToRgb converter;
		VideoRing ring;                // two buffers per slot: the packed frame as handed over, the converted image
	};
	std::unique_ptr<VideoPlayback> playback;
	void video_play_release();

	void bake_render_graph();
	void add_main_pass_deferred(const std::string &tag);
	void add_hdr_input_pass(const std::string &tag);
	void add_mv_pass(const std::string &tag);
};
} // namespace Granite
