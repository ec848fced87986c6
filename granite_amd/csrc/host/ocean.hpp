// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Granite::Ocean (renderer/ocean.{hpp,cpp}) reduced to its compute side and its static geometry.
//   `ocean-update-fft`: three animated spectra (gr_ocean_generate_fft), three inverse FFTs (Granite::FFT), the gradient / Jacobian and
//   height / displacement maps (gr_ocean_bake_maps) and three mip chains (emit_single_pass_downsample for RGBA16F, gr_ocean_mipmap level
//   by level otherwise).
//   `ocean-update-lods`, when the ocean was created with a LOD request: the LOD map (gr_ocean_update_lod), the eight indirect draws
//   (gr_ocean_init_counter_buffer) and the culled, bucketed patches (gr_ocean_cull_blocks), three launches on the pass's stream.
//   The LOD and border meshes of build_buffers and the uniform block of get_render_info_heightmap (host/ocean_lod.hpp).
// All of its drawing is not built: a rasteriser binds ocean-lod-counter as its indirect buffer, ocean-lod-data as its
// per-instance storage, the meshes and the maps.
//
// The passes run either inside a RenderGraph (add_lod_update_pass, add_fft_update_pass: the graph owns the resources) or directly
// (create_resources + update_lod_pass, update_fft_pass: the ocean owns resources of the same names, sizes and formats).  The three plans
// execute one after the other on the pass's stream, so a plan is in flight on one stream at a time.  An ocean without a LOD request
// runs and allocates what it did before the LOD update existed.
#pragma once
#include <string>
#include "fft/fft.hpp"
#include "ocean_distribution.hpp"
#include "ocean_lod.hpp"
#include "render_graph.hpp"

namespace Granite
{
// What the reference decides by config.heightmap and by having a scene node; here it is asked for.
struct OceanLodRequest
{
	bool lod_update = false;     // add the `ocean-update-lods` pass and its three resources, upload the meshes
	bool fixed_position = false; // the reference's `node`: the grid stays around center_position
	vec3 center_position;
};

class Ocean
{
public:
	static constexpr unsigned FrequencyBands = 8;
	static constexpr unsigned ResourceCount = 9;    // of the FFT update
	static constexpr unsigned LodResourceCount = 3; // ocean-lods, ocean-lod-counter, ocean-lod-data: ids 9, 10, 11
	static constexpr unsigned TotalResourceCount = ResourceCount + LodResourceCount;
	// The reference's resource names, in the order of gra_ocean_read's `which`.
	static const char *const ResourceNames[TotalResourceCount];

	// Throws std::invalid_argument for what derive_ocean_parameters refuses, before anything is allocated.  With
	// force_mipmap_shader every mip chain is built level by level with gr_ocean_mipmap, as on a device without the single-pass
	// downsampler.
	// A LOD request is refused the same way for what OceanLod::check_lod_update refuses.
	explicit Ocean(const OceanConfig &config, bool force_mipmap_shader = false, const OceanLodRequest &lod_request = {});
	~Ocean();
	Ocean(const Ocean &) = delete;
	void operator=(const Ocean &) = delete;

	const OceanConfig &get_config() const { return parameters.config; }
	vec2 heightmap_world_size() const { return parameters.heightmap_world_size(); }
	vec2 normalmap_world_size() const { return parameters.normalmap_world_size(); }
	vec2 get_wind_direction() const { return parameters.wind_direction; }
	float get_phillips_L() const { return parameters.phillips_L; }
	void set_frequency_band_amplitude(unsigned band, float amplitude);
	void set_frequency_band_modulation(bool enable) { freq_band_modulation = enable; }
	// Stands in for context->get_frame_parameters().elapsed_time.
	void set_elapsed_time(double seconds) { elapsed_time = seconds; }

	// on_pipeline_created: plans the three FFTs and uploads the distributions (once).
	void on_device_created(HIP::Device &device);
	void init_distributions(HIP::Device &device);
	const OceanDistributions &get_distributions() const { return distributions; }

	void add_fft_update_pass(RenderGraph &graph);
	void create_resources(HIP::Device &device);
	void update_fft_pass(HIP::CommandBuffer &cmd);

	// The LOD update.  set_camera stands in for refresh() and the context's visibility frustum; until it is called the camera is at
	// the origin and every block is in view.
	bool has_lod_update() const { return lod_request.lod_update; }
	void set_camera(const vec3 &position, const vec4 planes[6]) { lod.set_camera(position, planes); }
	void add_lod_update_pass(RenderGraph &graph);
	void update_lod_pass(HIP::CommandBuffer &cmd);
	const OceanLod &get_lod() const { return lod; }
	// The meshes on the device (made once in on_device_created, with a LOD request only); nullptr if there is none.
	HIP::Buffer *get_lod_vbo(unsigned index) { return index < lod_vbos.size() ? lod_vbos[index].get() : nullptr; }
	HIP::Buffer *get_lod_ibo(unsigned index) { return index < lod_ibos.size() ? lod_ibos[index].get() : nullptr; }
	HIP::Buffer *get_border_vbo() { return border_vbo.get(); }
	HIP::Buffer *get_border_ibo() { return border_ibo.get(); }

	// For reading back: the buffer or image behind a resource name on the route in use; nullptr if it does not exist
	// (ocean-height-displacement-output without a heightmap).
	HIP::Buffer *get_buffer(unsigned which);
	HIP::Image *get_image(unsigned which);
	// Levels of the mip chain that update_fft_pass fills (1 for the FFT outputs without a chain).
	unsigned get_levels(unsigned which);

private:
	OceanParameters parameters;
	OceanDistributions distributions;
	bool force_mipmap_shader;
	bool freq_band_modulation = false;
	float frequency_bands[FrequencyBands];
	double elapsed_time = 0.0;

	HIP::Device *device = nullptr;
	FFT height_fft, normal_fft, displacement_fft;
	HIP::BufferHandle distribution_buffer, distribution_buffer_displacement, distribution_buffer_normal;

	RenderGraph *graph = nullptr;
	RenderBufferResource *graph_buffers[TotalResourceCount] = {};
	RenderTextureResource *graph_textures[TotalResourceCount] = {};
	HIP::BufferHandle own_buffers[TotalResourceCount];
	HIP::ImageHandle own_images[TotalResourceCount];

	OceanLodRequest lod_request;
	OceanLod lod;
	std::vector<HIP::BufferHandle> lod_vbos, lod_ibos;
	HIP::BufferHandle border_vbo, border_ibo;

	void update_fft_input(HIP::CommandBuffer &cmd);
	void compute_fft(HIP::CommandBuffer &cmd);
	void bake_maps(HIP::CommandBuffer &cmd);
	void generate_mipmaps(HIP::CommandBuffer &cmd);

	void build_buffers(HIP::Device &device);
	void build_lod_map(HIP::CommandBuffer &cmd);
	void init_counter_buffer(HIP::CommandBuffer &cmd);
	void cull_blocks(HIP::CommandBuffer &cmd);
};
} // namespace Granite
