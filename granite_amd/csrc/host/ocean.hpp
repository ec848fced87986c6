// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Granite::Ocean (renderer/ocean.{hpp,cpp}) reduced to its per-frame compute pass `ocean-update-fft`: three animated spectra
// (gr_ocean_generate_fft), three inverse FFTs (Granite::FFT), the gradient / Jacobian and height / displacement maps
// (gr_ocean_bake_maps) and three mip chains (emit_single_pass_downsample for RGBA16F, gr_ocean_mipmap level by level otherwise).
// The LOD passes, the indirect buffers and all drawing are not built.
//
// The pass runs either inside a RenderGraph (add_fft_update_pass: the graph owns the nine resources) or directly
// (create_resources + update_fft_pass: the ocean owns resources of the same names, sizes and formats).  The three plans execute one
// after the other on the pass's stream, so a plan is in flight on one stream at a time.
#pragma once
#include <string>
#include "fft/fft.hpp"
#include "ocean_distribution.hpp"
#include "render_graph.hpp"

namespace Granite
{
class Ocean
{
public:
	static constexpr unsigned FrequencyBands = 8;
	static constexpr unsigned ResourceCount = 9;
	// The reference's resource names, in the order of gra_ocean_read's `which`.
	static const char *const ResourceNames[ResourceCount];

	// Throws std::invalid_argument for what derive_ocean_parameters refuses, before anything is allocated.  With
	// force_mipmap_shader every mip chain is built level by level with gr_ocean_mipmap, as on a device without the single-pass
	// downsampler.
	explicit Ocean(const OceanConfig &config, bool force_mipmap_shader = false);
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
	RenderBufferResource *graph_buffers[ResourceCount] = {};
	RenderTextureResource *graph_textures[ResourceCount] = {};
	HIP::BufferHandle own_buffers[ResourceCount];
	HIP::ImageHandle own_images[ResourceCount];

	void update_fft_input(HIP::CommandBuffer &cmd);
	void compute_fft(HIP::CommandBuffer &cmd);
	void bake_maps(HIP::CommandBuffer &cmd);
	void generate_mipmaps(HIP::CommandBuffer &cmd);
};
} // namespace Granite
