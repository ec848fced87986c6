// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The host-only part of Granite::Ocean (renderer/ocean.{hpp,cpp}): its configuration, what the constructor derives from it, and the
// Phillips distributions the FFT update animates.  Nothing here touches the device, so tests/cpp/ocean_host.cpp links this unit alone.
#pragma once
#include <vector>
#include "math.hpp"

namespace Granite
{
// ocean.hpp:40-75, fields and defaults.
struct OceanConfig
{
	unsigned fft_resolution = 1024;       // heightmap and normal map FFT size
	unsigned displacement_downsample = 1; // the displacement FFT is fft_resolution >> this
	unsigned grid_count = 64;
	unsigned grid_resolution = 128;
	vec2 ocean_size = vec2(1024.0f);
	vec2 wind_velocity = vec2(4.0f, 2.0f);
	float normal_mod = 7.3f;
	float amplitude = 0.2f;
	bool heightmap = true;
	float lod_bias = -3.5f;
};

// What Ocean's constructor makes of a configuration (ocean.cpp:45-68), after refusing with std::invalid_argument: an fft_resolution
// that is no power of two, fft_resolution >> displacement_downsample below 64 (the spectrum dispatch would have no group), a zero
// grid_count or grid_resolution, a zero wind velocity.
struct OceanParameters
{
	OceanConfig config; // amplitude normalised by sqrt(base_freq.x * base_freq.y); the grid recomposed when there is no heightmap
	vec2 wind_direction;
	float phillips_L = 0.0f;
	vec2 heightmap_world_size() const;
	vec2 normalmap_world_size() const;
	// Levels of the height / displacement chain: the reference's quad_lod.size(), one LOD per halving of grid_resolution down to 2
	// (build_buffers), cut to the image's own chain as setup_render_pass_resources does.  0 without a heightmap.
	unsigned vertex_levels() const;
};
OceanParameters derive_ocean_parameters(const OceanConfig &config);

// generate_distribution (ocean.cpp:1460-1480): Nx * Nz complex numbers, rows outermost, x drawn before y from
// std::normal_distribution<float>(0, 1) on a default-constructed std::default_random_engine that is fresh in every call.
void generate_distribution(vec2 *output, const vec2 &mod, unsigned Nx, unsigned Nz, float amplitude, float max_l, const vec2 &wind_dir, float L);
// downsample_distribution: bin i of the small spectrum is bin alias(i) of the large one, a negative frequency counted from its end.
void downsample_distribution(vec2 *output, const vec2 *input, unsigned Nx, unsigned Nz, unsigned rate_log2);

struct OceanDistributions
{
	std::vector<vec2> height, displacement, normal;
};
// init_distributions without the upload: the normal map has its own mod and amplitude * normal_mod.
OceanDistributions make_ocean_distributions(const OceanParameters &parameters);
} // namespace Granite
