// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "ocean_distribution.hpp"
#include <algorithm>
#include <random>
#include <stdexcept>

namespace Granite
{
namespace
{
constexpr float G = 9.81f;
constexpr float TwoPi = 6.28318530717958647692f;

int alias(int x, int N) { return x > N / 2 ? x - N : x; }

unsigned floor_log2(unsigned v)
{
	unsigned l = 0;
	while (v >>= 1)
		l++;
	return l;
}

float phillips(float kx, float ky, float max_l, const vec2 &wind_dir, float L)
{
	const float k_len = std::sqrt(kx * kx + ky * ky);
	if (k_len == 0.0f)
		return 0.0f;
	const float kL = k_len * L;
	const float kw = (kx / k_len) * wind_dir.x + (ky / k_len) * wind_dir.y;
	return (kw * kw) * std::exp(-1.0f * k_len * k_len * max_l * max_l) * std::exp(-1.0f / (kL * kL)) * std::pow(k_len, -4.0f);
}
} // namespace

vec2 OceanParameters::heightmap_world_size() const
{
	const float scale = float(config.fft_resolution) / float(config.grid_resolution);
	return {config.ocean_size.x / float(config.grid_count) * scale, config.ocean_size.y / float(config.grid_count) * scale};
}

vec2 OceanParameters::normalmap_world_size() const
{
	const vec2 size = heightmap_world_size();
	return {size.x / config.normal_mod, size.y / config.normal_mod};
}

unsigned OceanParameters::vertex_levels() const
{
	if (!config.heightmap)
		return 0;
	return std::min(floor_log2(config.grid_resolution), floor_log2(config.fft_resolution) + 1u);
}

OceanParameters derive_ocean_parameters(const OceanConfig &config)
{
	const unsigned n = config.fft_resolution;
	if (n == 0 || (n & (n - 1u)) != 0)
		throw std::invalid_argument("Ocean: fft_resolution is not a power of two.");
	if (config.displacement_downsample >= 32 || (n >> config.displacement_downsample) < 64)
		throw std::invalid_argument("Ocean: fft_resolution >> displacement_downsample is below 64.");
	if (config.grid_count == 0 || config.grid_resolution == 0)
		throw std::invalid_argument("Ocean: grid_count and grid_resolution must not be zero.");
	const float wind2 = config.wind_velocity.x * config.wind_velocity.x + config.wind_velocity.y * config.wind_velocity.y;
	if (!(wind2 > 0.0f))
		throw std::invalid_argument("Ocean: the wind velocity is zero.");

	OceanParameters p;
	p.config = config;
	const float wind_len = std::sqrt(wind2);
	p.wind_direction = {config.wind_velocity.x / wind_len, config.wind_velocity.y / wind_len};
	p.phillips_L = wind2 / G;
	// Noise: energy is integrated, not amplitude, so the amplitude follows the density of the frequency grid.
	const vec2 world = p.heightmap_world_size();
	p.config.amplitude *= std::sqrt((1.0f / world.x) * (1.0f / world.y));
	if (!p.config.heightmap)
	{
		while (p.config.grid_count > 8 && p.config.grid_count % 2 == 0)
		{
			p.config.grid_count /= 2;
			p.config.grid_resolution *= 2;
		}
	}
	return p;
}

void generate_distribution(vec2 *output, const vec2 &mod, unsigned Nx, unsigned Nz, float amplitude, float max_l, const vec2 &wind_dir, float L)
{
	std::normal_distribution<float> normal_dist(0.0f, 1.0f);
	std::default_random_engine engine;
	for (unsigned z = 0; z < Nz; z++)
	{
		for (unsigned x = 0; x < Nx; x++)
		{
			const float kx = mod.x * float(alias(int(x), int(Nx))), ky = mod.y * float(alias(int(z), int(Nz)));
			const float dx = normal_dist(engine);
			const float dy = normal_dist(engine);
			const float root = std::sqrt(0.5f * phillips(kx, ky, max_l, wind_dir, L));
			output[size_t(z) * Nx + x] = {dx * amplitude * root, dy * amplitude * root};
		}
	}
}

void downsample_distribution(vec2 *output, const vec2 *input, unsigned Nx, unsigned Nz, unsigned rate_log2)
{
	const unsigned out_width = Nx >> rate_log2, out_height = Nz >> rate_log2;
	for (unsigned z = 0; z < out_height; z++)
	{
		for (unsigned x = 0; x < out_width; x++)
		{
			int ax = alias(int(x), int(out_width)), az = alias(int(z), int(out_height));
			if (ax < 0)
				ax += int(Nx);
			if (az < 0)
				az += int(Nz);
			output[size_t(z) * out_width + x] = input[size_t(az) * Nx + unsigned(ax)];
		}
	}
}

OceanDistributions make_ocean_distributions(const OceanParameters &p)
{
	const unsigned n = p.config.fft_resolution, m = n >> p.config.displacement_downsample;
	OceanDistributions d;
	d.height.resize(size_t(n) * n);
	d.displacement.resize(size_t(m) * m);
	d.normal.resize(size_t(n) * n);
	const vec2 world = p.heightmap_world_size(), normal_world = p.normalmap_world_size();
	generate_distribution(d.height.data(), {TwoPi / world.x, TwoPi / world.y}, n, n, p.config.amplitude, 0.02f, p.wind_direction, p.phillips_L);
	generate_distribution(d.normal.data(), {TwoPi / normal_world.x, TwoPi / normal_world.y}, n, n, p.config.amplitude * p.config.normal_mod, 0.02f,
	                      p.wind_direction, p.phillips_L);
	downsample_distribution(d.displacement.data(), d.height.data(), n, n, p.config.displacement_downsample);
	return d;
}
} // namespace Granite
