// Stand-alone driver of granite_amd/csrc/host/ocean_distribution.cpp for tests/test_ocean_host_cpu.py: no device, no Python.
//   ocean_host dist fft_resolution displacement_downsample grid_count grid_resolution ocean_size wind_x wind_y heightmap
//       writes 8 floats (world sizes, wind direction, L, amplitude) and the height, displacement and normal distributions to stdout, raw
//   ocean_host draws count            the raw draws of the same engine and distribution, in the same order
//   ocean_host refusals               exit status 0 if every refused configuration throws std::invalid_argument and a good one does not
#include "../../granite_amd/csrc/host/ocean_distribution.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>

using namespace Granite;

static bool refuses(const OceanConfig &config)
{
	try
	{
		derive_ocean_parameters(config);
	}
	catch (const std::invalid_argument &)
	{
		return true;
	}
	return false;
}

static void put(const void *data, size_t bytes)
{
	if (fwrite(data, 1, bytes, stdout) != bytes)
		exit(3);
}

int main(int argc, char **argv)
{
	if (argc == 10 && !strcmp(argv[1], "dist"))
	{
		OceanConfig config;
		config.fft_resolution = unsigned(atoi(argv[2]));
		config.displacement_downsample = unsigned(atoi(argv[3]));
		config.grid_count = unsigned(atoi(argv[4]));
		config.grid_resolution = unsigned(atoi(argv[5]));
		config.ocean_size = vec2(float(atof(argv[6])));
		config.wind_velocity = vec2(float(atof(argv[7])), float(atof(argv[8])));
		config.heightmap = atoi(argv[9]) != 0;
		const OceanParameters p = derive_ocean_parameters(config);
		const vec2 world = p.heightmap_world_size(), normal = p.normalmap_world_size();
		const float header[8] = {world.x, world.y, normal.x, normal.y, p.wind_direction.x, p.wind_direction.y, p.phillips_L, p.config.amplitude};
		const OceanDistributions d = make_ocean_distributions(p);
		put(header, sizeof(header));
		put(d.height.data(), d.height.size() * sizeof(vec2));
		put(d.displacement.data(), d.displacement.size() * sizeof(vec2));
		put(d.normal.data(), d.normal.size() * sizeof(vec2));
		return 0;
	}
	if (argc == 3 && !strcmp(argv[1], "draws"))
	{
		std::normal_distribution<float> normal_dist(0.0f, 1.0f);
		std::default_random_engine engine;
		for (int i = 0, n = atoi(argv[2]); i < n; i++)
		{
			const float v = normal_dist(engine);
			put(&v, sizeof(v));
		}
		return 0;
	}
	if (argc == 2 && !strcmp(argv[1], "refusals"))
	{
		OceanConfig good;
		good.fft_resolution = 128;
		OceanConfig not_pot = good, small = good, no_count = good, no_resolution = good, no_wind = good, big_shift = good;
		not_pot.fft_resolution = 96;
		small.fft_resolution = 64; // >> 1 = 32
		no_count.grid_count = 0;
		no_resolution.grid_resolution = 0;
		no_wind.wind_velocity = vec2(0.0f);
		big_shift.displacement_downsample = 40;
		const bool ok = !refuses(good) && refuses(not_pot) && refuses(small) && refuses(no_count) && refuses(no_resolution) && refuses(no_wind) &&
		                refuses(big_shift);
		puts(ok ? "refusals: ok" : "refusals: WRONG");
		return ok ? 0 : 1;
	}
	fprintf(stderr, "usage: ocean_host dist ... | draws count | refusals\n");
	return 2;
}
