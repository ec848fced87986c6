// Stand-alone driver of granite_amd/csrc/host/ocean_lod.cpp (with ocean_distribution.cpp) for tests/test_ocean_lod_host_cpu.py: no device,
// no Python, so that it also runs under -fsanitize=address,undefined.
//   ocean_lod_host state fft_resolution grid_count grid_resolution ocean_size lod_bias heightmap fixed cx cy cz camx camy camz [24 plane floats]
//       stdout, raw: gr_push_ocean_update_lod, gr_push_ocean_cull, 24 plane floats, uint32 wrap, 16 counts, OceanData (64 bytes), uint32
//       lods, lod_stride, border_count, index_type; then per LOD mesh uint32 vertices, uint32 indices, the vertices, the indices; then the
//       border mesh the same way
//   ocean_lod_host refusals    exit status 0 if everything that must be refused throws std::invalid_argument and a good request does not
#include "../../granite_amd/csrc/host/ocean_lod.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>

using namespace Granite;

static void put(const void *data, size_t bytes)
{
	if (bytes && fwrite(data, 1, bytes, stdout) != bytes)
		exit(3);
}
static void put_u32(uint32_t v) { put(&v, 4); }

template <typename Fn> static bool refuses(Fn &&fn)
{
	try
	{
		fn();
	}
	catch (const std::invalid_argument &)
	{
		return true;
	}
	return false;
}

int main(int argc, char **argv)
{
	if ((argc == 15 || argc == 39) && !strcmp(argv[1], "state"))
	{
		OceanConfig config;
		config.fft_resolution = unsigned(atoi(argv[2]));
		config.grid_count = unsigned(atoi(argv[3]));
		config.grid_resolution = unsigned(atoi(argv[4]));
		config.ocean_size = vec2(float(atof(argv[5])));
		config.lod_bias = float(atof(argv[6]));
		config.heightmap = atoi(argv[7]) != 0;
		const bool fixed = atoi(argv[8]) != 0;
		const vec3 center(float(atof(argv[9])), float(atof(argv[10])), float(atof(argv[11])));
		const vec3 camera(float(atof(argv[12])), float(atof(argv[13])), float(atof(argv[14])));
		const OceanParameters parameters = derive_ocean_parameters(config);
		OceanLod lod(parameters.config, fixed, center);
		if (argc == 39)
		{
			vec4 planes[6];
			for (int i = 0; i < 24; i++)
				planes[i / 4][i % 4] = float(atof(argv[15 + i]));
			lod.set_camera(camera, planes);
		}
		const gr_push_ocean_update_lod up = lod.update_lod_push();
		const gr_push_ocean_cull cp = lod.cull_push();
		put(&up, sizeof(up));
		put(&cp, sizeof(cp));
		put(lod.get_frustum(), 24 * sizeof(float));
		put_u32(lod.get_wrap());
		uint32_t counts[16];
		lod.get_counts(counts);
		put(counts, sizeof(counts));
		const OceanDrawInfo info = lod.get_draw_info();
		put(&info.data, sizeof(info.data));
		put_u32(info.lods);
		put_u32(info.lod_stride);
		put_u32(info.border_count);
		put_u32(info.index_type);
		for (unsigned i = 0; i < lod.get_lod_count(); i++)
		{
			const OceanLodMesh &mesh = lod.get_lod_mesh(i);
			put_u32(uint32_t(mesh.vertices.size()));
			put_u32(uint32_t(mesh.indices.size()));
			put(mesh.vertices.data(), mesh.vertices.size() * sizeof(OceanVertex));
			put(mesh.indices.data(), mesh.indices.size() * sizeof(uint16_t));
		}
		const OceanBorderMesh &border = lod.get_border_mesh();
		put_u32(uint32_t(border.positions.size()));
		put_u32(uint32_t(border.indices.size()));
		put(border.positions.data(), border.positions.size() * sizeof(vec3));
		put(border.indices.data(), border.indices.size() * sizeof(uint16_t));
		return 0;
	}
	if (argc == 2 && !strcmp(argv[1], "refusals"))
	{
		OceanConfig good;
		good.fft_resolution = 128;
		good.grid_count = 16;
		good.grid_resolution = 32;
		good.ocean_size = vec2(256.0f);
		auto request = [](OceanConfig c) { return refuses([&]() { OceanLod::check_lod_update(c); }); };
		auto with = [&](unsigned count, unsigned resolution, bool heightmap) {
			OceanConfig c = good;
			c.grid_count = count;
			c.grid_resolution = resolution;
			c.heightmap = heightmap;
			return c;
		};
		bool ok = !request(good) && !request(with(4, 4, true)) && !request(with(128, 128, true));
		ok = ok && request(with(16, 32, false)) && request(with(2, 32, true)) && request(with(256, 32, true)) && request(with(24, 32, true)) &&
		     request(with(16, 2, true)) && request(with(16, 256, true)) && request(with(16, 48, true)) && request(with(0, 32, true));

		vec4 planes[6];
		for (auto &p : planes)
			p = vec4(0.0f, 1.0f, 0.0f, 1.0f);
		const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
		OceanLod moving(good, false, vec3(0.0f)), fixed(good, true, vec3(1.0f, 2.0f, 3.0f));
		ok = ok && !refuses([&]() { moving.set_camera(vec3(1.0f, 2.0f, 3.0f), planes); });
		ok = ok && refuses([&]() { moving.set_camera(vec3(nan, 2.0f, 3.0f), planes); }) && refuses([&]() { moving.set_camera(vec3(1.0f, inf, 3.0f), planes); });
		vec4 bad[6];
		memcpy(bad, planes, sizeof(bad));
		bad[4].w = nan;
		ok = ok && refuses([&]() { moving.set_camera(vec3(1.0f), bad); });
		// 16 units a block: 2^20 blocks are 16777216 units out
		ok = ok && !refuses([&]() { moving.set_camera(vec3(16.0f * 1048000.0f, 0.0f, -16.0f * 1048000.0f), planes); });
		ok = ok && refuses([&]() { moving.set_camera(vec3(16.0f * 1048577.0f, 0.0f, 0.0f), planes); }) &&
		     refuses([&]() { moving.set_camera(vec3(0.0f, 0.0f, -3.0e9f), planes); });
		ok = ok && !refuses([&]() { fixed.set_camera(vec3(3.0e9f, 0.0f, 0.0f), planes); }); // a fixed grid does not follow the camera
		// a refused camera leaves the state of the last good one
		moving.set_camera(vec3(40.0f, 2.0f, -40.0f), planes);
		const gr_push_ocean_update_lod before = moving.update_lod_push();
		ok = ok && refuses([&]() { moving.set_camera(vec3(nan), planes); });
		const gr_push_ocean_update_lod after = moving.update_lod_push();
		ok = ok && !memcmp(&before, &after, sizeof(before));
		puts(ok ? "refusals: ok" : "refusals: WRONG");
		return ok ? 0 : 1;
	}
	fprintf(stderr, "usage: ocean_lod_host state ... | refusals\n");
	return 2;
}
