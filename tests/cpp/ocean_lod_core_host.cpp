// TEST INFRASTRUCTURE.  The LOD update's per-lane arithmetic of granite_amd/csrc/ocean_core.hpp -- what the kernels of ocean.hip call --
// built for the host (g++ -ffp-contract=off) as a stand-alone program, so that it also runs under -fsanitize=address,undefined.
// tests/test_ocean_lod_core_cpu.py holds it to the golden of the executed shaders (tests/golden/ocean_lod_shader_v1.npz) before a device
// sees the code.
//
//   ocean_lod_core_host <case file>
// case file: int32 n, int32 wrap, the 64 bytes of gr_push_ocean_update_lod, the 96 of gr_push_ocean_cull, 24 floats of planes, 16 counts,
// then the n x n R16F LOD image the cull reads.  stdout: the LOD image update_lod_texel gives, the 8 draws after initialisation, the 8
// draws after the cull, and the lod_stride * 8 patches.  The append follows k_ocean_cull: 8 x 8 groups one after the other, and inside a
// group LOD by LOD, lanes in order.
#include "../../granite_amd/csrc/ocean_core.hpp"
#include "../../include/granite_hip.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace gr_ocean;

static void get(void *data, size_t bytes, FILE *f)
{
	if (fread(data, 1, bytes, f) != bytes)
	{
		fprintf(stderr, "ocean_lod_core_host: short case file\n");
		exit(3);
	}
}
static void put(const void *data, size_t bytes)
{
	if (bytes && fwrite(data, 1, bytes, stdout) != bytes)
		exit(3);
}

int main(int argc, char **argv)
{
	if (argc != 2)
	{
		fprintf(stderr, "usage: ocean_lod_core_host <case file>\n");
		return 2;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	int32_t n = 0, wrap = 0;
	gr_push_ocean_update_lod up;
	gr_push_ocean_cull cp;
	float planes[24];
	uint32_t counts[16];
	get(&n, 4, f);
	get(&wrap, 4, f);
	get(&up, sizeof(up), f);
	get(&cp, sizeof(cp), f);
	get(planes, sizeof(planes), f);
	get(counts, sizeof(counts), f);
	if (n < 4 || n > 128 || up.num_threads[0] != n || int32_t(cp.num_threads[0]) != n || cp.lod_stride < uint32_t(n * n))
		return 2;
	std::vector<uint16_t> golden_lods(size_t(n) * n);
	get(golden_lods.data(), golden_lods.size() * 2, f);
	fclose(f);

	UpdateLodArgs u = {};
	memcpy(u.camera, up.shifted_camera_pos, sizeof(u.camera));
	u.max_lod = up.max_lod;
	u.offset_x = up.image_offset[0];
	u.offset_y = up.image_offset[1];
	u.n = n;
	u.base_x = up.grid_base[0];
	u.base_y = up.grid_base[1];
	u.size_x = up.grid_size[0];
	u.size_y = up.grid_size[1];
	u.lod_bias = up.lod_bias;
	std::vector<uint16_t> lods(size_t(n) * n, 0xffffu);
	for (int y = 0; y < n; y++)
		for (int x = 0; x < n; x++)
		{
			int ix, iy;
			const uint16_t bits = update_lod_texel(u, x, y, ix, iy);
			lods.at(size_t(iy) * n + ix) = bits;
		}
	put(lods.data(), lods.size() * 2);

	uint32_t draws[MAX_LOD_INDIRECT][8] = {};
	for (uint32_t i = 0; i < MAX_LOD_INDIRECT; i++)
		draws[i][0] = counts[i];
	put(draws, sizeof(draws));

	CullArgs c = {};
	memcpy(c.world_offset, cp.world_offset, sizeof(c.world_offset));
	c.offset_x = cp.image_offset[0];
	c.offset_y = cp.image_offset[1];
	c.n = n;
	c.base_x = cp.grid_base[0];
	c.base_y = cp.grid_base[1];
	c.size_x = cp.grid_size[0];
	c.size_y = cp.grid_size[1];
	c.resolution_x = cp.grid_resolution[0];
	c.resolution_y = cp.grid_resolution[1];
	c.range_lo = cp.heightmap_range[0];
	c.range_hi = cp.heightmap_range[1];
	c.guard_band = cp.guard_band;
	c.lod_stride = cp.lod_stride;
	c.max_lod = cp.max_lod;
	c.handle_edge_lods = cp.handle_edge_lods != 0;
	c.wrap = wrap != 0;
	memcpy(c.frustum, planes, sizeof(planes));
	c.lods = {reinterpret_cast<const uint8_t *>(golden_lods.data()), n, n, uint32_t(n) * 2u};
	const uint32_t num_lods = uint32_t(cp.max_lod) + 1u;
	std::vector<Patch> patches(size_t(cp.lod_stride) * MAX_LOD_INDIRECT);
	for (int gy = 0; gy < (n + 7) / 8; gy++)
		for (int gx = 0; gx < (n + 7) / 8; gx++)
		{
			Patch patch[64];
			int lod[64];
			for (int lane = 0; lane < 64; lane++)
			{
				const int x = gx * 8 + (lane & 7), y = gy * 8 + lane / 8;
				lod[lane] = x < n && y < n && box_in_frustum(c, x, y) ? cull_patch(c, x, y, patch[lane]) : -1;
			}
			for (uint32_t l = 0; l < num_lods; l++)
				for (int lane = 0; lane < 64; lane++)
					if (lod[lane] == int(l))
						patches.at(size_t(cp.lod_stride) * l + draws[l][1]++) = patch[lane];
		}
	put(draws, sizeof(draws));
	put(patches.data(), patches.size() * sizeof(Patch));
	return 0;
}
