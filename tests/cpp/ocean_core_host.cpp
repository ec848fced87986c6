// TEST INFRASTRUCTURE.  granite_amd/csrc/ocean_core.hpp -- the per-lane arithmetic the kernels of ocean.hip call -- built for the host as
// a shared library (g++ -ffp-contract=off).  Every bin and texel is computed as the kernels compute it, one lane after the other.
// tests/test_ocean_core_cpu.py holds it to the golden of the executed shaders (tests/golden/ocean_shader_v1.npz) before a device sees
// the code.
#include "../../granite_amd/csrc/ocean_core.hpp"

using namespace gr_ocean;

// push: the 7 dwords of gr_push_ocean_generate; bands: 8 floats or null
extern "C" void ocean_host_generate(const float *distribution, uint32_t *out, const void *push, uint32_t variant, const float *bands)
{
	GenerateArgs g = {};
	const float *pf = static_cast<const float *>(push);
	const uint32_t *pu = static_cast<const uint32_t *>(push);
	g.mod_x = pf[0];
	g.mod_y = pf[1];
	g.nx = pu[2];
	g.ny = pu[3];
	g.freq_to_band_mod = pf[4];
	g.time = pf[5];
	g.period = pf[6];
	g.variant = variant;
	g.use_bands = bands ? 1u : 0u;
	if (bands)
		memcpy(g.bands, bands, sizeof(g.bands));
	for (uint32_t y = 0; y < g.ny; y++)
		for (uint32_t x = 0; x < g.nx; x++)
		{
			const uint32_t wx = (g.nx - x) & (g.nx - 1u), wy = (g.ny - y) & (g.ny - 1u);
			const float *a = distribution + 2 * (size_t(y) * g.nx + x), *b = distribution + 2 * (size_t(wy) * g.nx + wx);
			out[size_t(y) * g.nx + x] = generate_bin(g, x, y, {a[0], a[1]}, {b[0], b[1]});
		}
}

// Tightly packed images.  push: inv_size[4], scale[4].  height_displacement may be null.
extern "C" void ocean_host_bake(const uint16_t *height, int w, int h, const uint16_t *displacement, int dw, int dh, const float *push,
                                uint32_t *grad_jacobian, uint32_t *height_displacement)
{
	BakeArgs a = {};
	a.height = {reinterpret_cast<const uint8_t *>(height), w, h, uint32_t(w) * 2u};
	a.displacement = {reinterpret_cast<const uint8_t *>(displacement), dw, dh, uint32_t(dw) * 4u};
	memcpy(a.inv_size, push, 16);
	memcpy(a.scale, push + 4, 16);
	for (int y = 0; y < h; y++)
		for (int x = 0; x < w; x++)
		{
			uint2_bits hd, gj;
			bake_texel(a, uint32_t(x), uint32_t(y), hd, gj);
			const size_t at = 2 * (size_t(y) * w + x);
			grad_jacobian[at] = gj.x;
			grad_jacobian[at + 1] = gj.y;
			if (height_displacement)
			{
				height_displacement[at] = hd.x;
				height_displacement[at + 1] = hd.y;
			}
		}
}

// push: result_mod[4], inv_resolution[2], count[2], lod.  channels 1, 2 or 4; returns -1 for anything else.
extern "C" int ocean_host_mipmap(const uint16_t *in, int w, int h, int channels, const void *push, uint16_t *out)
{
	MipmapArgs a = {};
	a.in = {reinterpret_cast<const uint8_t *>(in), w, h, uint32_t(w) * 2u * uint32_t(channels)};
	memcpy(a.result_mod, push, 16);
	memcpy(a.inv_resolution, static_cast<const uint8_t *>(push) + 16, 8);
	memcpy(&a.count_x, static_cast<const uint8_t *>(push) + 24, 4);
	memcpy(&a.count_y, static_cast<const uint8_t *>(push) + 28, 4);
	for (uint32_t y = 0; y < a.count_y; y++)
		for (uint32_t x = 0; x < a.count_x; x++)
		{
			uint16_t *at = out + (size_t(y) * a.count_x + x) * channels;
			if (channels == 1)
				mipmap_texel<1>(a, x, y, at);
			else if (channels == 2)
				mipmap_texel<2>(a, x, y, at);
			else if (channels == 4)
				mipmap_texel<4>(a, x, y, at);
			else
				return -1;
		}
	return 0;
}
