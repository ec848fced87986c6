// granite_amd/csrc/decal_core.hpp built for the host: a stand-alone program (tests/test_decal_core_cpu.py builds it plainly and with
// -fsanitize=address,undefined and runs it directly).  It walks cells and pixels the way the kernels of decal.hip do -- one 8 x 8 tile of
// 64 "lanes" at a time, the tile test before the cell test, the wave-wide OR of the lanes' masked words as the candidate set, the quad
// partners' uv taken from lanes ^ 1 and ^ 8 -- so that the same text is held to the executed shaders before a device sees it.
//
//   decal_core_host <case file>      writes the result to stdout
// case file, little endian, 32-bit words:
//   0 (binning): prm[44] n_mvp_floats mvps[]                                   -> bitmask words
//   1 (apply):   prm[44] width height inv_vp[16] n rows[n] n bitmask[n] n range[n] albedo[w*h] depth[w*h] srgb[256]
//                num_textures { width height num_levels format n texels[n] }   -> colour[w*h*3] floats, then touched[w*h] words
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../granite_amd/csrc/decal_core.hpp"
#include "../../include/granite_hip.h"

using namespace gr_decal;

namespace
{
struct Reader
{
	std::vector<uint32_t> words;
	size_t at = 0;
	uint32_t u32()
	{
		if (at >= words.size())
		{
			fprintf(stderr, "case file is too short\n");
			exit(2);
		}
		return words[at++];
	}
	template <typename T> std::vector<T> array(size_t count)
	{
		static_assert(sizeof(T) == 4, "32-bit elements");
		std::vector<T> out(count);
		for (auto &v : out)
		{
			const uint32_t w = u32();
			memcpy(&v, &w, 4);
		}
		return out;
	}
	template <typename T> std::vector<T> counted() { return array<T>(u32()); }
};

gr_cluster_params read_params(Reader &r)
{
	const auto raw = r.array<uint32_t>(sizeof(gr_cluster_params) / 4);
	gr_cluster_params p;
	memcpy(&p, raw.data(), sizeof(p));
	return p;
}

void binning(Reader &r)
{
	const gr_cluster_params prm = read_params(r);
	const auto mvps = r.counted<float>();
	const uint32_t res_x = uint32_t(prm.resolution_xy[0]), res_y = uint32_t(prm.resolution_xy[1]);
	const uint32_t n = uint32_t(prm.num_decals), n32 = uint32_t(prm.num_decals_32);
	const float inv_x = prm.inv_resolution_xy[0], inv_y = prm.inv_resolution_xy[1];
	std::vector<uint32_t> bitmask(size_t(res_x) * res_y * n32, 0xcdcdcdcdu);
	for (uint32_t pair = 0; pair < (n32 + 1u) / 2u; pair++)
		for (uint32_t tile_y = 0; tile_y < res_y / 8u; tile_y++)
			for (uint32_t tile_x = 0; tile_x < res_x / 8u; tile_x++)
			{
				Vec4 bb[64];
				uint64_t ballot = 0;
				for (uint32_t lane = 0; lane < 64u; lane++)
				{
					const uint32_t decal = 64u * pair + lane;
					bb[lane] = {1.0f, 1.0f, -1.0f, -1.0f};
					if (decal < n)
						bb[lane] = compute_decal_screen_bb(&mvps[size_t(decal) * 16u]);
					if (test_decal(cell_uv(tile_x * 8u, inv_x), cell_uv(tile_y * 8u, inv_y), (2.0f * 8.0f) * inv_x, (2.0f * 8.0f) * inv_y, bb[lane]))
						ballot |= 1ull << lane;
				}
				for (uint32_t lane = 0; lane < 64u; lane++)
				{
					const uint32_t px = tile_x * 8u + (lane & 7u), py = tile_y * 8u + (lane >> 3u);
					uint32_t mask[2] = {0u, 0u};
					for (uint64_t walk = ballot; walk != 0ull; walk &= walk - 1ull)
					{
						const int bit = __builtin_ctzll(walk);
						if (test_decal(cell_uv(px, inv_x), cell_uv(py, inv_y), 2.0f * inv_x, 2.0f * inv_y, bb[bit]))
							mask[bit >> 5] |= 1u << (bit & 31);
					}
					const size_t base = (size_t(py) * res_x + px) * n32 + 2u * pair;
					bitmask[base] = mask[0];
					if (2u * pair + 1u < n32)
						bitmask[base + 1u] = mask[1];
				}
			}
	fwrite(bitmask.data(), 4, bitmask.size(), stdout);
}

void apply(Reader &r)
{
	const gr_cluster_params cl = read_params(r);
	const uint32_t width = r.u32(), height = r.u32();
	const auto inv_vp = r.array<float>(16);
	const auto rows = r.counted<float>();
	const auto bitmask = r.counted<uint32_t>();
	const auto range = r.counted<uint32_t>();
	const auto albedo = r.array<uint32_t>(size_t(width) * height);
	const auto depth = r.array<float>(size_t(width) * height);
	const auto srgb = r.array<float>(256);
	const uint32_t num_textures = r.u32();
	std::vector<std::vector<uint32_t>> texels(num_textures);
	std::vector<Texture> textures(num_textures);
	for (uint32_t i = 0; i < num_textures; i++)
	{
		textures[i].width = r.u32();
		textures[i].height = r.u32();
		textures[i].num_levels = r.u32();
		textures[i].format = r.u32();
		texels[i] = r.counted<uint32_t>();
		textures[i].levels = texels[i].data();
	}
	const uint32_t num_decals = uint32_t(cl.num_decals), n32 = uint32_t(cl.num_decals_32);
	const float inv_width = 1.0f / float(width), inv_height = 1.0f / float(height);
	std::vector<float> colour(size_t(width) * height * 3u);
	std::vector<uint32_t> touched(size_t(width) * height, 0u);
	for (size_t i = 0; i < albedo.size(); i++)
		for (uint32_t c = 0; c < 3u; c++)
			colour[3u * i + c] = srgb[(albedo[i] >> (8u * c)) & 255u];

	for (uint32_t tile_y = 0; tile_y < (height + 7u) / 8u; tile_y++)
		for (uint32_t tile_x = 0; tile_x < (width + 7u) / 8u; tile_x++)
		{
			bool active[64];
			Vec3 pos[64];
			uint32_t range_x[64], range_y[64];
			size_t cluster_base[64];
			uint32_t z_start = 0xffffffffu, z_end = 0u;
			bool any = false;
			for (uint32_t lane = 0; lane < 64u; lane++)
			{
				const uint32_t x = tile_x * 8u + (lane & 7u), y = tile_y * 8u + (lane >> 3u);
				const bool inside = x < width && y < height;
				const float d = inside ? depth[size_t(y) * width + x] : 0.0f;
				active[lane] = inside && d != 0.0f;
				any = any || active[lane];
				pos[lane] = active[lane] ? world_position(inv_vp.data(), x, y, inv_width, inv_height, d) : Vec3{0.0f, 0.0f, 0.0f};
				range_x[lane] = 0xffffffffu;
				range_y[lane] = 0u;
				cluster_base[lane] = 0;
				if (active[lane])
				{
					const int cx = cluster_cell(x, inv_width, cl.xy_scale[0], cl.resolution_xy[0]);
					const int cy = cluster_cell(y, inv_height, cl.xy_scale[1], cl.resolution_xy[1]);
					cluster_base[lane] = (size_t(cy) * uint32_t(cl.resolution_xy[0]) + uint32_t(cx)) * n32;
					const size_t slice = size_t(z_slice(pos[lane], cl.camera_base, cl.camera_front, cl.z_scale, cl.z_max_index));
					range_x[lane] = range.at(2u * slice);
					range_y[lane] = range.at(2u * slice + 1u);
				}
				z_start = range_x[lane] < z_start ? range_x[lane] : z_start;
				z_end = range_y[lane] > z_end ? range_y[lane] : z_end;
			}
			if (!any || n32 == 0u)
				continue;
			z_start >>= 5u;
			z_end = (z_end >> 5u) < n32 - 1u ? (z_end >> 5u) : n32 - 1u;
			for (uint32_t i = z_start; i <= z_end && z_start <= z_end; i++)
			{
				uint32_t own[64], candidates = 0u;
				for (uint32_t lane = 0; lane < 64u; lane++)
				{
					own[lane] = active[lane] ? cluster_mask_range(bitmask.at(cluster_base[lane] + i), range_x[lane], range_y[lane], 32u * i) : 0u;
					candidates |= own[lane];
				}
				for (; candidates != 0u; candidates &= candidates - 1u)
				{
					const uint32_t bit = uint32_t(__builtin_ctz(candidates));
					const uint32_t index = 32u * i + bit, texture_index = uint32_t(cl.decals_texture_offset) + index;
					if (index >= num_decals || texture_index >= num_textures)
						continue;
					Vec3 uvw[64];
					for (uint32_t lane = 0; lane < 64u; lane++)
						uvw[lane] = decal_uvw(&rows.at(size_t(index) * 12u), pos[lane]);
					for (uint32_t lane = 0; lane < 64u; lane++)
					{
						if (!(((own[lane] >> bit) & 1u) != 0u && uvw_in_range(uvw[lane])))
							continue;
						const float u = uvw[lane].x + 0.5f, v = uvw[lane].y + 0.5f;
						const uint32_t lx = lane ^ 1u, ly = lane ^ 8u;
						const bool has_dx = active[lx], has_dy = active[ly];
						const float sign_x = (lane & 1u) ? 1.0f : -1.0f, sign_y = (lane & 8u) ? 1.0f : -1.0f;
						const float dudx = has_dx ? sign_x * (u - (uvw[lx].x + 0.5f)) : 0.0f, dvdx = has_dx ? sign_x * (v - (uvw[lx].y + 0.5f)) : 0.0f;
						const float dudy = has_dy ? sign_y * (u - (uvw[ly].x + 0.5f)) : 0.0f, dvdy = has_dy ? sign_y * (v - (uvw[ly].y + 0.5f)) : 0.0f;
						const Texture &tex = textures[texture_index];
						const float lambda = texture_lod(dudx, dvdx, dudy, dvdy, tex.width, tex.height, tex.num_levels);
						const Vec4 decal = sample_texture(tex, u, v, lambda, srgb.data());
						const size_t pixel = size_t(tile_y * 8u + (lane >> 3u)) * width + tile_x * 8u + (lane & 7u);
						const Vec3 blended = blend_decal({colour[3u * pixel], colour[3u * pixel + 1u], colour[3u * pixel + 2u]}, decal);
						colour[3u * pixel] = blended.x;
						colour[3u * pixel + 1u] = blended.y;
						colour[3u * pixel + 2u] = blended.z;
						touched[pixel] = 1u;
					}
				}
			}
		}
	fwrite(colour.data(), 4, colour.size(), stdout);
	fwrite(touched.data(), 4, touched.size(), stdout);
}
} // namespace

int main(int argc, char **argv)
{
	if (argc != 2)
	{
		fprintf(stderr, "usage: %s <case file>\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f)
	{
		perror(argv[1]);
		return 2;
	}
	Reader r;
	uint32_t w;
	while (fread(&w, 4, 1, f) == 1)
		r.words.push_back(w);
	fclose(f);
	const uint32_t mode = r.u32();
	if (mode == 0u)
		binning(r);
	else
		apply(r);
	return 0;
}
