// granite_amd/csrc/sky_core.hpp built for the host: a stand-alone program (tests/test_sky_core_cpu.py builds it plainly and with
// -fsanitize=address,undefined and runs it directly), so that the text the kernels of sky.hip run is held to the executed shaders before a
// device sees it.  It visits the far pixels of an image the way k_sky_apply does -- 16 x 16 tiles, the tile's far pixels compacted into a
// list in lane order, the list walked -- and the texels of a cube as k_sky_cube does.
//
//   sky_core_host <case file>      writes the result to stdout
// case file, little endian, 32-bit words:
//   0 (apply): width height inv[16] color[3] camera_height sun_direction[3] cube_size cube_levels n cube_words[n] depth[w*h]
//                                                            -> rgb[w*h*3] floats (0 where not far), then written[w*h] words
//   1 (cube):  size sun_color[3] camera_y sun_direction[3]   -> rgba[6*size*size*4] floats
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../granite_amd/csrc/sky_core.hpp"

using namespace gr_sky;

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
	float f32()
	{
		const uint32_t w = u32();
		float f;
		memcpy(&f, &w, 4);
		return f;
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
};

template <typename T> void emit(const std::vector<T> &v) { fwrite(v.data(), sizeof(T), v.size(), stdout); }

void apply(Reader &r)
{
	const uint32_t width = r.u32(), height = r.u32();
	const auto inv = r.array<float>(16), color = r.array<float>(3);
	const float camera_height = r.f32();
	const auto sun = r.array<float>(3);
	const uint32_t cube_size = r.u32(), cube_levels = r.u32();
	// 8-byte texels: the words live in a vector of 64-bit elements
	const auto cube_words = r.array<uint32_t>(r.u32());
	std::vector<uint64_t> cube_store((cube_words.size() + 1) / 2);
	if (!cube_words.empty())
		memcpy(cube_store.data(), cube_words.data(), cube_words.size() * 4);
	const auto depth = r.array<float>(size_t(width) * height);
	const gr_env::Cube cube = {reinterpret_cast<const uint8_t *>(cube_store.data()), cube_size, cube_levels};
	if (cube_size && cube_words.size() * 4 < gr_env::chain_offset(cube_size, cube_levels, 0))
	{
		fprintf(stderr, "the cube's words do not cover its chain\n");
		exit(2);
	}

	std::vector<float> rgb(size_t(width) * height * 3, 0.0f);
	std::vector<uint32_t> written(size_t(width) * height, 0u);
	constexpr uint32_t TILE = 16;
	for (uint32_t tile_y = 0; tile_y < height; tile_y += TILE)
		for (uint32_t tile_x = 0; tile_x < width; tile_x += TILE)
		{
			uint8_t list[TILE * TILE];
			uint32_t total = 0;
			for (uint32_t tid = 0; tid < TILE * TILE; tid++)
			{
				const uint32_t x = tile_x + (tid & (TILE - 1)), y = tile_y + tid / TILE;
				if (x < width && y < height && depth[size_t(y) * width + x] == 0.0f)
					list[total++] = uint8_t(tid);
			}
			for (uint32_t i = 0; i < total; i++)
			{
				const uint32_t x = tile_x + (list[i] & (TILE - 1)), y = tile_y + list[i] / TILE;
				const f3 c = cube_size ? sky_textured(cube, inv.data(), width, height, x, y, color.data())
				                       : sky_procedural(pixel_direction(inv.data(), width, height, x, y), color.data(), sun.data(), camera_height);
				float *o = &rgb[(size_t(y) * width + x) * 3];
				o[0] = c.x, o[1] = c.y, o[2] = c.z;
				written[size_t(y) * width + x]++;
			}
		}
	emit(rgb);
	emit(written);
}

void cube(Reader &r)
{
	const uint32_t size = r.u32();
	const auto sun_color = r.array<float>(3);
	const float camera_y = r.f32();
	const auto sun = r.array<float>(3);
	const float inv_resolution = 1.0f / float(size);
	std::vector<float> rgba(size_t(6) * size * size * 4);
	for (uint32_t face = 0; face < 6; face++)
		for (uint32_t index = 0; index < size * size; index++)
		{
			const f3 c = sky_cube_texel(face, index % size, index / size, inv_resolution, sun_color.data(), sun.data(), camera_y);
			float *o = &rgba[(size_t(face) * size * size + index) * 4];
			o[0] = c.x, o[1] = c.y, o[2] = c.z, o[3] = 1.0f;
		}
	emit(rgba);
}
} // namespace

int main(int argc, char **argv)
{
	if (argc != 2)
	{
		fprintf(stderr, "usage: sky_core_host <case file>\n");
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
	switch (r.u32())
	{
	case 0: apply(r); break;
	case 1: cube(r); break;
	default: fprintf(stderr, "unknown case kind\n"); return 2;
	}
	return 0;
}
