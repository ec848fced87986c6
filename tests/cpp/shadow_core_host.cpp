// granite_amd/csrc/shadow_core.hpp built for the host: a stand-alone program (tests/test_shadow_core_cpu.py builds it plainly and with
// -fsanitize=address,undefined and runs it directly), so that the text the kernels of shadow.hip run is held to the executed shaders before
// a device sees it.  Every pixel indexes the cascade matrices by its own layers: what the kernel's wave-uniform loop selects.
//
//   shadow_core_host <case file>      writes the result to stdout
// case file, little endian, 32-bit words (16-bit and 8-bit arrays padded to whole words):
//   0 (directional): width height mode cascaded fallback ao_w ao_h map_w map_h layers map_format(0 D16, 1 D32, 2 RG32F)
//                    inv_vp[16] transforms[64] color[3] camera_pos[3] direction[3] camera_front[3] log_bias srgb[256]
//                    albedo[w*h] normal[w*h] depth[w*h] emissive[w*h*4 halves] pbr[w*h halves] ao[ao_w*ao_h bytes] maps
//                    -> hdr[w*h*4] halves, term[w*h] floats, layers[w*h*2] words, lerps[w*h*2] floats
//   1 (moments):     width height format depth            -> moments[w*h*2] floats
//   2 (blur):        in_w in_h layers out_w out_h up in[layers*in_h*in_w*2] -> out[layers*out_h*out_w*2] floats
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../granite_amd/csrc/shadow_core.hpp"

using namespace gr_shadow;

namespace
{
struct Reader
{
	std::vector<uint32_t> words;
	size_t at = 0;
	void need(size_t count)
	{
		if (count > words.size() - at)
		{
			fprintf(stderr, "case file is too short\n");
			exit(2);
		}
	}
	uint32_t u32()
	{
		need(1);
		return words[at++];
	}
	float f32()
	{
		const uint32_t w = u32();
		float f;
		memcpy(&f, &w, 4);
		return f;
	}
	// `bytes` bytes, padded to whole words in the file; the copy is 8-byte aligned and holds whole words
	std::vector<uint64_t> bytes(size_t bytes)
	{
		const size_t count = (bytes + 3) / 4;
		need(count);
		std::vector<uint64_t> out((count + 1) / 2 + 1);
		if (count)
			memcpy(out.data(), words.data() + at, count * 4);
		at += count;
		return out;
	}
	std::vector<float> floats(size_t count)
	{
		std::vector<float> out(count);
		for (auto &v : out)
			v = f32();
		return out;
	}
};

template <typename T> void emit(const std::vector<T> &v) { fwrite(v.data(), sizeof(T), v.size(), stdout); }
uint32_t limited(Reader &r, uint32_t lo, uint32_t hi, const char *what)
{
	const uint32_t v = r.u32();
	if (v < lo || v > hi)
	{
		fprintf(stderr, "%s %u is not %u .. %u\n", what, v, lo, hi);
		exit(2);
	}
	return v;
}

template <int MODE, bool D16>
float pixel_term(const Maps &maps, bool cascaded, const float *transforms, f3 pos, f3 camera_pos, f3 camera_front, float log_bias, int32_t *layers, float *lerps)
{
	if (!cascaded)
		return layer_term<MODE, D16>(maps.layer[0], maps.width, maps.height, light_clip(transforms, pos));
	const Cascade c = compute_shadow_cascade(pos, camera_pos, camera_front, log_bias);
	layers[0] = c.layer_near, layers[1] = c.layer_far;
	lerps[0] = c.shadow_lerp, lerps[1] = c.white_lerp;
	float term_near = 1.0f, term_far = 1.0f;
	for (int i = c.layer_near; i <= c.layer_far; i++)
		cascade_turn<MODE, D16>(maps, transforms, i, c, pos, term_near, term_far);
	return blend_cascade(c, term_near, term_far);
}

void directional(Reader &r)
{
	const uint32_t width = limited(r, 1, 4096, "width"), height = limited(r, 1, 4096, "height");
	const uint32_t mode = limited(r, 1, 3, "mode"), cascaded = limited(r, 0, 1, "cascaded"), fallback = limited(r, 0, 1, "fallback");
	const uint32_t ao_w = limited(r, 0, 4096, "ao_w"), ao_h = limited(r, 0, 4096, "ao_h");
	const uint32_t map_w = limited(r, 1, 16384, "map_w"), map_h = limited(r, 1, 16384, "map_h"), layers = limited(r, 1, 4, "layers");
	const uint32_t format = limited(r, 0, 2, "map_format");
	if ((mode == uint32_t(MODE_VSM)) != (format == 2u) || (cascaded && layers != 4u))
	{
		fprintf(stderr, "the map's format or layer count does not fit the mode\n");
		exit(2);
	}
	const auto inv_vp = r.floats(16), transforms = r.floats(64), color = r.floats(3), camera_pos = r.floats(3), direction = r.floats(3), camera_front = r.floats(3);
	const float log_bias = r.f32();
	const auto srgb = r.floats(256);
	const size_t pixels = size_t(width) * height;
	const auto albedo = r.bytes(pixels * 4), normal = r.bytes(pixels * 4), depth = r.bytes(pixels * 4), emissive = r.bytes(pixels * 8), pbr = r.bytes(pixels * 2);
	const auto ao = r.bytes(size_t(ao_w) * ao_h);
	const uint32_t texel = format == 0 ? 2u : (format == 1 ? 4u : 8u);
	const auto map_store = r.bytes(size_t(layers) * map_w * map_h * texel);

	Maps maps = {};
	maps.width = int(map_w), maps.height = int(map_h);
	for (uint32_t i = 0; i < layers; i++)
		maps.layer[i] = {reinterpret_cast<const uint8_t *>(map_store.data()) + size_t(i) * map_w * map_h * texel, map_w * texel};

	std::vector<uint16_t> hdr(pixels * 4);
	std::vector<float> term(pixels, 1.0f), lerps(pixels * 2, 0.0f);
	std::vector<int32_t> layer_out(pixels * 2, 0);
	memcpy(hdr.data(), emissive.data(), pixels * 8);
	const float inv_width = 1.0f / float(width), inv_height = 1.0f / float(height);
	const f3 cam = {camera_pos[0], camera_pos[1], camera_pos[2]}, front = {camera_front[0], camera_front[1], camera_front[2]};
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++)
		{
			const size_t p = size_t(y) * width + x;
			const float z = reinterpret_cast<const float *>(depth.data())[p];
			if (z == 0.0f)
				continue;
			const f3 pos = world_position(inv_vp.data(), inv_vp.data() + 8, inv_width, inv_height, x, y, z);
			float t;
			int32_t *lo = &layer_out[2 * p];
			float *le = &lerps[2 * p];
			if (mode == uint32_t(MODE_VSM))
				t = pixel_term<MODE_VSM, false>(maps, cascaded, transforms.data(), pos, cam, front, log_bias, lo, le);
			else if (mode == uint32_t(MODE_PCF_WIDE))
				t = format == 0 ? pixel_term<MODE_PCF_WIDE, true>(maps, cascaded, transforms.data(), pos, cam, front, log_bias, lo, le)
				                : pixel_term<MODE_PCF_WIDE, false>(maps, cascaded, transforms.data(), pos, cam, front, log_bias, lo, le);
			else
				t = format == 0 ? pixel_term<MODE_PCF, true>(maps, cascaded, transforms.data(), pos, cam, front, log_bias, lo, le)
				                : pixel_term<MODE_PCF, false>(maps, cascaded, transforms.data(), pos, cam, front, log_bias, lo, le);
			term[p] = t;
			const Material m = decode_material(reinterpret_cast<const uint32_t *>(albedo.data())[p], reinterpret_cast<const uint32_t *>(normal.data())[p],
			                                   reinterpret_cast<const uint16_t *>(pbr.data())[p], srgb.data());
			f3 c = compute_lighting(m, t, pos, cam, {direction[0], direction[1], direction[2]}, {color[0], color[1], color[2]});
			if (fallback)
			{
				float base_ambient = 1.0f;
				if (ao_w && ao_h)
					base_ambient = sample_ambient_occlusion(reinterpret_cast<const uint8_t *>(ao.data()), ao_w, int(ao_w), int(ao_h), (float(x) + 0.5f) * inv_width,
					                                        (float(y) + 0.5f) * inv_height);
				c = add_ambient_fallback(c, m.base, base_ambient);
			}
			uint16_t *o = &hdr[4 * p];
			o[0] = uint16_t(gr_core::float_to_half(gr_core::half_to_float(o[0]) + c.x));
			o[1] = uint16_t(gr_core::float_to_half(gr_core::half_to_float(o[1]) + c.y));
			o[2] = uint16_t(gr_core::float_to_half(gr_core::half_to_float(o[2]) + c.z));
		}
	emit(hdr);
	emit(term);
	emit(layer_out);
	emit(lerps);
}

void moments(Reader &r)
{
	const uint32_t width = limited(r, 1, 16384, "width"), height = limited(r, 1, 16384, "height"), format = limited(r, 0, 1, "format");
	const uint32_t texel = format == 0 ? 2u : 4u;
	const auto store = r.bytes(size_t(width) * height * texel);
	const Layer depth = {reinterpret_cast<const uint8_t *>(store.data()), width * texel};
	std::vector<float> out(size_t(width) * height * 2);
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++)
		{
			const float z = format == 0 ? depth_texel<true>(depth, int(x), int(y)) : depth_texel<false>(depth, int(x), int(y));
			out[2 * (size_t(y) * width + x)] = z;
			out[2 * (size_t(y) * width + x) + 1] = z * z;
		}
	emit(out);
}

void blur(Reader &r)
{
	const uint32_t in_w = limited(r, 1, 16384, "in_w"), in_h = limited(r, 1, 16384, "in_h"), layers = limited(r, 1, 4, "layers");
	const uint32_t out_w = limited(r, 1, 16384, "out_w"), out_h = limited(r, 1, 16384, "out_h"), up = limited(r, 0, 1, "up");
	const auto store = r.bytes(size_t(layers) * in_w * in_h * 8);
	std::vector<float> out(size_t(layers) * out_w * out_h * 2);
	for (uint32_t layer = 0; layer < layers; layer++)
	{
		const Layer in = {reinterpret_cast<const uint8_t *>(store.data()) + size_t(layer) * in_w * in_h * 8, in_w * 8u};
		for (uint32_t y = 0; y < out_h; y++)
			for (uint32_t x = 0; x < out_w; x++)
			{
				float *o = &out[((size_t(layer) * out_h + y) * out_w + x) * 2];
				vsm_blur(in, int(in_w), int(in_h), (float(x) + 0.5f) / float(out_w), (float(y) + 0.5f) / float(out_h), up ? 0.875f : 1.75f, o[0], o[1]);
			}
	}
	emit(out);
}
} // namespace

int main(int argc, char **argv)
{
	if (argc != 2)
	{
		fprintf(stderr, "usage: shadow_core_host <case file>\n");
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
	case 0: directional(r); break;
	case 1: moments(r); break;
	case 2: blur(r); break;
	default: fprintf(stderr, "unknown case kind\n"); return 2;
	}
	return 0;
}
