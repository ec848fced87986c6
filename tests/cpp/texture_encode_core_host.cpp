// granite_amd/csrc/texture_encode_core.hpp built for the host: a stand-alone program for tests/test_texture_encode_core_cpu.py.
// It walks an image the way the kernels of texture_encode.hip do -- a group of 16 lanes a channel block, each step of the kernel a loop
// over the lanes with the kernel's shared arrays between the steps; one destination texel at a time for the mip level -- and holds
// the group walk to encode_channel_block, the same rules in a single thread's order.
//
//   texture_encode_core_host <case file>      the result goes to stdout
// case file, little endian u32 words then bytes:
//   0, width, height, stride, channels, pitch, pixels[height * pitch]          -> ceil(w/4) * ceil(h/4) blocks of 8 * channels bytes
//   1, src_width, src_height, channels, pixels[src_height * src_width * channels]  -> the level below, tightly packed
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../granite_amd/csrc/texture_encode_core.hpp"

namespace te = gr_texenc;
constexpr int GROUP = 16;

static void group_encode(const uint8_t *image, uint32_t bx, uint32_t by, uint32_t channel, uint32_t width, uint32_t height, uint32_t pitch, uint32_t stride,
                         uint8_t *out)
{
	uint8_t texels[16], sorted[16] = {};
	int below[16] = {}, above[16] = {}, value[GROUP], error[GROUP] = {};
	uint64_t bits[GROUP] = {};
	for (int lane = 0; lane < 16; lane++)
		texels[lane] = uint8_t(value[lane] = image[te::block_texel_offset(bx, by, lane, width, height, pitch, stride) + channel]);
	int lo = 255, hi = 0;
	for (int i = 0; i < 16; i++)
	{
		lo = texels[i] < lo ? texels[i] : lo;
		hi = texels[i] > hi ? texels[i] : hi;
	}
	const int range = hi - lo;
	int e0 = hi, e1 = lo;
	const bool searched = range >= te::RANGE_THRESHOLD;
	for (int lane = 0; lane < 16 && range != 0; lane++)
	{
		const int position = te::quantise(value[lane], lo, te::divider7(range));
		error[lane] = te::error7(value[lane], lo, range, position);
		bits[lane] = uint64_t(te::remap7(position)) << (3 * lane);
	}
	if (searched)
	{
		for (int lane = 0; lane < 16; lane++)
			sorted[te::rank_of(texels, lane)] = uint8_t(value[lane]);
		for (int lane = 0; lane < 15; lane++)
		{
			below[lane] = te::below_sum(sorted, lane);
			above[lane] = te::above_sum(sorted, lane);
		}
		int total = 0;
		for (int lane = 0; lane < 16; lane++)
			total += error[lane];
		uint32_t best = te::search_key(total, 0);
		for (int lane = 0; lane < GROUP; lane++)
		{
			for (int k = lane; k < te::CANDIDATES; k += GROUP)
			{
				int p, q;
				te::partition_by_width(k, p, q);
				const uint32_t key = te::search_key(below[p] + te::inside_sum(sorted, p, q, te::divider5(sorted[q] - sorted[p])) + above[q], te::candidate_index(p, q) + 1);
				best = key < best ? key : best;
			}
		}
		if (const int slot = te::key_slot(best))
		{
			int p, q;
			te::candidate_partition(slot - 1, p, q);
			e0 = sorted[p];
			e1 = sorted[q];
			for (int lane = 0; lane < 16; lane++)
				bits[lane] = uint64_t(te::code5(value[lane], e0, e1, te::divider5(e1 - e0))) << (3 * lane);
		}
	}
	uint64_t all = 0;
	for (int lane = 0; lane < 16; lane++)
		all |= bits[lane];
	out[0] = uint8_t(e0);
	out[1] = uint8_t(e1);
	for (int i = 0; i < 6; i++)
		out[2 + i] = uint8_t(all >> (8 * i));

	uint8_t serial[8];
	te::encode_channel_block(texels, serial);
	if (memcmp(serial, out, 8) != 0)
	{
		fprintf(stderr, "block (%u, %u) channel %u: the group walk and encode_channel_block differ\n", bx, by, channel);
		exit(3);
	}
}

// partition_by_width visits every partition of the search order once, widest first, and candidate_index inverts candidate_partition.
static bool orders_agree()
{
	bool seen[te::CANDIDATES] = {};
	int width = 14;
	for (int k = 0; k < te::CANDIDATES; k++)
	{
		int lo, hi, p, q;
		te::partition_by_width(k, lo, hi);
		if (lo < 0 || hi < lo || hi > 14 || hi - lo > width)
			return false;
		width = hi - lo;
		const int c = te::candidate_index(lo, hi);
		te::candidate_partition(c, p, q);
		if (c < 0 || c >= te::CANDIDATES || seen[c] || p != lo || q != hi)
			return false;
		seen[c] = true;
	}
	return true;
}

int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	for (int range = 0; range < 256; range++)
	{
		if (!te::ends_cost_nothing(range))
		{
			fprintf(stderr, "range %d: an end of a partition does not decode to itself\n", range);
			return 3;
		}
	}
	if (!orders_agree())
	{
		fprintf(stderr, "partition_by_width is no permutation of the search order\n");
		return 3;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	std::vector<uint8_t> raw;
	uint8_t chunk[4096];
	size_t n;
	while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0)
		raw.insert(raw.end(), chunk, chunk + n);
	fclose(f);
	auto word = [&](size_t i) {
		uint32_t v;
		memcpy(&v, raw.data() + 4 * i, 4);
		return v;
	};
	if (raw.size() < 4)
		return 2;
	if (word(0) == 0)
	{
		if (raw.size() < 24)
			return 2;
		const uint32_t width = word(1), height = word(2), stride = word(3), channels = word(4), pitch = word(5);
		if (raw.size() != 24 + size_t(height) * pitch || !width || !height || pitch < width * stride || channels > stride || channels < 1 || channels > 2)
			return 2;
		const uint8_t *image = raw.data() + 24;
		const uint32_t blocks_x = (width + 3) / 4, blocks_y = (height + 3) / 4;
		std::vector<uint8_t> out(size_t(blocks_x) * blocks_y * channels * 8);
		for (uint32_t by = 0; by < blocks_y; by++)
			for (uint32_t index = 0; index < blocks_x * channels; index++)
				group_encode(image, index / channels, by, index % channels, width, height, pitch, stride, out.data() + (size_t(by) * blocks_x * channels + index) * 8);
		fwrite(out.data(), 1, out.size(), stdout);
		return 0;
	}
	if (word(0) == 1)
	{
		if (raw.size() < 16)
			return 2;
		const uint32_t src_width = word(1), src_height = word(2), channels = word(3);
		if (!src_width || !src_height || raw.size() != 16 + size_t(src_width) * src_height * channels)
			return 2;
		const uint8_t *src = raw.data() + 16;
		const uint32_t width = src_width >> 1 ? src_width >> 1 : 1, height = src_height >> 1 ? src_height >> 1 : 1;
		const float rescale_x = te::mip_rescale(src_width, width), rescale_y = te::mip_rescale(src_height, height);
		std::vector<uint8_t> out(size_t(width) * height * channels);
		for (uint32_t y = 0; y < height; y++)
		{
			for (uint32_t x = 0; x < width; x++)
			{
				uint32_t x0, x1, y0, y1;
				float wx, wy;
				te::mip_axis(x, rescale_x, src_width, x0, x1, wx);
				te::mip_axis(y, rescale_y, src_height, y0, y1, wy);
				const uint8_t *top = src + size_t(y0) * src_width * channels, *bottom = src + size_t(y1) * src_width * channels;
				for (uint32_t c = 0; c < channels; c++)
					out[(size_t(y) * width + x) * channels + c] = uint8_t(
					    te::mip_filter(top[x0 * channels + c], top[x1 * channels + c], bottom[x0 * channels + c], bottom[x1 * channels + c], wx, wy));
			}
		}
		fwrite(out.data(), 1, out.size(), stdout);
		return 0;
	}
	return 2;
}
