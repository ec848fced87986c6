// TEST INFRASTRUCTURE.  granite_amd/csrc/astc_decode.hpp -- the ASTC decode the device kernel of texture_decode.hip calls -- built for the
// host.  tests/test_astc_host_cpu.py holds it to the golden of the executed shader (tests/golden/astc_decode_shader_v1.npz) before a
// device sees the code, plain and under -fsanitize=address,undefined.
//   astc_decode_host decode BW BH WIDTH HEIGHT blocks.bin out.bin   tightly packed blocks -> tightly packed RGBA8, in the kernel's order:
//                                                                   64 neighbouring blocks parsed into records (the block half), then
//                                                                   their texels row by row, 64 to a turn (the texel half)
//   astc_decode_host tables out.bin       the compile-time tables in the layout of the shader's buffers: endpoint quantiser
//                                         u16[9][128][4], endpoint unquantise u8[1192], weight quantiser u8[16][4], weight unquantise
//                                         u8[142], trits / quints u16[384]
//   astc_decode_host partition BW BH out.bin   the partition table the shader reads as a texture, u8[32 * BH][32 * BW], from the hash
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../granite_amd/csrc/astc_decode.hpp"

static bool read_file(const char *path, std::vector<uint8_t> &data)
{
	FILE *f = fopen(path, "rb");
	if (!f)
		return false;
	const bool ok = fread(data.data(), 1, data.size(), f) == data.size();
	fclose(f);
	return ok;
}

static int write_file(const char *path, const std::vector<uint8_t> &data)
{
	FILE *f = fopen(path, "wb");
	if (!f || fwrite(data.data(), 1, data.size(), f) != data.size())
		return 3;
	return fclose(f) == 0 ? 0 : 3;
}

static void decode(const uint8_t *blocks, uint8_t *out, int bw, int bh, int w, int h)
{
	const int blocks_x = (w + bw - 1) / bw, blocks_y = (h + bh - 1) / bh;
	for (int by = 0; by < blocks_y; by++)
		for (int bx0 = 0; bx0 < blocks_x; bx0 += 64)
		{
			gr_astc::Block records[64];
			for (int lane = 0; lane < 64 && bx0 + lane < blocks_x; lane++)
			{
				gr_astc::Payload p;
				memcpy(&p.lo, blocks + (size_t(by) * blocks_x + bx0 + lane) * 16, 8);
				memcpy(&p.hi, blocks + (size_t(by) * blocks_x + bx0 + lane) * 16 + 8, 8);
				gr_astc::decode_block(p, bw, bh, records[lane]);
			}
			for (int turn = 0; turn < bw * bh; turn++)
				for (int lane = 0; lane < 64; lane++)
				{
					const int ly = turn / bw, lx = (turn % bw) * 64 + lane;
					const int x = bx0 * bw + lx, y = by * bh + ly;
					if (x >= w || y >= h)
						continue;
					const uint32_t texel = gr_astc::decode_texel(records[lx / bw], lx % bw, ly, bw, bh);
					memcpy(out + (size_t(y) * w + x) * 4, &texel, 4);
				}
		}
}

template <typename T> static void append(std::vector<uint8_t> &out, T v)
{
	uint8_t raw[sizeof(T)];
	memcpy(raw, &v, sizeof(T));
	out.insert(out.end(), raw, raw + sizeof(T));
}

static bool is_footprint(int bw, int bh)
{
	for (int i = 0; i < gr_astc::FOOTPRINT_COUNT; i++)
		if (gr_astc::footprint(i).w == bw && gr_astc::footprint(i).h == bh)
			return true;
	return false;
}

int main(int argc, char **argv)
{
	if (argc == 3 && !strcmp(argv[1], "tables"))
	{
		const gr_astc::Tables &t = gr_astc::tables();
		std::vector<uint8_t> out;
		for (int pairs = 0; pairs < 9; pairs++)
			for (int remaining = 0; remaining < 128; remaining++)
			{
				const int m = t.endpoint_quantiser[pairs][remaining];
				const gr_astc::Quant q = m == 0xff ? gr_astc::Quant{0, 0, 0} : gr_astc::endpoint_mode(m);
				append<uint16_t>(out, q.bits);
				append<uint16_t>(out, q.trits);
				append<uint16_t>(out, q.quints);
				append<uint16_t>(out, m == 0xff ? 0 : t.endpoint_unquant_offset[m]);
			}
		out.insert(out.end(), t.endpoint_unquant, t.endpoint_unquant + gr_astc::ENDPOINT_UNQUANT_SIZE);
		for (int m = 0; m < gr_astc::WEIGHT_MODES; m++)
		{
			const gr_astc::Quant q = gr_astc::weight_mode(m);
			out.push_back(q.bits);
			out.push_back(q.trits);
			out.push_back(q.quints);
			out.push_back(t.weight_unquant_offset[m]);
		}
		out.insert(out.end(), t.weight_unquant, t.weight_unquant + gr_astc::WEIGHT_UNQUANT_SIZE);
		for (int i = 0; i < 256 + 128; i++)
			append<uint16_t>(out, t.trits_quints[i]);
		return write_file(argv[2], out);
	}
	if (argc == 5 && !strcmp(argv[1], "partition"))
	{
		const int bw = atoi(argv[2]), bh = atoi(argv[3]);
		if (!is_footprint(bw, bh))
			return 2;
		std::vector<uint8_t> out(size_t(32 * bw) * (32 * bh));
		for (int seed = 0; seed < 1024; seed++)
			for (int y = 0; y < bh; y++)
				for (int x = 0; x < bw; x++)
				{
					int packed = 0;
					for (int partitions = 2; partitions <= 4; partitions++)
					{
						gr_astc::Block b = {};
						b.partitions = uint8_t(partitions);
						gr_astc::partition_hash(b, seed, partitions);
						packed |= gr_astc::partition_of(b, x, y, bw * bh < 31) << (2 * partitions - 4);
					}
					out[size_t((seed >> 5) * bh + y) * (32 * bw) + (seed & 31) * bw + x] = uint8_t(packed);
				}
		return write_file(argv[4], out);
	}
	if (argc != 8 || strcmp(argv[1], "decode"))
		return 2;
	const int bw = atoi(argv[2]), bh = atoi(argv[3]), w = atoi(argv[4]), h = atoi(argv[5]);
	if (!is_footprint(bw, bh) || w <= 0 || h <= 0)
		return 2;
	std::vector<uint8_t> blocks(size_t((w + bw - 1) / bw) * ((h + bh - 1) / bh) * 16), out(size_t(w) * h * 4);
	if (!read_file(argv[6], blocks))
		return 3;
	decode(blocks.data(), out.data(), bw, bh, w, h);
	return write_file(argv[7], out);
}
