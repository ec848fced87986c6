// TEST INFRASTRUCTURE.  granite_amd/csrc/bc_decode.hpp -- the block decode the device kernel of texture_decode.hip calls -- built for the
// host: bc_decode_host KIND LANES WIDTH HEIGHT blocks.bin out.bin decodes tightly packed blocks into a tightly packed image, one
// "lane" after another with the kernel's split of a block's rows over LANES lanes.  tests/test_bc_ref_cpu.py holds it to the golden of the
// executed shaders (tests/golden/bc_decode_shader_v1.npz) before a device sees the code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../granite_amd/csrc/bc_decode.hpp"

template <int KIND, int LANES>
static void decode(const uint8_t *blocks, uint8_t *out, int w, int h)
{
	constexpr int ROWS = 4 / LANES, BB = gr_bc::block_bytes(KIND), TB = gr_bc::texel_bytes(KIND);
	const int bw = (w + 3) / 4, bh = (h + 3) / 4;
	for (int by = 0; by < bh; by++)
		for (int bx = 0; bx < bw; bx++)
			for (int lane = 0; lane < LANES; lane++)
			{
				gr_bc::Payload p = {0, 0};
				memcpy(&p.lo, blocks + (size_t(by) * bw + bx) * BB, 8);
				if (BB == 16)
					memcpy(&p.hi, blocks + (size_t(by) * bw + bx) * BB + 8, 8);
				uint32_t words[ROWS][gr_bc::ROW_WORDS_MAX];
				gr_bc::decode_rows<KIND, ROWS>(p, lane * ROWS, words);
				for (int r = 0; r < ROWS; r++)
				{
					const int y = 4 * by + lane * ROWS + r;
					if (y >= h)
						break;
					const int texels = w - 4 * bx < 4 ? w - 4 * bx : 4;
					memcpy(out + (size_t(y) * w + 4 * bx) * TB, words[r], size_t(texels) * TB);
				}
			}
}

int main(int argc, char **argv)
{
	if (argc != 7)
		return 2;
	const int kind = atoi(argv[1]), lanes = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]);
	if (kind < 0 || kind >= gr_bc::KIND_COUNT || (lanes != 1 && lanes != 4) || w <= 0 || h <= 0)
		return 2;
	std::vector<uint8_t> blocks(size_t((w + 3) / 4) * ((h + 3) / 4) * gr_bc::block_bytes(kind)), out(size_t(w) * h * gr_bc::texel_bytes(kind));
	FILE *f = fopen(argv[5], "rb");
	if (!f || fread(blocks.data(), 1, blocks.size(), f) != blocks.size())
		return 3;
	fclose(f);
#define CASE(k) \
	case k: lanes == 4 ? decode<k, 4>(blocks.data(), out.data(), w, h) : decode<k, 1>(blocks.data(), out.data(), w, h); break;
	switch (kind)
	{
		CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
	}
	f = fopen(argv[6], "wb");
	if (!f || fwrite(out.data(), 1, out.size(), f) != out.size())
		return 3;
	return fclose(f) == 0 ? 0 : 3;
}
