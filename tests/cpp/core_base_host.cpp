// granite_amd/csrc/core_base.hpp built for the host: a stand-alone program (tests/test_core_base_cpu.py builds it plainly and with
// -fsanitize=address,undefined and runs it directly), so that the two fp16 conversions every *_core.hpp header takes from it are held to
// numpy's.  Of the project's headers it includes core_base.hpp alone.
//
//   core_base_host <input file>    writes the result to stdout
// input file: fp32 bit patterns, little-endian 32-bit words
// result: float_to_half of each as a 16-bit word, then the bit pattern of half_to_float of all 65536 codes as 32-bit words
#include <cstdio>
#include <vector>
#include "../../granite_amd/csrc/core_base.hpp"

int main(int argc, char **argv)
{
	FILE *file = argc == 2 ? fopen(argv[1], "rb") : nullptr;
	if (!file)
	{
		fprintf(stderr, "usage: core_base_host <input file>\n");
		return 2;
	}
	std::vector<uint32_t> in;
	uint32_t block[4096];
	for (size_t n; (n = fread(block, 4, 4096, file)) != 0;)
		in.insert(in.end(), block, block + n);
	fclose(file);

	std::vector<uint16_t> halves(in.size());
	for (size_t i = 0; i < in.size(); i++)
	{
		float f;
		memcpy(&f, &in[i], 4);
		halves[i] = uint16_t(gr_core::float_to_half(f));
	}
	std::vector<uint32_t> floats(65536);
	for (uint32_t h = 0; h < 65536u; h++)
	{
		const float f = gr_core::half_to_float(h);
		memcpy(&floats[h], &f, 4);
	}
	fwrite(halves.data(), 2, halves.size(), stdout);
	fwrite(floats.data(), 4, floats.size(), stdout);
	return 0;
}
