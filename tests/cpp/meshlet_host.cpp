// TEST INFRASTRUCTURE.  granite_amd/csrc/host/mesh/meshlet.cpp -- create_mesh_view and decode_mesh's host arithmetic -- with no device:
//   meshlet_host FILE RUNTIME_STYLE FLAGS PRIMITIVE_OFFSET VERTEX_OFFSET out.bin
// writes build_decode_offsets' records, then build_indirect_records' bytes.  tests/test_meshlet_arith_cpu.py compares both with
// tests/meshlet_ref.py, whose answers tests/test_meshlet_ref_cpu.py holds to hand-written ones.  Exit 5 with the reason on stderr for a
// file the view refuses.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../granite_amd/csrc/host/mesh/meshlet.hpp"

using namespace Granite::Meshlet;

int main(int argc, char **argv)
{
	if (argc != 7)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 3;
	fseek(f, 0, SEEK_END);
	const size_t size = size_t(ftell(f));
	fseek(f, 0, SEEK_SET);
	std::vector<uint32_t> words((size + 3) / 4);
	if (fread(words.data(), 1, size, f) != size)
		return 3;
	fclose(f);
	std::string why;
	const MeshView view = create_mesh_view(words.data(), size, &why);
	if (!view.format_header)
	{
		fprintf(stderr, "%s\n", why.c_str());
		return 5;
	}
	const RuntimeStyle style = atoi(argv[2]) ? RuntimeStyle::Meshlet : RuntimeStyle::MDI;
	const std::vector<Offsets> offsets = build_decode_offsets(view, style, DecodeModeFlags(atoi(argv[3])));
	const std::vector<uint8_t> records = build_indirect_records(view, style, uint32_t(atoi(argv[4])), uint32_t(atoi(argv[5])));
	if (records.size() != view.num_bounds_256 * indirect_stride(style))
		return 4;
	f = fopen(argv[6], "wb");
	if (!f)
		return 3;
	if (!offsets.empty() && fwrite(offsets.data(), sizeof(Offsets), offsets.size(), f) != offsets.size())
		return 3;
	if (!records.empty() && fwrite(records.data(), 1, records.size(), f) != records.size())
		return 3;
	return fclose(f) == 0 ? 0 : 3;
}
