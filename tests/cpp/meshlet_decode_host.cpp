// TEST INFRASTRUCTURE.  granite_amd/csrc/meshlet_decode.hpp -- the mesh decode the device kernel of meshlet.hip calls -- built for the
// host.  tests/test_meshlet_host_cpu.py holds it to the golden of the executed shader (tests/golden/meshlet_decode_shader_v1.npz) and, on
// malformed headers, to tests/meshlet_ref.py, plain and under -fsanitize=address,undefined.
//   meshlet_decode_host in.bin out.bin [index_base_offset]
// in.bin: nine uint32 {meshlet_count, stream_count, payload_words, target_style, flags, primitive_offset, vertex_offset,
// primitive_capacity, vertex_capacity}, then the Stream records, the payload words and the Offsets records.  Every array is allocated at
// exactly its size -- the payload at payload_words words with no padding word -- so that the sanitizer sees any access outside it.  The
// outputs start filled with 0xcd; out.bin is indices, positions, attributes, skin, one after the other.  Lanes are walked as the kernel
// launches them: whole groups of eight meshlets of 32 lanes, the lanes past meshlet_count included.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../../granite_amd/csrc/meshlet_decode.hpp"

template <typename T> static std::unique_ptr<T[]> read_array(FILE *f, size_t count)
{
	std::unique_ptr<T[]> data(new T[count]); // exactly `count` elements
	if (count && fread(data.get(), sizeof(T), count, f) != count)
		exit(3);
	return data;
}

template <int INDEX_BYTES> static void run(const gr_meshlet::DecodeArgs &a, bool aligned)
{
	const uint32_t groups = (a.meshlet_count + 7u) / 8u;
	for (uint32_t group = a.wg_offset; group < groups; group++)
		for (uint32_t thread = 0; thread < 256u; thread++)
		{
			if (aligned)
				gr_meshlet::decode_lane<INDEX_BYTES, true>(a, 8u * group + (thread >> 5), thread & 31u);
			else
				gr_meshlet::decode_lane<INDEX_BYTES, false>(a, 8u * group + (thread >> 5), thread & 31u);
		}
}

int main(int argc, char **argv)
{
	if (argc != 3 && argc != 4)
		return 2;
	const size_t base_offset = argc == 4 ? size_t(atoi(argv[3])) : 0;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 3;
	uint32_t h[9];
	if (fread(h, 4, 9, f) != 9)
		return 3;
	const uint32_t meshlets = h[0], stream_count = h[1], payload_words = h[2], flags = h[4];
	auto streams = read_array<gr_meshlet::Stream>(f, size_t(meshlets) * stream_count);
	auto payload = read_array<uint32_t>(f, payload_words);
	auto offsets = read_array<gr_meshlet::Offsets>(f, meshlets);
	fclose(f);

	const int index_bytes = (flags & 1u) ? 4 : ((flags & 2u) ? 2 : 1);
	const size_t prim_cap = h[7], vert_cap = h[8];
	const size_t sizes[4] = {prim_cap * 3 * index_bytes, vert_cap * 12, vert_cap * 16, vert_cap * 8};
	std::unique_ptr<uint8_t[]> index_storage(new uint8_t[sizes[0] + base_offset]);
	std::unique_ptr<float[]> positions(new float[vert_cap * 3]);
	std::unique_ptr<gr_meshlet::TexturedAttr[]> attributes(new gr_meshlet::TexturedAttr[vert_cap]);
	std::unique_ptr<uint32_t[]> skin(new uint32_t[vert_cap * 2]);
	memset(index_storage.get(), 0xcd, sizes[0] + base_offset);
	memset(positions.get(), 0xcd, sizes[1]);
	memset(attributes.get(), 0xcd, sizes[2]);
	memset(skin.get(), 0xcd, sizes[3]);

	gr_meshlet::DecodeArgs a = {};
	a.streams = streams.get();
	a.payload = {payload.get(), payload_words};
	a.offsets = offsets.get();
	a.indices = index_storage.get() + base_offset;
	a.positions = positions.get();
	a.attributes = attributes.get();
	a.skin = skin.get();
	a.index_capacity = prim_cap;
	a.position_capacity = a.attribute_capacity = a.skin_capacity = vert_cap;
	a.primitive_offset = h[5];
	a.vertex_offset = h[6];
	a.meshlet_count = meshlets;
	a.stream_count = stream_count;
	a.target_style = h[3];
	const bool aligned = (reinterpret_cast<uintptr_t>(a.indices) & uintptr_t(index_bytes - 1)) == 0;
	if (index_bytes == 4)
		run<4>(a, aligned);
	else if (index_bytes == 2)
		run<2>(a, aligned);
	else
		run<1>(a, true);
	for (size_t i = 0; i < base_offset; i++)
		if (index_storage[i] != 0xcd)
			return 4; // the bytes before an offset index buffer
	f = fopen(argv[2], "wb");
	if (!f)
		return 3;
	const void *outs[4] = {a.indices, positions.get(), attributes.get(), skin.get()};
	for (int i = 0; i < 4; i++)
		if (sizes[i] && fwrite(outs[i], 1, sizes[i], f) != sizes[i])
			return 3;
	return fclose(f) == 0 ? 0 : 3;
}
