// TEST INFRASTRUCTURE ONLY -- used by make_astc_decode_golden.py to record tests/golden/astc_decode_shader_v1.npz.
//
// Runs the reference's decode/astc.comp on the CPU: the shader (with bitextract.h expanded into it) is re-spelled into gen/astc.inc by
// oracle/ref_build/glsl2cpp.py at generation time (a temporary directory, removed afterwards) and compiled as C++ against
// oracle/ref_build/glsl_cpu.hpp with -DSPEC_DECODE_8BIT=true.  This file supplies what that header lacks: the six lookup tables as
// texel buffers and a texture, the block payload as an RGBA32UI texture, a uimage2D stored as RGBA8UI, the push constants, the
// local_size_x_id / local_size_y_id workgroup shape as a variable, and the integer built-ins the shader uses.  The tables come from the
// reference's own builders: the generator cuts them out of vulkan/texture/texture_decoder.cpp into gen/astc_tables.inc, next to the
// shader, and nothing of either is kept.
//
// One invocation per texel in groups of footprint x 4 (2 x 2 blocks), edge groups included, with the LDR error colour, as
// dispatch_kernel_astc(..., HDR = false) launches them.
#include <cassert>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "glsl_cpu.hpp"

namespace ref_tables
{
#include "gen/astc_tables.inc"
} // namespace ref_tables

namespace glsl
{
struct utextureBuffer
{
	const void *data = nullptr;
	int texels = 0, components = 1, bytes = 1; // components per texel, bytes per component (1 or 2)
};
inline uvec4 texelFetch(const utextureBuffer &t, int i)
{
	uint c[4] = {0u, 0u, 0u, 1u};
	if (i < 0 || i >= t.texels)
		return uvec4(0u, 0u, 0u, 0u); // a robust buffer read
	for (int k = 0; k < t.components; k++)
		c[k] = t.bytes == 2 ? static_cast<const uint16_t *>(t.data)[i * t.components + k] : static_cast<const uint8_t *>(t.data)[i * t.components + k];
	return uvec4(c[0], c[1], c[2], c[3]);
}
struct utexture2D
{
	const void *data = nullptr;
	int words = 4, w = 0, h = 0; // 4: R32G32B32A32_UINT; 0: R8_UINT
};
inline uvec4 texelFetch(const utexture2D &t, const ivec2 &p, int)
{
	const int x = orc::clampi(p.x, 0, t.w - 1), y = orc::clampi(p.y, 0, t.h - 1);
	if (t.words == 0)
		return uvec4(static_cast<const uint8_t *>(t.data)[size_t(y) * t.w + x], 0u, 0u, 1u);
	const uint32_t *b = static_cast<const uint32_t *>(t.data) + (size_t(y) * t.w + x) * 4;
	return uvec4(b[0], b[1], b[2], b[3]);
}
struct uimage2D
{
	uint8_t *data = nullptr;
	int w = 0, h = 0;
};
inline void imageStore(uimage2D &img, const ivec2 &p, const uvec4 &v)
{
	if (p.x < 0 || p.y < 0 || p.x >= img.w || p.y >= img.h)
		return;
	uint8_t *dst = img.data + (size_t(p.y) * img.w + p.x) * 4;
	dst[0] = uint8_t(v.x);
	dst[1] = uint8_t(v.y);
	dst[2] = uint8_t(v.z);
	dst[3] = uint8_t(v.w);
}
inline uint bitfieldReverse(uint v)
{
	uint r = 0;
	for (int i = 0; i < 32; i++)
		r |= ((v >> i) & 1u) << (31 - i);
	return r;
}
// the signed form sign-extends from the field's top bit
inline int bitfieldExtract(int v, int offset, int bits)
{
	if (bits == 0)
		return 0;
	const uint field = bitfieldExtract(uint(v), offset, bits);
	return bits == 32 ? int(field) : int(field << (32 - bits)) >> (32 - bits);
}
inline uvec4 bitfieldReverse(const uvec4 &v) { return uvec4(bitfieldReverse(v.x), bitfieldReverse(v.y), bitfieldReverse(v.z), bitfieldReverse(v.w)); }
inline ivec4 &operator<<=(ivec4 &a, int s)
{
	a = a << s;
	return a;
}
template <int N, int A, int B, int C> inline swz3<int, N, A, B, C, true> &operator<<=(swz3<int, N, A, B, C, true> &a, int s)
{
	a = ivec3(a) << s;
	return a;
}
inline uvec4 operator--(uvec4 &a, int)
{
	const uvec4 before = a;
	a = uvec4(a.x - 1u, a.y - 1u, a.z - 1u, a.w - 1u);
	return before;
}
inline uvec4 &operator&=(uvec4 &a, const uvec4 &b)
{
	a = a & b;
	return a;
}

namespace
{
namespace shader
{
static uvec3 gl_WorkGroupSize(4u, 4u, 4u);
#include "gen/astc.inc"
} // namespace shader
} // namespace
} // namespace glsl

extern "C" int ref_astc_table_sizes(int *endpoint_unquant, int *weight_unquant)
{
	auto &luts = ref_tables::get_astc_luts();
	*endpoint_unquant = int(luts.color_endpoint.unquant_offset);
	*weight_unquant = int(luts.weights.unquant_offset);
	return 0;
}

// endpoint_quantiser: u16[9][128][4]; endpoint_unquant / weight_unquant: as many bytes as ref_astc_table_sizes says; weight_quantiser:
// u8[16][4]; trits_quints: u16[384].
extern "C" void ref_astc_tables(uint16_t *endpoint_quantiser, uint8_t *endpoint_unquant, uint8_t *weight_quantiser, uint8_t *weight_unquant, uint16_t *trits_quints)
{
	auto &luts = ref_tables::get_astc_luts();
	memcpy(endpoint_quantiser, luts.color_endpoint.lut, sizeof(luts.color_endpoint.lut));
	memcpy(endpoint_unquant, luts.color_endpoint.unquant_lut, luts.color_endpoint.unquant_offset);
	memcpy(weight_quantiser, luts.weights.lut, sizeof(luts.weights.lut));
	memcpy(weight_unquant, luts.weights.unquant_lut, luts.weights.unquant_offset);
	memcpy(trits_quints, luts.integer.trits_quints, sizeof(luts.integer.trits_quints));
}

// u8[32 * bh][32 * bw]
extern "C" void ref_astc_partition_table(int bw, int bh, uint8_t *out)
{
	auto &t = ref_tables::get_astc_luts().get_partition_table(unsigned(bw), unsigned(bh));
	memcpy(out, t.lut_buffer.data(), t.lut_buffer.size());
}

// One dispatch.  blocks: tightly packed, 16 bytes each, ceil(width / bw) to a row; out: width x height RGBA8, tightly packed.
extern "C" int ref_astc_decode(const void *blocks, int bw, int bh, int width, int height, void *out)
{
	using namespace glsl;
	namespace s = glsl::shader;
	auto &luts = ref_tables::get_astc_luts();
	auto &partition = luts.get_partition_table(unsigned(bw), unsigned(bh));
	s::LUTRemainingBitsToEndpointQuantizer = {luts.color_endpoint.lut, 9 * 128, 4, 2};
	s::LUTEndpointUnquantize = {luts.color_endpoint.unquant_lut, int(luts.color_endpoint.unquant_offset), 1, 1};
	s::LUTWeightQuantizer = {luts.weights.lut, 16, 4, 1};
	s::LUTWeightUnquantize = {luts.weights.unquant_lut, int(luts.weights.unquant_offset), 1, 1};
	s::LUTTritQuintDecode = {luts.integer.trits_quints, 256 + 128, 1, 2};
	s::LUTPartitionTable = {partition.lut_buffer.data(), 0, int(partition.lut_width), int(partition.lut_height)};
	const int blocks_x = (width + bw - 1) / bw, blocks_y = (height + bh - 1) / bh;
	s::PayloadInput = {blocks, 4, blocks_x, blocks_y};
	s::OutputImage = {static_cast<uint8_t *>(out), width, height};
	s::registers.error_color = uvec4(0xffu, 0u, 0xffu, 0xffu);
	s::registers.resolution = ivec2(width, height);
	s::gl_WorkGroupSize = uvec3(unsigned(bw), unsigned(bh), 4u);
	for (unsigned gy = 0; gy < unsigned(blocks_y + 1) / 2; gy++)
		for (unsigned gx = 0; gx < unsigned(blocks_x + 1) / 2; gx++)
			for (unsigned lz = 0; lz < 4; lz++)
				for (unsigned ly = 0; ly < unsigned(bh); ly++)
					for (unsigned lx = 0; lx < unsigned(bw); lx++)
					{
						gl_WorkGroupID = uvec3(gx, gy, 0u);
						gl_LocalInvocationID = uvec3(lx, ly, lz);
						gl_LocalInvocationIndex = (lz * bh + ly) * bw + lx;
						gl_GlobalInvocationID = uvec3(gx * bw + lx, gy * bh + ly, lz);
						s::decode_error = false; // a global of the shader: every invocation starts with its initialiser
						s::main();
					}
	return 0;
}
