// TEST INFRASTRUCTURE ONLY -- used by make_bc_decode_golden.py to record tests/golden/bc_decode_shader_v1.npz.
//
// Runs the reference's decode/{s3tc,rgtc,bc7,bc6}.comp on the CPU: the shaders are re-spelled into gen/ by oracle/ref_build/glsl2cpp.py
// at generation time (a temporary directory, removed afterwards) and compiled as C++ against oracle/ref_build/glsl_cpu.hpp.  This file
// supplies what that header lacks: the block payload as a utexture2D read with texelFetch (R32G32_UINT for 8-byte blocks,
// R32G32B32A32_UINT for 16-byte ones, as compressed_format_to_payload_format binds it), a uimage2D stored as RGBA8UI / RGBA16UI, and the
// integer built-ins the shaders use.  Every object built from this file holds one shader with one set of specialisation constants
// (-DBC_SHADER=0..3 with -DSPEC_...) and registers it; the object built with -DBC_ENTRY holds the registry and the entry point.
//
// One invocation per texel in 4 x 4 x 4 groups of 8 x 8 texels, edge groups included, as dispatch_kernel_* launches them.
#include <vector>
#include "glsl_cpu.hpp"

namespace bc
{
struct Call
{
	const uint32_t *blocks; // blocks_x * blocks_y * words
	int words, blocks_x, blocks_y;
	void *out;
	int width, height;
	int out_kind; // 0 RGBA8 UNORM (float store), 1 R8, 2 RG8, 3 RGBA8UI, 4 RGBA16UI
};
struct Variant
{
	int shader, spec0, spec1;
	void (*run)(const Call &call);
};
std::vector<Variant> &registry();
} // namespace bc

#ifndef BC_ENTRY
namespace glsl
{
struct utexture2D
{
	const uint32_t *data = nullptr;
	int words = 4, w = 0, h = 0;
};
inline uvec4 texelFetch(const utexture2D &t, const ivec2 &p, int)
{
	const int x = orc::clampi(p.x, 0, t.w - 1), y = orc::clampi(p.y, 0, t.h - 1);
	const uint32_t *b = t.data + (size_t(y) * t.w + x) * t.words;
	return t.words == 4 ? uvec4(b[0], b[1], b[2], b[3]) : uvec4(b[0], b[1], 0u, 1u);
}
struct uimage2D
{
	void *data = nullptr;
	int w = 0, h = 0, bits = 8;
};
inline void imageStore(uimage2D &img, const ivec2 &p, const uvec4 &v)
{
	if (p.x < 0 || p.y < 0 || p.x >= img.w || p.y >= img.h)
		return;
	const size_t i = (size_t(p.y) * img.w + p.x) * 4;
	const uint c[4] = {v.x, v.y, v.z, v.w};
	for (int k = 0; k < 4; k++)
		if (img.bits == 8)
			static_cast<uint8_t *>(img.data)[i + k] = uint8_t(c[k]);
		else
			static_cast<uint16_t *>(img.data)[i + k] = uint16_t(c[k]);
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
inline ivec3 bitfieldExtract(const ivec3 &v, int offset, int bits)
{
	return ivec3(bitfieldExtract(v.x, offset, bits), bitfieldExtract(v.y, offset, bits), bitfieldExtract(v.z, offset, bits));
}
inline uvec3 bitfieldExtract(const uvec3 &v, int offset, int bits)
{
	return uvec3(bitfieldExtract(v.x, offset, bits), bitfieldExtract(v.y, offset, bits), bitfieldExtract(v.z, offset, bits));
}
inline ivec3 mix(const ivec3 &a, const ivec3 &b, const bvec3 &pick_b) { return ivec3(pick_b.x ? b.x : a.x, pick_b.y ? b.y : a.y, pick_b.z ? b.z : a.z); }
inline ivec3 operator|(int a, const ivec3 &b) { return ivec3(a | b.x, a | b.y, a | b.z); }
template <typename T> inline tvec3<T> &operator&=(tvec3<T> &a, const tvec3<T> &b)
{
	a = tvec3<T>(a.x & b.x, a.y & b.y, a.z & b.z);
	return a;
}

namespace
{
namespace shader
{
static constexpr struct
{
	unsigned x = 4, y = 4, z = 4;
} gl_WorkGroupSize;
#if BC_SHADER == 0
#include "gen/s3tc.inc"
#elif BC_SHADER == 1
#include "gen/rgtc.inc"
#elif BC_SHADER == 2
#include "gen/bc7.inc"
#else
#include "gen/bc6.inc"
#endif
} // namespace shader
} // namespace
} // namespace glsl

namespace bc
{
namespace
{
void run(const Call &call)
{
	using namespace glsl;
	namespace s = glsl::shader;
	s::uInput.data = call.blocks;
	s::uInput.words = call.words;
	s::uInput.w = call.blocks_x;
	s::uInput.h = call.blocks_y;
	s::uOutput.data = call.out;
	s::uOutput.w = call.width;
	s::uOutput.h = call.height;
#if BC_SHADER < 2
	s::uOutput.format = call.out_kind == 1 ? Format::R8_UNORM : call.out_kind == 2 ? Format::RG8_UNORM : Format::RGBA8_UNORM;
#else
	s::uOutput.bits = call.out_kind == 4 ? 16 : 8;
#endif
	s::registers.resolution = ivec2(call.width, call.height);
	for (unsigned gy = 0; gy < unsigned(call.height + 7) / 8; gy++)
		for (unsigned gx = 0; gx < unsigned(call.width + 7) / 8; gx++)
			for (unsigned lz = 0; lz < 4; lz++)
				for (unsigned ly = 0; ly < 4; ly++)
					for (unsigned lx = 0; lx < 4; lx++)
					{
						gl_WorkGroupID = uvec3(gx, gy, 0u);
						gl_LocalInvocationID = uvec3(lx, ly, lz);
						gl_LocalInvocationIndex = (lz * 4 + ly) * 4 + lx;
						gl_GlobalInvocationID = uvec3(gx * 4 + lx, gy * 4 + ly, lz);
						s::main();
					}
}
const bool registered = (registry().push_back({BC_SHADER, BC_SPEC0, BC_SPEC1, run}), true);
} // namespace
} // namespace bc

#else // BC_ENTRY
namespace bc
{
std::vector<Variant> &registry()
{
	static std::vector<Variant> variants;
	return variants;
}
} // namespace bc

// One dispatch.  shader: 0 s3tc (spec0 = USE_ALPHA, spec1 = BC_VERSION), 1 rgtc (spec0 = DUAL_COMPONENT), 2 bc7, 3 bc6 (spec0 = SIGNED).
// blocks: tightly packed, block_bytes each; out: width x height texels, tightly packed (RGBA8, R8, RG8 or RGBA16 by shader and spec).
// Returns -1 when this set of specialisation constants was not built.
extern "C" int ref_bc_decode(int shader, int spec0, int spec1, const void *blocks, int block_bytes, int width, int height, void *out)
{
	for (const auto &v : bc::registry())
		if (v.shader == shader && v.spec0 == spec0 && v.spec1 == spec1)
		{
			bc::Call call = {};
			call.blocks = static_cast<const uint32_t *>(blocks);
			call.words = block_bytes / 4;
			call.blocks_x = (width + 3) / 4;
			call.blocks_y = (height + 3) / 4;
			call.out = out;
			call.width = width;
			call.height = height;
			call.out_kind = shader == 0 ? 0 : shader == 1 ? (spec0 ? 2 : 1) : shader == 2 ? 3 : 4;
			v.run(call);
			return 0;
		}
	return -1;
}
#endif
