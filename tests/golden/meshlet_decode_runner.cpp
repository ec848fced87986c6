// TEST INFRASTRUCTURE ONLY -- used by make_meshlet_golden.py to record tests/golden/meshlet_decode_shader_v1.npz.
//
// Runs the reference's decode/meshlet_decode.comp on the CPU, the way astc_decode_runner.cpp and ocean_lod_runner.cpp run theirs:
// re-spelled into gen/ by oracle/ref_build/glsl2cpp.py at generation time (a temporary directory, removed afterwards) and compiled as
// C++ against oracle/ref_build/glsl_cpu.hpp with -ffp-contract=off.  One object per specialisation set, one exported function each,
// named by -DMESHLET_FN; the set is -DSPEC_NUM_U32_STREAMS, -DSPEC_UNROLLED_MESH, -DSPEC_TARGET_MESH_STYLE, -DSPEC_INDEX16.
// What glsl_cpu.hpp lacks is supplied here, each as the GLSL specification (4.60, chapter 8) or its extension states it:
//   u8vec3, u8vec4, i8vec4        GL_EXT_shader_explicit_arithmetic_types_int8: conversion from uvec truncates (wraps) per component
//   pack32(u8vec4), unpack8(uint) the same extension: component 0 in the least significant byte
//   packUint2x32(uvec2)           first component in the least significant 32 bits
//   ldexp(vecN, ivecN)            x * 2^exp per component
//   unpackUnorm4x8 / packUnorm4x8 f / 255.0; round(clamp(c, 0, 1) * 255.0); component 0 in the least significant byte
//   bitfieldExtract on uvecN      per component, the scalar form of the header (0 for bits == 0)
//   mat2x4                        two columns of vec4
// The scalar-layout output blocks need u8vec3, u16vec3 and vec3 of 3, 6 and 12 bytes: asserted below.
// One invocation per lane of every 32 x 8 group, in order; gl_SubgroupSize stays at the header's 1, so the shader takes the
// gl_LocalInvocationID route (x the lane, y the meshlet of the group).
#include <cstddef>
#include <cstdint>
#include "glsl_cpu.hpp"

namespace glsl
{
using u8vec3 = tvec3<uint8_t>;
using u8vec4 = tvec4<uint8_t>;
using i8vec4 = tvec4<int8_t>;
static_assert(sizeof(u8vec3) == 3 && sizeof(u16vec3) == 6 && sizeof(vec3) == 12, "scalar block layout: tight element sizes");
static_assert(sizeof(uvec3) == 12 && sizeof(uvec2) == 8 && sizeof(vec2) == 8, "scalar block layout: tight element sizes");

inline uint pack32(const u8vec4 &v) { return uint(v.x) | (uint(v.y) << 8) | (uint(v.z) << 16) | (uint(v.w) << 24); }
inline u8vec4 unpack8(uint v) { return u8vec4(uint8_t(v), uint8_t(v >> 8), uint8_t(v >> 16), uint8_t(v >> 24)); }
inline uint64_t packUint2x32(const uvec2 &v) { return uint64_t(v.x) | (uint64_t(v.y) << 32); }
inline vec2 ldexp(const vec2 &v, const ivec2 &e) { return vec2(ldexpf(v.x, e.x), ldexpf(v.y, e.y)); }
inline vec3 ldexp(const vec3 &v, const ivec3 &e) { return vec3(ldexpf(v.x, e.x), ldexpf(v.y, e.y), ldexpf(v.z, e.z)); }
inline vec4 unpackUnorm4x8(uint v) { return vec4(float(v & 0xffu) / 255.0f, float((v >> 8) & 0xffu) / 255.0f, float((v >> 16) & 0xffu) / 255.0f, float(v >> 24) / 255.0f); }
inline uint packUnorm4x8(const vec4 &v)
{
	uint r = 0;
	for (int i = 0; i < 4; i++)
		r |= uint(roundf(fminf(fmaxf(v.d[i], 0.0f), 1.0f) * 255.0f)) << (8 * i);
	return r;
}
inline uvec2 bitfieldExtract(const uvec2 &v, int o, int b) { return uvec2(bitfieldExtract(v.x, o, b), bitfieldExtract(v.y, o, b)); }
inline uvec3 bitfieldExtract(const uvec3 &v, int o, int b) { return uvec3(bitfieldExtract(v.x, o, b), bitfieldExtract(v.y, o, b), bitfieldExtract(v.z, o, b)); }
inline uvec4 bitfieldExtract(const uvec4 &v, int o, int b)
{
	return uvec4(bitfieldExtract(v.x, o, b), bitfieldExtract(v.y, o, b), bitfieldExtract(v.z, o, b), bitfieldExtract(v.w, o, b));
}
struct mat2x4
{
	vec4 c[2];
	mat2x4(const vec4 &a, const vec4 &b) { c[0] = a; c[1] = b; }
	vec4 &operator[](int i) { return c[i]; }
};

namespace
{
namespace shader
{
#include "gen/meshlet_decode.inc"
} // namespace shader
} // namespace
} // namespace glsl

using namespace glsl;

// streams: meshlet_count * NUM_U32_STREAMS records of four dwords; payload: the words, followed by at least one readable zero word (the
// file's padding word, which the shader's last window reads); offsets: meshlet_count records of three dwords; push: the four dwords of
// the push block; groups: workgroups to run, gl_WorkGroupID.x = 0 .. groups - 1.
extern "C" void MESHLET_FN(const void *streams, const uint32_t *payload_words, const void *offsets, const uint32_t *push, void *indices, void *positions,
                           void *attributes, void *skin, uint32_t groups)
{
	namespace s = glsl::shader;
	static_assert(sizeof(s::MeshletStream) == 16 && sizeof(s::Offsets) == 12 && sizeof(s::TexturedAttr) == 16, "std430 records");
	s::meshlet_streams.data = static_cast<s::MeshletStream *>(const_cast<void *>(streams));
	s::payload.data = const_cast<uint32_t *>(payload_words);
	s::output_offsets.data = static_cast<s::Offsets *>(const_cast<void *>(offsets));
	s::output_indices32.data = static_cast<uvec3 *>(indices);
	s::output_indices16.data = static_cast<u16vec3 *>(indices);
	s::output_indices8.data = static_cast<u8vec3 *>(indices);
	s::output_stream_pos.data = static_cast<vec3 *>(positions);
	s::output_stream_textured_attr.data = static_cast<s::TexturedAttr *>(attributes);
	s::output_stream_skin.data = static_cast<uvec2 *>(skin);
	s::registers.primitive_offset = push[0];
	s::registers.vertex_offset = push[1];
	s::registers.meshlet_count = push[2];
	s::registers.wg_offset = push[3];
	for (uint32_t wg = 0; wg < groups; wg++)
		for (uint32_t y = 0; y < 8u; y++)
			for (uint32_t x = 0; x < 32u; x++)
			{
				gl_WorkGroupID = uvec3(wg, 0u, 0u);
				gl_LocalInvocationID = uvec3(x, y, 0u);
				s::main();
			}
}
