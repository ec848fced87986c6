// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// MESHLET4 payload decode: what assets/shaders/decode/meshlet_decode.comp computes per lane with inc/meshlet_payload_decode.h and
// inc/meshlet_attribute_decode.h.  Plain functions: meshlet.hip calls them from its kernel, tests/cpp/meshlet_decode_host.cpp builds the
// same text for the host, where tests/test_meshlet_host_cpu.py holds it to the executed shader's outputs
// (tests/golden/meshlet_decode_shader_v1.npz) before a device sees it.
//
// The window.  Element i of a stream with `bits` bits and C components starts at bit i * bits * C of the stream's words and is read
// through the 64 bits of two consecutive words; component k is the window shifted right by (start & 31) + k * bits, truncated to 32 bits
// and masked to `bits` bits.  With 13 .. 15 bits and three components the last component can start past bit 63 - bits: it then loses
// its high bits, here as in the shader, since it is the same arithmetic.  Three rules the shader leaves to its environment:
//   - bits == 0 is a constant stream and gives 0 (GLSL's bitfieldExtract(v, 0, 0)), never a shift by 32;
//   - a word index at or past payload_words reads as 0.  The shader's second word of the last element can be word payload_words: its
//     file has one padding word there, a linear buffer has not.  Any other index past the end is malformed data, and also reads 0;
//   - a shift of 64 or more (bits above what create_mesh_view admits) gives 0.
// Truncation to 16 and 8 bits wraps, as i16vec3(value) and u8vec4(value) do.
//
// Floating point: every operation here is one IEEE fp32 operation, in the order oracle/ref_build/glsl_cpu.hpp states: x / 127.0,
// normalize(a) = a / sqrt(a.x * a.x + a.y * a.y + a.z * a.z) summed left to right, round() half away from zero.  Build without
// contraction and with correctly rounded division and square root.  Positions and UV are exact by construction (an int16, a power of two).
// Bone weights: unpackUnorm4x8 then packUnorm4x8 is the identity on every byte (tests/test_meshlet_ref_cpu.py shows all 256), so the
// four bytes are copied.
#pragma once
#include <cmath>
#include <cstdint>
#include "core_base.hpp"

namespace gr_meshlet
{
constexpr uint32_t MAX_ELEMENTS = 32;
constexpr uint32_t CHUNK_FACTOR = 8;
enum StreamType : uint32_t
{
	STREAM_PRIMITIVE = 0,
	STREAM_POSITION,
	STREAM_NORMAL_TANGENT_OCT8,
	STREAM_UV,
	STREAM_BONE_INDICES,
	STREAM_BONE_WEIGHTS
};

struct Stream // Meshlet::Stream; stream 0 of a meshlet holds {prim_count, vert_count} in base
{
	uint32_t base[2];
	uint32_t bits;
	uint32_t offset_in_words;
};
struct Offsets
{
	uint32_t primitive_output_offset, vertex_output_offset, index_offset;
};
struct Payload
{
	const uint32_t *words;
	uint32_t count;
};
struct TexturedAttr
{
	uint32_t normal, tangent;
	float uv[2];
};
static_assert(sizeof(Stream) == 16 && sizeof(Offsets) == 12 && sizeof(TexturedAttr) == 16, "records are the shader's");

GR_HD uint32_t payload_word(const Payload &p, uint32_t index) { return index < p.count ? p.words[index] : 0u; }

// the 64-bit window of element `index` of a stream of `components` x `bits`, and the bit at which the element starts in it
GR_HD uint64_t window(const Payload &p, uint32_t offset_in_words, uint32_t index, uint32_t bits, uint32_t components, uint32_t &start_bit)
{
	const uint32_t first_bit = index * bits * components;
	const uint32_t start_word = offset_in_words + first_bit / 32u; // wraps as the shader's uint does; the bound check follows
	start_bit = first_bit & 31u;
	const uint32_t word0 = payload_word(p, start_word), word1 = payload_word(p, start_word + 1u);
	return uint64_t(word0) | (uint64_t(word1) << 32);
}
GR_HD uint32_t field(uint64_t word, uint32_t shift, uint32_t bits)
{
	const uint32_t v = shift < 64u ? uint32_t(word >> shift) : 0u;
	return bits == 0u ? 0u : (bits >= 32u ? v : v & ((1u << bits) - 1u));
}
GR_HD void decode2(const Payload &p, uint32_t offset_in_words, uint32_t index, uint32_t bits, uint32_t v[2])
{
	uint32_t start;
	const uint64_t word = window(p, offset_in_words, index, bits, 2u, start);
	v[0] = field(word, start, bits);
	v[1] = field(word, start + bits, bits);
}
GR_HD void decode3(const Payload &p, uint32_t offset_in_words, uint32_t index, uint32_t bits, uint32_t v[3])
{
	uint32_t start;
	const uint64_t word = window(p, offset_in_words, index, bits, 3u, start);
	v[0] = field(word, start, bits);
	v[1] = field(word, start + bits, bits);
	v[2] = field(word, start + 2u * bits, bits);
}
GR_HD void decode4(const Payload &p, uint32_t offset_in_words, uint32_t index, uint32_t bits, uint32_t v[4])
{
	uint32_t start;
	const uint64_t word = window(p, offset_in_words, index, bits, 4u, start);
	v[0] = field(word, start, bits);
	v[1] = field(word, start + bits, bits);
	v[2] = field(word, start + 2u * bits, bits);
	v[3] = field(word, start + 3u * bits, bits);
}

// ---- the six stream decoders ----------------------------------------------------------------------------------------------------------
GR_HD void decode_index_buffer(const Payload &p, const Stream &s, uint32_t lane, uint32_t v[3]) { decode3(p, s.offset_in_words, lane, 5u, v); }

GR_HD void decode_snorm_scaled_i16x3(const Payload &p, const Stream &s, uint32_t lane, int16_t v[3], int &exponent)
{
	exponent = int32_t(s.bits) >> 16;
	uint32_t value[3];
	decode3(p, s.offset_in_words, lane, s.bits & 0xffu, value);
	v[0] = int16_t(uint16_t(value[0] + (s.base[0] & 0xffffu)));
	v[1] = int16_t(uint16_t(value[1] + (s.base[0] >> 16)));
	v[2] = int16_t(uint16_t(value[2] + (s.base[1] & 0xffffu)));
}
GR_HD void decode_snorm_scaled_i16x2(const Payload &p, const Stream &s, uint32_t lane, int16_t v[2], int &exponent)
{
	exponent = int32_t(s.bits) >> 16;
	uint32_t value[2];
	decode2(p, s.offset_in_words, lane, s.bits & 0xffu, value);
	v[0] = int16_t(uint16_t(value[0] + (s.base[0] & 0xffffu)));
	v[1] = int16_t(uint16_t(value[1] + (s.base[0] >> 16)));
}
// base + delta of a four-byte stream, each component still 32 bits wide
GR_HD void decode_bytes4(const Payload &p, const Stream &s, uint32_t lane, uint32_t v[4])
{
	decode4(p, s.offset_in_words, lane, s.bits & 0xffu, v);
	for (int i = 0; i < 4; i++)
		v[i] += (s.base[0] >> (8 * i)) & 0xffu;
}
GR_HD uint32_t pack_bytes4(const uint32_t v[4]) { return (v[0] & 0xffu) | ((v[1] & 0xffu) << 8) | ((v[2] & 0xffu) << 16) | ((v[3] & 0xffu) << 24); }
// the four bytes nx, ny, tx, ty as one word, and the tangent's sign: aux 3 takes it from the low bit of ty, aux 2 is negative, else positive
GR_HD uint32_t decode_normal_tangent_oct8(const Payload &p, const Stream &s, uint32_t lane, bool &t_sign)
{
	uint32_t v[4];
	decode_bytes4(p, s, lane, v);
	const uint32_t aux = s.bits >> 16;
	if (aux == 3u)
	{
		t_sign = (v[3] & 1u) != 0u;
		v[3] &= ~1u;
	}
	else
		t_sign = aux == 2u;
	return pack_bytes4(v);
}
GR_HD uint32_t decode_bone_indices(const Payload &p, const Stream &s, uint32_t lane)
{
	uint32_t v[4];
	decode_bytes4(p, s, lane, v);
	return pack_bytes4(v);
}
GR_HD uint32_t decode_bone_weights(const Payload &p, const Stream &s, uint32_t lane) { return decode_bone_indices(p, s, lane); }

// ---- attributes -----------------------------------------------------------------------------------------------------------------------
GR_HD float snorm_exp_position(int16_t v, int exponent) { return ldexpf(float(v), exponent); }
GR_HD float snorm_exp_uv(int16_t v, int exponent) { return 0.5f * ldexpf(float(v), exponent) + 0.5f; }

GR_HD void oct_normal(float fx, float fy, float n[3])
{
	n[0] = fx;
	n[1] = fy;
	n[2] = 1.0f - fabsf(fx) - fabsf(fy);
	const float t = fmaxf(-n[2], 0.0f);
	n[0] += n[0] >= 0.0f ? -t : t;
	n[1] += n[1] >= 0.0f ? -t : t;
	const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
	n[0] /= len;
	n[1] /= len;
	n[2] /= len;
}
GR_HD uint32_t quantize_snorm(float v, float scale, uint32_t mask) { return uint32_t(int32_t(roundf(fminf(fmaxf(v, -1.0f), 1.0f) * scale))) & mask; }
GR_HD uint32_t pack_a2bgr10(float x, float y, float z, float w)
{
	return (quantize_snorm(w, 1.0f, 3u) << 30) | (quantize_snorm(z, 511.0f, 1023u) << 20) | (quantize_snorm(y, 511.0f, 1023u) << 10) | quantize_snorm(x, 511.0f, 1023u);
}
// nt: the word of decode_normal_tangent_oct8.  normal.w is 0, tangent.w is -1 for t_sign and 1 otherwise.
GR_HD void oct8_normal_tangent(uint32_t nt, bool t_sign, uint32_t &normal, uint32_t &tangent)
{
	float f[4], n[3], t[3];
	for (int i = 0; i < 4; i++)
		f[i] = float(int8_t(uint8_t(nt >> (8 * i)))) / 127.0f;
	oct_normal(f[0], f[1], n);
	oct_normal(f[2], f[3], t);
	normal = pack_a2bgr10(n[0], n[1], n[2], 0.0f);
	tangent = pack_a2bgr10(t[0], t[1], t[2], t_sign ? -1.0f : 1.0f);
}

// ---- one lane of one meshlet ----------------------------------------------------------------------------------------------------------
// Everything a lane reads and writes.  Capacities are in elements; a lane whose element lies at or past its capacity stores nothing,
// counts above 32 are clamped and payload reads are bounded (payload_word): device data the host did not vouch for gives wrong values,
// never an access outside these buffers.
struct DecodeArgs
{
	const Stream *streams; // meshlet_count * stream_count, 16-byte aligned
	Payload payload;
	const Offsets *offsets; // meshlet_count
	uint8_t *indices;       // INDEX_BYTES * 3 bytes per primitive, any alignment
	float *positions;       // 3 floats per vertex
	TexturedAttr *attributes;
	uint32_t *skin; // 2 words per vertex
	uint64_t index_capacity, position_capacity, attribute_capacity, skin_capacity;
	uint32_t primitive_offset, vertex_offset, meshlet_count, wg_offset;
	uint32_t stream_count, target_style;
};

GR_HD Stream load_stream(const Stream *s)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const uint4 v = *reinterpret_cast<const uint4 *>(s); // one 16-byte load, the same address in all 32 lanes of a meshlet
	return Stream{{v.x, v.y}, v.z, v.w};
#else
	return *s;
#endif
}
template <typename T> GR_HD void store_aligned(uint8_t *at, T v) { __builtin_memcpy(__builtin_assume_aligned(at, sizeof(T)), &v, sizeof(T)); }

// INDEX_BYTES: 4 (unrolled mesh), 2 (INDEX16) or 1.  ALIGNED: `indices` is a multiple of INDEX_BYTES; otherwise bytes are stored one by one.
template <int INDEX_BYTES, bool ALIGNED> GR_HD void store_index(uint8_t *at, uint32_t v)
{
	if (INDEX_BYTES == 1)
		at[0] = uint8_t(v);
	else if (ALIGNED && INDEX_BYTES == 2)
		store_aligned(at, uint16_t(v));
	else if (ALIGNED)
		store_aligned(at, v);
	else
		for (int i = 0; i < INDEX_BYTES; i++)
			at[i] = uint8_t(v >> (8 * i));
}

template <int INDEX_BYTES, bool ALIGNED> GR_HD void decode_lane(const DecodeArgs &a, uint32_t meshlet, uint32_t lane)
{
	if (meshlet >= a.meshlet_count || lane >= MAX_ELEMENTS)
		return;
	const Stream *streams = a.streams + size_t(meshlet) * a.stream_count;
	const Offsets offsets = a.offsets[meshlet];
	const Stream counts = load_stream(streams + STREAM_PRIMITIVE);
	const uint32_t primitive_count = counts.base[0] < MAX_ELEMENTS ? counts.base[0] : MAX_ELEMENTS;
	const uint32_t vertex_count = counts.base[1] < MAX_ELEMENTS ? counts.base[1] : MAX_ELEMENTS;

	if (lane < primitive_count)
	{
		uint32_t v[3];
		decode_index_buffer(a.payload, counts, lane, v);
		const uint32_t element = offsets.primitive_output_offset + a.primitive_offset + lane;
		if (element < a.index_capacity)
			for (int i = 0; i < 3; i++)
				store_index<INDEX_BYTES, ALIGNED>(a.indices + (size_t(element) * 3u + i) * INDEX_BYTES, v[i] + offsets.index_offset);
	}
	if (lane >= vertex_count)
		return;
	const uint32_t element = offsets.vertex_output_offset + a.vertex_offset + lane;
	{
		int16_t v[3];
		int exponent;
		decode_snorm_scaled_i16x3(a.payload, load_stream(streams + STREAM_POSITION), lane, v, exponent);
		if (element < a.position_capacity)
			for (int i = 0; i < 3; i++)
				a.positions[size_t(element) * 3u + i] = snorm_exp_position(v[i], exponent);
	}
	if (a.target_style >= 1u)
	{
		bool t_sign;
		const uint32_t nt = decode_normal_tangent_oct8(a.payload, load_stream(streams + STREAM_NORMAL_TANGENT_OCT8), lane, t_sign);
		int16_t uv[2];
		int exponent;
		decode_snorm_scaled_i16x2(a.payload, load_stream(streams + STREAM_UV), lane, uv, exponent);
		TexturedAttr attr;
		oct8_normal_tangent(nt, t_sign, attr.normal, attr.tangent);
		attr.uv[0] = snorm_exp_uv(uv[0], exponent);
		attr.uv[1] = snorm_exp_uv(uv[1], exponent);
		if (element < a.attribute_capacity)
			a.attributes[element] = attr;
	}
	if (a.target_style >= 2u)
	{
		const uint32_t indices = decode_bone_indices(a.payload, load_stream(streams + STREAM_BONE_INDICES), lane);
		const uint32_t weights = decode_bone_weights(a.payload, load_stream(streams + STREAM_BONE_WEIGHTS), lane);
		if (element < a.skin_capacity)
		{
			a.skin[size_t(element) * 2u] = indices;
			a.skin[size_t(element) * 2u + 1u] = weights;
		}
	}
}
} // namespace gr_meshlet
