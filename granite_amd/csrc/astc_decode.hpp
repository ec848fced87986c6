// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// ASTC LDR block decode, 2-D footprints 4 x 4 ... 12 x 12: what assets/shaders/decode/astc.comp computes per texel with DECODE_8BIT = true
// (dispatch_kernel_astc(..., HDR = false)), split in two.  decode_block() runs once per block: block mode, void extent, partition count
// and hash coefficients, the CEM field(s), the endpoint quantiser from the bits that remain, the endpoint integers unpacked and
// unquantised into per-partition RGBA8 endpoints, and the whole weight grid unpacked from the bit-reversed stream and unquantised.
// decode_texel() takes that record and a texel inside the footprint: partition index, bilinear weight infill for one or two planes,
// interpolation, and the error rule.  Plain integer functions: texture_decode.hip calls them from its kernel, tests/cpp/astc_decode_host.cpp
// builds the same text for the host, where tests/test_astc_host_cpu.py holds it to the executed shader's outputs
// (tests/golden/astc_decode_shader_v1.npz) before a device sees it.
//
// Two places follow the shader and not the Khronos text.  (1) UNORM and SRGB alike expand an endpoint c to (c << 8) | 0x80, interpolate
// in 16 bits and store the top byte; with e0, e1 the 8-bit endpoints and w the weight that is exactly (e0 * (64 - w) + e1 * w + 32) >> 6,
// which is what decode_texel() computes.  (2) The error colour (0xff, 0, 0xff, 0xff) is stored per texel: a partition whose endpoint
// mode is an HDR one gives the error colour to its own texels only; the block's LDR partitions decode.  A void extent stores the top
// bytes of its four 16-bit values whether or not its HDR flag is set (the shader raises no error for the flag in 8-bit mode).
//
// The shader's six lookup tables are compile-time constants here, built from the same rules (texture_decoder.cpp:187-778): nothing is
// uploaded and no context state exists.  The partition index is the specification's hash computed per texel from eight coefficients
// and four offsets that decode_block() derives once.  The decoder is total: every shift and bit offset is bounded for any 16 bytes.
#pragma once
#include <cstdint>
#include "core_base.hpp"

namespace gr_astc
{
constexpr uint32_t ERROR_COLOUR = 0xffff00ffu; // R = 0xff, G = 0, B = 0xff, A = 0xff as the bytes of one little-endian word
constexpr int FOOTPRINT_COUNT = 14;

struct Footprint
{
	uint8_t w, h;
};
// In VkFormat order: format = 157 + 2 * index (+ 1 for SRGB).
constexpr Footprint footprint(int index)
{
	constexpr Footprint table[FOOTPRINT_COUNT] = {{4, 4}, {5, 4}, {5, 5}, {6, 5}, {6, 6}, {8, 5}, {8, 6}, {8, 8}, {10, 5}, {10, 6}, {10, 8}, {10, 10}, {12, 10}, {12, 12}};
	return table[index];
}

struct Quant
{
	uint8_t bits, trits, quints;
};

// ---- the tables -------------------------------------------------------------------------------------------------------------------

constexpr int ENDPOINT_MODES = 17, WEIGHT_MODES = 16;
constexpr int ENDPOINT_UNQUANT_SIZE = 1192, WEIGHT_UNQUANT_SIZE = 142;

// Endpoint quantisers from the finest down: the first that fits the remaining bits is the block's.
constexpr Quant endpoint_mode(int i)
{
	constexpr Quant table[ENDPOINT_MODES] = {{8, 0, 0}, {6, 1, 0}, {5, 0, 1}, {7, 0, 0}, {5, 1, 0}, {4, 0, 1}, {6, 0, 0}, {4, 1, 0}, {3, 0, 1},
	                                         {5, 0, 0}, {3, 1, 0}, {2, 0, 1}, {4, 0, 0}, {2, 1, 0}, {1, 0, 1}, {3, 0, 0}, {1, 1, 0}};
	return table[i];
}
// Weight quantisers by the block mode's 4-bit range index; 0, 1, 8 and 9 are reserved (no values).
constexpr Quant weight_mode(int i)
{
	constexpr Quant table[WEIGHT_MODES] = {{0, 0, 0}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {2, 0, 0}, {0, 0, 1}, {1, 1, 0}, {3, 0, 0},
	                                       {0, 0, 0}, {0, 0, 0}, {1, 0, 1}, {2, 1, 0}, {4, 0, 0}, {2, 0, 1}, {3, 1, 0}, {5, 0, 0}};
	return table[i];
}
constexpr int value_range(Quant q)
{
	const int r = (1 << q.bits) * (q.trits ? 3 : 1) * (q.quints ? 5 : 1);
	return r == 1 ? 0 : r;
}
// Bits of n values of a quantiser.
constexpr int sequence_bits(Quant q, int n) { return q.bits * n + (q.trits * 8 * n + 4) / 5 + (q.quints * 7 * n + 2) / 3; }

constexpr uint8_t unquant_endpoint(Quant q, int i)
{
	if (!q.trits && !q.quints)
	{
		switch (q.bits)
		{
		case 1: return uint8_t(i * 0xff);
		case 2: return uint8_t(i * 0x55);
		case 3: return uint8_t((i << 5) | (i << 2) | (i >> 1));
		case 4: return uint8_t(i * 0x11);
		case 5: return uint8_t((i << 3) | (i >> 2));
		case 6: return uint8_t((i << 2) | (i >> 4));
		case 7: return uint8_t((i << 1) | (i >> 6));
		default: return uint8_t(i);
		}
	}
	const int b = (i >> 1) & 1, c = (i >> 2) & 1, d = (i >> 3) & 1, e = (i >> 4) & 1, f = (i >> 5) & 1;
	const int A = (i & 1) * 0x1ff, D = i >> q.bits;
	int B = 0, C = 0;
	if (q.trits)
	{
		constexpr int Cs[6] = {204, 93, 44, 22, 11, 5};
		C = Cs[q.bits - 1];
		B = q.bits == 2 ? b * 0x116 : q.bits == 3 ? b * 0x85 + c * 0x10a : q.bits == 4 ? b * 0x41 + c * 0x82 + d * 0x104 :
		    q.bits == 5 ? b * 0x20 + c * 0x40 + d * 0x81 + e * 0x102 : q.bits == 6 ? b * 0x10 + c * 0x20 + d * 0x40 + e * 0x80 + f * 0x101 : 0;
	}
	else
	{
		constexpr int Cs[5] = {113, 54, 26, 13, 6};
		C = Cs[q.bits - 1];
		B = q.bits == 2 ? b * 0x10c : q.bits == 3 ? b * 0x82 + c * 0x105 : q.bits == 4 ? b * 0x40 + c * 0x81 + d * 0x102 :
		    q.bits == 5 ? b * 0x20 + c * 0x40 + d * 0x80 + e * 0x101 : 0;
	}
	const int unq = (D * C + B) ^ A;
	return uint8_t((A & 0x80) | (unq >> 2));
}

// 0 ... 64, the expansion of [0, 63] past 32 included.
constexpr uint8_t unquant_weight(Quant q, int i)
{
	int v = 0;
	if (!q.trits && !q.quints)
		v = q.bits == 1 ? i * 63 : q.bits == 2 ? i * 0x15 : q.bits == 3 ? i * 9 : q.bits == 4 ? (i << 2) | (i >> 2) : q.bits == 5 ? (i << 1) | (i >> 4) : 0;
	else if (q.bits == 0)
		v = q.trits ? 32 * i : 16 * i;
	else
	{
		const int b = (i >> 1) & 1, c = (i >> 2) & 1;
		const int A = 0x7f * (i & 1), D = i >> q.bits;
		int B = 0, C = 0;
		if (q.trits)
		{
			constexpr int Cs[3] = {50, 23, 11};
			C = Cs[q.bits - 1];
			B = q.bits == 2 ? 0x45 * b : q.bits == 3 ? 0x21 * b + 0x42 * c : 0;
		}
		else
		{
			constexpr int Cs[2] = {28, 13};
			C = Cs[q.bits - 1];
			B = q.bits == 2 ? 0x42 * b : 0;
		}
		const int unq = (D * C + B) ^ A;
		v = (A & 0x20) | (unq >> 2);
	}
	if (q.bits != 0 && v > 32)
		v++;
	return uint8_t(v);
}

// Five trits of the 8-bit T as 3-bit fields, then three quints of the 7-bit Q at 256 + Q (the specification's ISE tables).
constexpr uint16_t trit_quint(int i)
{
	if (i < 256)
	{
		const int T = i;
		int C = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
		if (((T >> 2) & 7) == 7)
		{
			C = (((T >> 5) & 7) << 2) | (T & 3);
			t4 = t3 = 2;
		}
		else
		{
			C = T & 0x1f;
			if (((T >> 5) & 3) == 3)
			{
				t4 = 2;
				t3 = (T >> 7) & 1;
			}
			else
			{
				t4 = (T >> 7) & 1;
				t3 = (T >> 5) & 3;
			}
		}
		if ((C & 3) == 3)
		{
			t2 = 2;
			t1 = (C >> 4) & 1;
			t0 = (((C >> 3) & 1) << 1) | (((C >> 2) & 1) & ~((C >> 3) & 1));
		}
		else if (((C >> 2) & 3) == 3)
		{
			t2 = 2;
			t1 = 2;
			t0 = C & 3;
		}
		else
		{
			t2 = (C >> 4) & 1;
			t1 = (C >> 2) & 3;
			t0 = (((C >> 1) & 1) << 1) | ((C & 1) & ~((C >> 1) & 1));
		}
		return uint16_t(t0 | (t1 << 3) | (t2 << 6) | (t3 << 9) | (t4 << 12));
	}
	const int Q = i - 256;
	int C = 0, q0 = 0, q1 = 0, q2 = 0;
	if (((Q >> 1) & 3) == 3 && ((Q >> 5) & 3) == 0)
	{
		q2 = ((Q & 1) << 2) | ((((Q >> 4) & 1) & ~(Q & 1)) << 1) | (((Q >> 3) & 1) & ~(Q & 1));
		q1 = q0 = 4;
	}
	else
	{
		if (((Q >> 1) & 3) == 3)
		{
			q2 = 4;
			C = (((Q >> 3) & 3) << 3) | ((~(Q >> 5) & 3) << 1) | (Q & 1);
		}
		else
		{
			q2 = (Q >> 5) & 3;
			C = Q & 0x1f;
		}
		if ((C & 7) == 5)
		{
			q1 = 4;
			q0 = (C >> 3) & 3;
		}
		else
		{
			q1 = (C >> 3) & 3;
			q0 = C & 7;
		}
	}
	return uint16_t(q0 | (q1 << 3) | (q2 << 6));
}

struct Tables
{
	uint8_t endpoint_quantiser[9][128];                 // [pairs - 1][remaining bits] -> endpoint_mode index, 0xff = nothing fits
	uint16_t endpoint_unquant_offset[ENDPOINT_MODES];   // into endpoint_unquant
	uint8_t endpoint_unquant[ENDPOINT_UNQUANT_SIZE];
	uint8_t weight_unquant_offset[WEIGHT_MODES];        // into weight_unquant
	uint8_t weight_unquant[WEIGHT_UNQUANT_SIZE];
	uint16_t trits_quints[256 + 128];
};

constexpr Tables build_tables()
{
	Tables t = {};
	int offset = 0;
	for (int m = 0; m < ENDPOINT_MODES; m++)
	{
		t.endpoint_unquant_offset[m] = uint16_t(offset);
		for (int i = 0; i < value_range(endpoint_mode(m)); i++)
			t.endpoint_unquant[offset++] = unquant_endpoint(endpoint_mode(m), i);
	}
	for (int pairs = 1; pairs <= 9; pairs++)
		for (int remaining = 0; remaining < 128; remaining++)
		{
			t.endpoint_quantiser[pairs - 1][remaining] = 0xff;
			for (int m = 0; m < ENDPOINT_MODES; m++)
				if (sequence_bits(endpoint_mode(m), 2 * pairs) <= remaining)
				{
					t.endpoint_quantiser[pairs - 1][remaining] = uint8_t(m);
					break;
				}
		}
	offset = 0;
	for (int m = 0; m < WEIGHT_MODES; m++)
	{
		t.weight_unquant_offset[m] = uint8_t(offset);
		for (int i = 0; i < value_range(weight_mode(m)); i++)
			t.weight_unquant[offset++] = unquant_weight(weight_mode(m), i);
	}
	for (int i = 0; i < 256 + 128; i++)
		t.trits_quints[i] = trit_quint(i);
	return t;
}

GR_HD const Tables &tables()
{
	static constexpr Tables t = build_tables();
	return t;
}

// ---- bits -----------------------------------------------------------------------------------------------------------------------------

struct Payload
{
	uint64_t lo, hi; // bits 0..63 and 64..127 of the block
};

// n bits (0..16) from bit `off` (>= 0); bits at and above 128 read as 0.
GR_HD uint32_t bits(const Payload &p, int off, int n)
{
	if (n <= 0 || off >= 128)
		return 0;
	uint64_t v;
	if (off >= 64)
		v = p.hi >> (off - 64);
	else if (off == 0)
		v = p.lo;
	else
		v = (p.lo >> off) | (p.hi << (64 - off));
	return uint32_t(v) & ((1u << n) - 1u);
}

// The low n bits (0..128) kept.
GR_HD Payload keep_low(const Payload &p, int n)
{
	Payload r;
	r.lo = n >= 64 ? p.lo : n <= 0 ? 0 : p.lo & ((uint64_t(1) << n) - 1);
	r.hi = n >= 128 ? p.hi : n <= 64 ? 0 : p.hi & ((uint64_t(1) << (n - 64)) - 1);
	return r;
}

GR_HD uint64_t reverse64(uint64_t v)
{
	v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
	v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
	v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
	v = ((v >> 8) & 0x00ff00ff00ff00ffull) | ((v & 0x00ff00ff00ff00ffull) << 8);
	v = ((v >> 16) & 0x0000ffff0000ffffull) | ((v & 0x0000ffff0000ffffull) << 16);
	return (v >> 32) | (v << 32);
}

// Value `index` of an integer sequence that starts at bit `start`: trits in groups of five (8 shared bits), quints in groups of three (7).
GR_HD int sequence_value(const Payload &p, int start, int index, Quant q)
{
	const int b = q.bits;
	if (q.trits)
	{
		const int group = index / 5, at = index - group * 5;
		start += group * (5 * b + 8);
		const uint32_t T = bits(p, start + b, 2) | (bits(p, start + 2 * b + 2, 2) << 2) | (bits(p, start + 3 * b + 4, 1) << 4) |
		                   (bits(p, start + 4 * b + 5, 2) << 5) | (bits(p, start + 5 * b + 7, 1) << 7);
		const int t = (tables().trits_quints[T] >> (3 * at)) & 7;
		return (t << b) | int(bits(p, start + at * b + (at * 8 + 4) / 5, b));
	}
	if (q.quints)
	{
		const int group = index / 3, at = index - group * 3;
		start += group * (3 * b + 7);
		const uint32_t Q = bits(p, start + b, 3) | (bits(p, start + 2 * b + 3, 2) << 3) | (bits(p, start + 3 * b + 5, 2) << 5);
		const int v = (tables().trits_quints[256 + Q] >> (3 * at)) & 7;
		return (v << b) | int(bits(p, start + at * b + (at * 7 + 2) / 3, b));
	}
	return int(bits(p, start + index * b, b));
}

// ---- the block half ----------------------------------------------------------------------------------------------------------------

enum : uint8_t
{
	BLOCK_CONSTANT = 1, // every texel is `constant`: a void extent, or an error of the whole block
	BLOCK_DUAL_PLANE = 2
};

struct Block
{
	uint32_t constant;
	uint32_t endpoint[4][2]; // [partition][0 / 1] as R | G << 8 | B << 16 | A << 24
	uint8_t weights[64];     // unquantised grid weights in stream order (two planes interleaved)
	uint8_t hash[8];         // the partition hash's coefficients of x and y for a, b, c, d, shifted
	uint8_t hash_bias[4];    // its constant terms, low six bits
	uint8_t flags, partitions, plane2_channel, grid_w, grid_h;
	uint8_t error_partitions; // bit p: partition p has an HDR endpoint mode, its texels take the error colour
};

GR_HD void set_constant(Block &b, uint32_t colour)
{
	b.flags = BLOCK_CONSTANT;
	b.constant = colour;
}

GR_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// clamp255(sum >> 1), clamped first.  Written the other way round, two of these next to each other in a word are selected as one
// v_ashr_pk_u8_i32 on gfx950, whose result keeps the upper half of its destination register where the code around it expects zeros:
// with a negative sum left in that register the blue and alpha bytes came out as 0xff on the device (the host build was right).
GR_HD int half_clamp255(int sum) { return (sum < 0 ? 0 : sum > 511 ? 511 : sum) >> 1; }
GR_HD uint32_t rgba(int r, int g, int b, int a) { return uint32_t(r) | (uint32_t(g) << 8) | (uint32_t(b) << 16) | (uint32_t(a) << 24); }
// (a, b) -> b with a's top bit shifted in, a as a signed 6-bit offset.
GR_HD void bit_transfer_signed(int &a, int &b)
{
	b = (b >> 1) | (a & 0x80);
	a = (a >> 1) & 0x3f;
	if (a & 0x20)
		a -= 0x40;
}

// The LDR endpoint modes.  v: the mode's 2, 4, 6 or 8 unquantised values.  Returns false for an HDR mode (2, 3, 7, 11, 14, 15).
GR_HD bool endpoints_of_mode(int mode, const int v_in[8], uint32_t &e0, uint32_t &e1)
{
	int v[8];
	for (int i = 0; i < 8; i++)
		v[i] = v_in[i];
	switch (mode)
	{
	case 0:
		e0 = rgba(v[0], v[0], v[0], 0xff);
		e1 = rgba(v[1], v[1], v[1], 0xff);
		return true;
	case 1:
	{
		const int l0 = (v[0] >> 2) | (v[1] & 0xc0), l1 = clamp255(l0 + (v[1] & 0x3f));
		e0 = rgba(l0, l0, l0, 0xff);
		e1 = rgba(l1, l1, l1, 0xff);
		return true;
	}
	case 4:
		e0 = rgba(v[0], v[0], v[0], v[2]);
		e1 = rgba(v[1], v[1], v[1], v[3]);
		return true;
	case 5:
	{
		bit_transfer_signed(v[1], v[0]);
		bit_transfer_signed(v[3], v[2]);
		const int l0 = clamp255(v[0]), l1 = clamp255(v[0] + v[1]);
		e0 = rgba(l0, l0, l0, clamp255(v[2]));
		e1 = rgba(l1, l1, l1, clamp255(v[2] + v[3]));
		return true;
	}
	case 6:
	case 10:
		e0 = rgba((v[0] * v[3]) >> 8, (v[1] * v[3]) >> 8, (v[2] * v[3]) >> 8, mode == 10 ? v[4] : 0xff);
		e1 = rgba(v[0], v[1], v[2], mode == 10 ? v[5] : 0xff);
		return true;
	case 8:
	case 12:
	{
		const int a0 = mode == 12 ? v[6] : 0xff, a1 = mode == 12 ? v[7] : 0xff;
		if (v[1] + v[3] + v[5] >= v[0] + v[2] + v[4])
		{
			e0 = rgba(v[0], v[2], v[4], a0);
			e1 = rgba(v[1], v[3], v[5], a1);
		}
		else // blue contraction, endpoints swapped
		{
			e0 = rgba((v[1] + v[5]) >> 1, (v[3] + v[5]) >> 1, v[5], a1);
			e1 = rgba((v[0] + v[4]) >> 1, (v[2] + v[4]) >> 1, v[4], a0);
		}
		return true;
	}
	case 9:
	case 13:
	{
		bit_transfer_signed(v[1], v[0]);
		bit_transfer_signed(v[3], v[2]);
		bit_transfer_signed(v[5], v[4]);
		int a0 = 0xff, a1 = 0xff;
		if (mode == 13)
		{
			bit_transfer_signed(v[7], v[6]);
			a0 = v[6];
			a1 = v[6] + v[7];
		}
		const int r1 = v[0] + v[1], g1 = v[2] + v[3], b1 = v[4] + v[5];
		if (v[1] + v[3] + v[5] >= 0)
		{
			e0 = rgba(clamp255(v[0]), clamp255(v[2]), clamp255(v[4]), clamp255(a0));
			e1 = rgba(clamp255(r1), clamp255(g1), clamp255(b1), clamp255(a1));
		}
		else
		{
			e0 = rgba(half_clamp255(r1 + b1), half_clamp255(g1 + b1), clamp255(b1), clamp255(a1));
			e1 = rgba(half_clamp255(v[0] + v[4]), half_clamp255(v[2] + v[4]), clamp255(v[4]), clamp255(a0));
		}
		return true;
	}
	default: return false;
	}
}

GR_HD uint32_t hash52(uint32_t p)
{
	p ^= p >> 15;
	p -= p << 17;
	p += p << 7;
	p += p << 4;
	p ^= p >> 5;
	p += p << 16;
	p ^= p >> 7;
	p ^= p >> 3;
	p ^= p << 6;
	p ^= p >> 17;
	return p;
}

// The specification's partition hash (astc_select_partition) up to the point where x and y enter.
GR_HD void partition_hash(Block &b, int seed, int partitions)
{
	const uint32_t rnum = hash52(uint32_t(seed + (partitions - 1) * 1024));
	int sh1, sh2;
	if (seed & 1)
	{
		sh1 = seed & 2 ? 4 : 5;
		sh2 = partitions == 3 ? 6 : 5;
	}
	else
	{
		sh1 = partitions == 3 ? 6 : 5;
		sh2 = seed & 2 ? 4 : 5;
	}
	for (int i = 0; i < 8; i++)
	{
		const uint32_t s = (rnum >> (4 * i)) & 0xf;
		b.hash[i] = uint8_t((s * s) >> (i & 1 ? sh2 : sh1));
	}
	b.hash_bias[0] = uint8_t((rnum >> 14) & 0x3f);
	b.hash_bias[1] = uint8_t((rnum >> 10) & 0x3f);
	b.hash_bias[2] = uint8_t((rnum >> 6) & 0x3f);
	b.hash_bias[3] = uint8_t((rnum >> 2) & 0x3f);
}

// Everything about a block that does not depend on the texel.  bw x bh: the footprint.
GR_HD void decode_block(const Payload &p, int bw, int bh, Block &b)
{
	const uint32_t x = uint32_t(p.lo);
	b.flags = 0;
	b.partitions = 1;
	b.plane2_channel = 0;
	b.error_partitions = 0;
	b.grid_w = b.grid_h = 1;

	if ((x & 0x1ffu) == 0x1fcu) // void extent
	{
		const int min_s = int(bits(p, 12, 13)), max_s = int(bits(p, 25, 13)), min_t = int(bits(p, 38, 13)), max_t = int(bits(p, 51, 13));
		const bool all_ones = min_s == 0x1fff && max_s == 0x1fff && min_t == 0x1fff && max_t == 0x1fff;
		if (bits(p, 10, 2) != 3u || (!all_ones && (min_s >= max_s || min_t >= max_t)))
			return set_constant(b, ERROR_COLOUR);
		// the top bytes of four 16-bit values
		return set_constant(b, uint32_t((p.hi >> 8) & 0xff) | uint32_t((p.hi >> 16) & 0xff00) | uint32_t((p.hi >> 24) & 0xff0000) | uint32_t((p.hi >> 32) & 0xff000000u));
	}

	// block mode: weight grid, weight range index, dual plane
	bool dual = (x >> 10) & 1, error = false;
	int gw = 0, gh = 0, range;
	const int a = int((x >> 5) & 3), bb = int((x >> 7) & 3);
	if (x & 3u)
	{
		range = int((x >> 4) & 1) | int((x << 1) & 6) | int((x >> 6) & 8);
		switch ((x >> 2) & 3u)
		{
		case 0: gw = bb + 4, gh = a + 2; break;
		case 1: gw = bb + 8, gh = a + 2; break;
		case 2: gw = a + 2, gh = bb + 8; break;
		default:
			if (x & 0x100u)
				gw = (bb & 1) + 2, gh = a + 2;
			else
				gw = a + 2, gh = (bb & 1) + 6;
		}
	}
	else
	{
		int p3 = int((x >> 9) & 1);
		switch (bb)
		{
		case 0: gw = 12, gh = a + 2; break;
		case 1: gw = a + 2, gh = 12; break;
		case 2:
			dual = false;
			p3 = 0;
			gw = a + 6;
			gh = int((x >> 9) & 3) + 6;
			break;
		default:
			if (a == 0)
				gw = 6, gh = 10;
			else if (a == 1)
				gw = 10, gh = 6;
			else
				error = true; // reserved
		}
		range = int((x >> 4) & 1) | int((x >> 1) & 2) | int((x >> 1) & 4) | (p3 << 3);
	}

	const int partitions = int((x >> 11) & 3) + 1;
	if (error || gw > bw || gh > bh || (dual && partitions > 3))
		return set_constant(b, ERROR_COLOUR);

	const Quant wq = weight_mode(range);
	const int weight_count = (gw * gh) << int(dual), weight_bits = sequence_bits(wq, weight_count);
	if (weight_bits < 24 || weight_bits > 96 || weight_count > 64)
		return set_constant(b, ERROR_COLOUR);

	// CEM field(s) and the bits the configuration takes
	int cem, config_bits, endpoint_offset;
	const bool multi = partitions > 1;
	if (multi)
	{
		cem = int(bits(p, 23, 6));
		endpoint_offset = 29;
		config_bits = (cem & 3) == 0 ? 29 : 25 + 3 * partitions;
	}
	else
	{
		cem = int(bits(p, 13, 4));
		endpoint_offset = config_bits = 17;
	}
	if (dual)
		config_bits += 2;
	const bool per_partition_cem = multi && (cem & 3) != 0;
	const int extra_cem_bits = per_partition_cem ? 3 * partitions - 4 : 0;

	// per-partition endpoint mode and the index of its first value
	int mode[4] = {0, 0, 0, 0}, base[4] = {0, 0, 0, 0}, pairs = 0;
	if (!multi)
	{
		mode[0] = cem;
		pairs = (cem >> 2) + 1;
	}
	else if (!per_partition_cem)
	{
		for (int i = 0; i < 4; i++)
		{
			mode[i] = cem >> 2;
			base[i] = 2 * ((cem >> 4) + 1) * i;
		}
		pairs = ((cem >> 4) + 1) * partitions;
	}
	else
	{
		const int base_class = (cem & 3) - 1;
		const int field = (int(bits(p, 128 - weight_bits - extra_cem_bits, extra_cem_bits)) << 4) | (cem >> 2);
		for (int i = 0; i < 4; i++)
			if (i < partitions)
			{
				const int cls = base_class + ((field >> i) & 1);
				mode[i] = 4 * cls + ((field >> (partitions + 2 * i)) & 3);
				base[i] = 2 * pairs;
				pairs += cls + 1;
			}
	}

	const int available = 128 - config_bits - weight_bits;
	if (pairs > 9 || available <= 0)
		return set_constant(b, ERROR_COLOUR);
	const int quantiser = tables().endpoint_quantiser[pairs - 1][available];
	if (quantiser == 0xff)
		return set_constant(b, ERROR_COLOUR);
	const Quant eq = endpoint_mode(quantiser);
	const uint8_t *unquant = tables().endpoint_unquant + tables().endpoint_unquant_offset[quantiser];
	const Payload endpoint_stream = keep_low(p, endpoint_offset + sequence_bits(eq, 2 * pairs));

	for (int i = 0; i < 4; i++)
	{
		b.endpoint[i][0] = b.endpoint[i][1] = 0;
		if (i >= partitions)
			continue;
		int v[8];
		for (int k = 0; k < 8; k++)
			v[k] = k < 2 * ((mode[i] >> 2) + 1) ? unquant[sequence_value(endpoint_stream, endpoint_offset, base[i] + k, eq)] : 0;
		if (!endpoints_of_mode(mode[i], v, b.endpoint[i][0], b.endpoint[i][1]))
			b.error_partitions |= uint8_t(1u << i);
	}
	if (b.error_partitions == (1u << partitions) - 1u)
		return set_constant(b, ERROR_COLOUR);

	b.partitions = uint8_t(partitions);
	b.grid_w = uint8_t(gw);
	b.grid_h = uint8_t(gh);
	if (dual)
	{
		b.flags |= BLOCK_DUAL_PLANE;
		b.plane2_channel = uint8_t(bits(p, 126 - weight_bits - extra_cem_bits, 2));
	}
	if (multi)
		partition_hash(b, int(bits(p, 13, 10)), partitions);

	// the weights: the block read from its top bit down
	Payload reversed = {reverse64(p.hi), reverse64(p.lo)};
	reversed = keep_low(reversed, weight_bits);
	const uint8_t *weight_unquant = tables().weight_unquant + tables().weight_unquant_offset[range];
	for (int i = 0; i < weight_count; i++)
		b.weights[i] = weight_unquant[sequence_value(reversed, 0, i, wq)];
}

// ---- the texel half ---------------------------------------------------------------------------------------------------------------

GR_HD int partition_of(const Block &b, int x, int y, bool small_block)
{
	if (small_block)
	{
		x <<= 1;
		y <<= 1;
	}
	const int a = (b.hash[0] * x + b.hash[1] * y + b.hash_bias[0]) & 0x3f;
	const int bv = (b.hash[2] * x + b.hash[3] * y + b.hash_bias[1]) & 0x3f;
	const int c = b.partitions < 3 ? 0 : (b.hash[4] * x + b.hash[5] * y + b.hash_bias[2]) & 0x3f;
	const int d = b.partitions < 4 ? 0 : (b.hash[6] * x + b.hash[7] * y + b.hash_bias[3]) & 0x3f;
	if (a >= bv && a >= c && a >= d)
		return 0;
	if (bv >= c && bv >= d)
		return 1;
	return c >= d ? 2 : 3;
}

// Texel (x, y) of a bw x bh footprint, as the four bytes of R8G8B8A8.
GR_HD uint32_t decode_texel(const Block &b, int x, int y, int bw, int bh)
{
	if (b.flags & BLOCK_CONSTANT)
		return b.constant;
	const int part = b.partitions > 1 ? partition_of(b, x, y, bw * bh < 31) : 0;
	if ((b.error_partitions >> part) & 1)
		return ERROR_COLOUR;

	// the texel in the weight grid, 4 fractional bits
	const int fx = ((1024 + bw / 2) / (bw - 1) * x * (b.grid_w - 1) + 32) >> 6, fy = ((1024 + bh / 2) / (bh - 1) * y * (b.grid_h - 1) + 32) >> 6;
	const int tx = fx & 15, ty = fy & 15;
	const int i00 = (fy >> 4) * b.grid_w + (fx >> 4), i10 = tx ? i00 + 1 : i00, i01 = ty ? i00 + b.grid_w : i00, i11 = ty ? i10 + b.grid_w : i10;
	const int w11 = (tx * ty + 8) >> 4, w10 = tx - w11, w01 = ty - w11, w00 = 16 - tx - ty + w11;
	const int dual = (b.flags & BLOCK_DUAL_PLANE) ? 1 : 0;
	int plane[2] = {0, 0};
	for (int k = 0; k <= dual; k++)
		plane[k] = (b.weights[((i00 << dual) + k) & 63] * w00 + b.weights[((i10 << dual) + k) & 63] * w10 + b.weights[((i01 << dual) + k) & 63] * w01 +
		            b.weights[((i11 << dual) + k) & 63] * w11 + 8) >> 4;

	const uint32_t e0 = b.endpoint[part][0], e1 = b.endpoint[part][1];
	uint32_t out = 0;
	for (int c = 0; c < 4; c++)
	{
		const int w = dual && c == b.plane2_channel ? plane[1] : plane[0];
		const int c0 = int((e0 >> (8 * c)) & 0xff), c1 = int((e1 >> (8 * c)) & 0xff);
		out |= uint32_t((c0 * (64 - w) + c1 * w + 32) >> 6) << (8 * c);
	}
	return out;
}
} // namespace gr_astc
