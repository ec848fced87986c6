// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// BC1-BC7 block decode, one block at a time: what assets/shaders/decode/{s3tc,rgtc,bc7,bc6}.comp compute per texel, restated per
// block.  A block's header (endpoints, partition, rotation, p-bits) is parsed once; the texels of the rows asked for are then
// interpolated from it.  Plain integer functions of the payload: texture_decode.hip calls them from its kernel, and
// tests/cpp/bc_decode_host.cpp builds the same text for the host, where tests/test_bc_ref_cpu.py holds it to the executed shaders' outputs
// (tests/golden/bc_decode_shader_v1.npz) without a device.
//
// BC1-BC5 use exact integer arithmetic (the rational value of the sample, rounded to nearest) where the shaders use fp32; the two
// agree everywhere except on BC1's three-colour midpoint when its exact value ends in 1/2, where fp32's side is chance.
// BC6H and BC7 are integer in the shaders too and are reproduced bit for bit, reserved modes included (all-zero endpoints).
// The partition, anchor and weight tables are constants of the formats (Khronos Data Format Specification, BPTC chapter).
#pragma once
#include <cstdint>
#include "core_base.hpp"

namespace gr_bc
{
enum Kind
{
	KIND_BC1_RGB = 0,
	KIND_BC1_RGBA,
	KIND_BC2,
	KIND_BC3,
	KIND_BC4,
	KIND_BC5,
	KIND_BC6H_UFLOAT,
	KIND_BC6H_SFLOAT,
	KIND_BC7,
	KIND_COUNT
};

constexpr int block_bytes(int kind) { return kind == KIND_BC1_RGB || kind == KIND_BC1_RGBA || kind == KIND_BC4 ? 8 : 16; }
constexpr int texel_bytes(int kind) { return kind == KIND_BC4 ? 1 : kind == KIND_BC5 ? 2 : kind == KIND_BC6H_UFLOAT || kind == KIND_BC6H_SFLOAT ? 8 : 4; }
// One decoded row of a block is 4 texels: 4, 8, 16 or 32 bytes, held as little-endian words.
constexpr int ROW_WORDS_MAX = 8;

struct Payload
{
	uint64_t lo, hi; // bits 0..63 and 64..127 of the block; 8-byte blocks leave hi at 0
};

// n bits (0..32) of the payload from bit `off`; off + n <= 128.
GR_HD uint32_t bits(const Payload &p, int off, int n)
{
	if (n <= 0)
		return 0;
	uint64_t v;
	if (off >= 64)
		v = p.hi >> (off - 64);
	else if (off == 0)
		v = p.lo;
	else
		v = (p.lo >> off) | (p.hi << (64 - off));
	return uint32_t(v) & (n >= 32 ? ~0u : ((1u << n) - 1u));
}

GR_HD int sign_extend(uint32_t v, int n) { return n >= 32 ? int(v) : int(v << (32 - n)) >> (32 - n); }
// n / d rounded to nearest, halves up.
GR_HD uint32_t round_div(uint32_t n, uint32_t d) { return (2u * n + d) / (2u * d); }

// ---- BC1 colour block (also the colour half of BC2 / BC3) --------------------------------------------------------------------

// The four palette entries as R | G << 8 | B << 16 | 0xff << 24.  `punch_through` is what index 3 of the three-colour mode stores.
GR_HD void bc1_palette(uint32_t endpoints, bool always_four, uint32_t punch_through, uint32_t pal[4])
{
	const uint32_t c0 = endpoints & 0xffffu, c1 = endpoints >> 16;
	const uint32_t red0 = c0 >> 11, green0 = (c0 >> 5) & 63u, blue0 = c0 & 31u;
	const uint32_t red1 = c1 >> 11, green1 = (c1 >> 5) & 63u, blue1 = c1 & 31u;
	const uint32_t opaque = 0xff000000u;
	pal[0] = round_div(255u * red0, 31u) | (round_div(255u * green0, 63u) << 8) | (round_div(255u * blue0, 31u) << 16) | opaque;
	pal[1] = round_div(255u * red1, 31u) | (round_div(255u * green1, 63u) << 8) | (round_div(255u * blue1, 31u) << 16) | opaque;
	if (always_four || c0 > c1)
	{
		pal[2] = round_div(255u * (2u * red0 + red1), 93u) | (round_div(255u * (2u * green0 + green1), 189u) << 8) | (round_div(255u * (2u * blue0 + blue1), 93u) << 16) | opaque;
		pal[3] = round_div(255u * (red0 + 2u * red1), 93u) | (round_div(255u * (green0 + 2u * green1), 189u) << 8) | (round_div(255u * (blue0 + 2u * blue1), 93u) << 16) | opaque;
	}
	else
	{
		pal[2] = round_div(255u * (red0 + red1), 62u) | (round_div(255u * (green0 + green1), 126u) << 8) | (round_div(255u * (blue0 + blue1), 62u) << 16) | opaque;
		pal[3] = punch_through;
	}
}

GR_HD uint32_t select4(uint32_t i, const uint32_t pal[4]) { return (i & 2u) ? ((i & 1u) ? pal[3] : pal[2]) : ((i & 1u) ? pal[1] : pal[0]); }

// ---- RGTC channel block (BC4, both halves of BC5, the alpha half of BC3) -----------------------------------------------------

GR_HD uint32_t rgtc_value(uint32_t e0, uint32_t e1, uint32_t k)
{
	if (k < 2u)
		return k ? e1 : e0;
	if (e0 > e1)
		return round_div(e0 * (8u - k) + e1 * (k - 1u), 7u);
	if (k > 5u)
		return (k & 1u) ? 255u : 0u;
	return round_div(e0 * (6u - k) + e1 * (k - 1u), 5u);
}

// Texel `pixel` (0..15) of an RGTC block.
GR_HD uint32_t rgtc_texel(uint64_t block, int pixel) { return rgtc_value(uint32_t(block) & 0xffu, uint32_t(block >> 8) & 0xffu, uint32_t(block >> (16 + 3 * pixel)) & 7u); }

// ---- BPTC tables --------------------------------------------------------------------------------------------------------------

// Subset of each texel, one bit per texel (two subsets) or two (three subsets), texel 0 in the low bits.
GR_HD uint32_t partition2(uint32_t shape)
{
	static constexpr uint16_t table[64] = {
		0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000,
		0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c,
		0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a, 0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x0660,
		0x0272, 0x04e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c, 0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0x0fcc, 0x7744, 0xee22};
	return table[shape];
}

GR_HD uint32_t partition3(uint32_t shape)
{
	static constexpr uint32_t table[64] = {
		0xaa685050u, 0x6a5a5040u, 0x5a5a4200u, 0x5450a0a8u, 0xa5a50000u, 0xa0a05050u, 0x5555a0a0u, 0x5a5a5050u,
		0xaa550000u, 0xaa555500u, 0xaaaa5500u, 0x90909090u, 0x94949494u, 0xa4a4a4a4u, 0xa9a59450u, 0x2a0a4250u,
		0xa5945040u, 0x0a425054u, 0xa5a5a500u, 0x55a0a0a0u, 0xa8a85454u, 0x6a6a4040u, 0xa4a45000u, 0x1a1a0500u,
		0x0050a4a4u, 0xaaa59090u, 0x14696914u, 0x69691400u, 0xa08585a0u, 0xaa821414u, 0x50a4a450u, 0x6a5a0200u,
		0xa9a58000u, 0x5090a0a8u, 0xa8a09050u, 0x24242424u, 0x00aa5500u, 0x24924924u, 0x24499224u, 0x50a50a50u,
		0x500aa550u, 0xaaaa4444u, 0x66660000u, 0xa5a0a5a0u, 0x50a050a0u, 0x69286928u, 0x44aaaa44u, 0x66666600u,
		0xaa444444u, 0x54a854a8u, 0x95809580u, 0x96969600u, 0xa85454a8u, 0x80959580u, 0xaa141414u, 0x96960000u,
		0xaaaa1414u, 0xa05050a0u, 0xa0a5a5a0u, 0x96000000u, 0x40804080u, 0xa9a8a9a8u, 0xaaaaaa44u, 0x2a4a5254u};
	return table[shape];
}

// Anchor texel of the second subset of a two-subset shape.
GR_HD int anchor2(uint32_t shape)
{
	static constexpr uint8_t table[64] = {15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
	                                      15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15};
	return table[shape];
}

// Anchor texels of the second and third subset of a three-subset shape, second | third << 4.
GR_HD uint32_t anchor3(uint32_t shape)
{
	static constexpr uint8_t second[64] = {3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
	                                       8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3};
	static constexpr uint8_t third[64] = {15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
	                                      15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8};
	return uint32_t(second[shape]) | (uint32_t(third[shape]) << 4);
}

// Interpolation weight of an n-bit index (n = 2, 3, 4): 0, 21, 43, 64 / 0, 9, ... 64 / 0, 4, 9, ... 64.
GR_HD uint32_t bptc_weight(int n, uint32_t index)
{
	const uint32_t top = (1u << n) - 1u;
	return (64u * index + top / 2u) / top;
}

// ---- BC7 ----------------------------------------------------------------------------------------------------------------------

struct Bc7Mode
{
	int subsets, partition_bits, rotation_bits, index_selection_bits, colour_bits, alpha_bits, endpoint_pbits, shared_pbits, index_bits, index_bits2;
};

constexpr Bc7Mode bc7_mode(int mode)
{
	switch (mode)
	{
	case 0: return {3, 4, 0, 0, 4, 0, 1, 0, 3, 0};
	case 1: return {2, 6, 0, 0, 6, 0, 0, 1, 3, 0};
	case 2: return {3, 6, 0, 0, 5, 0, 0, 0, 2, 0};
	case 3: return {2, 6, 0, 0, 7, 0, 1, 0, 2, 0};
	case 4: return {1, 0, 2, 1, 5, 6, 0, 0, 2, 3};
	case 5: return {1, 0, 2, 0, 7, 8, 0, 0, 2, 2};
	case 6: return {1, 0, 0, 0, 7, 7, 1, 0, 4, 0};
	default: return {2, 6, 0, 0, 5, 5, 1, 0, 2, 0};
	}
}

GR_HD uint32_t select3(uint32_t s, uint32_t a, uint32_t b, uint32_t c) { return s == 0u ? a : s == 1u ? b : c; }

// Rows [row0, row0 + ROWS) of a block of mode MODE as RGBA8 words.
template <int MODE, int ROWS>
GR_HD void bc7_rows(const Payload &p, int row0, uint32_t (*words)[ROW_WORDS_MAX])
{
	constexpr Bc7Mode m = bc7_mode(MODE);
	constexpr int channels = m.alpha_bits ? 4 : 3;
	constexpr int pbit = (m.endpoint_pbits || m.shared_pbits) ? 1 : 0;
	int off = MODE + 1;
	const uint32_t shape = bits(p, off, m.partition_bits);
	off += m.partition_bits;
	const uint32_t rotation = bits(p, off, m.rotation_bits);
	off += m.rotation_bits;
	const uint32_t index_selection = bits(p, off, m.index_selection_bits);
	off += m.index_selection_bits;

	// endpoint[subset][which][channel]; the stream holds, per channel, every subset's pair in turn
	uint32_t e[3][2][4];
	for (int c = 0; c < channels; c++)
		for (int s = 0; s < m.subsets; s++)
			for (int k = 0; k < 2; k++)
			{
				const int n = c < 3 ? m.colour_bits : m.alpha_bits;
				e[s][k][c] = bits(p, off, n);
				off += n;
			}
	for (int s = 0; s < m.subsets; s++)
	{
		uint32_t pb[2] = {0, 0};
		if (m.endpoint_pbits)
		{
			pb[0] = bits(p, off, 1);
			pb[1] = bits(p, off + 1, 1);
			off += 2;
		}
		else if (m.shared_pbits)
		{
			pb[0] = pb[1] = bits(p, off, 1);
			off += 1;
		}
		for (int k = 0; k < 2; k++)
		{
			for (int c = 0; c < channels; c++)
			{
				const int n = (c < 3 ? m.colour_bits : m.alpha_bits) + pbit;
				const uint32_t v = pbit ? ((e[s][k][c] << 1) | pb[k]) : e[s][k][c];
				e[s][k][c] = ((v << (8 - n)) | (v >> (2 * n - 8))) & 0xffu;
			}
			if (channels == 3)
				e[s][k][3] = 0xffu;
		}
	}
	// R | B << 16 and G | A << 16: two channels share one multiply where they share the weight
	uint32_t rb[3][2], ga[3][2];
	for (int s = 0; s < 3; s++)
		for (int k = 0; k < 2; k++)
		{
			const int t = s < m.subsets ? s : 0;
			rb[s][k] = e[t][k][0] | (e[t][k][2] << 16);
			ga[s][k] = e[t][k][1] | (e[t][k][3] << 16);
		}

	const int index_off = off, index_off2 = off + 16 * m.index_bits - m.subsets;
	const uint32_t subset_map = m.subsets == 2 ? partition2(shape) : m.subsets == 3 ? partition3(shape) : 0u;
	// 16 = no such anchor
	const int anchor_a = m.subsets == 2 ? anchor2(shape) : m.subsets == 3 ? int(anchor3(shape) & 15u) : 16;
	const int anchor_b = m.subsets == 3 ? int(anchor3(shape) >> 4) : 16;

	for (int r = 0; r < ROWS; r++)
		for (int x = 0; x < 4; x++)
		{
			const int pixel = 4 * (row0 + r) + x;
			const uint32_t s = m.subsets == 2 ? (subset_map >> pixel) & 1u : m.subsets == 3 ? (subset_map >> (2 * pixel)) & 3u : 0u;
			// an anchor texel's index has one bit less: every texel after it sits one bit earlier
			const int at = index_off + m.index_bits * pixel - (pixel > 0) - (pixel > anchor_a) - (pixel > anchor_b);
			const int n = m.index_bits - ((pixel == 0 || pixel == anchor_a || pixel == anchor_b) ? 1 : 0);
			uint32_t colour_weight = bptc_weight(m.index_bits, bits(p, at, n));
			uint32_t alpha_weight = colour_weight;
			if (m.index_bits2)
			{
				const int at2 = index_off2 + m.index_bits2 * pixel - (pixel > 0);
				alpha_weight = bptc_weight(m.index_bits2, bits(p, at2, m.index_bits2 - (pixel == 0 ? 1 : 0)));
				if (index_selection)
				{
					const uint32_t t = colour_weight;
					colour_weight = alpha_weight;
					alpha_weight = t;
				}
			}
			const uint32_t rb0 = select3(s, rb[0][0], rb[1][0], rb[2][0]), rb1 = select3(s, rb[0][1], rb[1][1], rb[2][1]);
			const uint32_t ga0 = select3(s, ga[0][0], ga[1][0], ga[2][0]), ga1 = select3(s, ga[0][1], ga[1][1], ga[2][1]);
			const uint32_t rb_out = (((64u - colour_weight) * rb0 + colour_weight * rb1 + 0x00200020u) >> 6) & 0x00ff00ffu;
			uint32_t red = rb_out & 0xffu, blue = rb_out >> 16, green, alpha;
			if (m.index_bits2)
			{
				green = ((64u - colour_weight) * (ga0 & 0xffffu) + colour_weight * (ga1 & 0xffffu) + 32u) >> 6;
				alpha = ((64u - alpha_weight) * (ga0 >> 16) + alpha_weight * (ga1 >> 16) + 32u) >> 6;
			}
			else
			{
				const uint32_t ga_out = (((64u - colour_weight) * ga0 + colour_weight * ga1 + 0x00200020u) >> 6) & 0x00ff00ffu;
				green = ga_out & 0xffu;
				alpha = ga_out >> 16;
			}
			if (m.rotation_bits)
			{
				const uint32_t a = alpha;
				if (rotation == 1u)
				{
					alpha = red;
					red = a;
				}
				else if (rotation == 2u)
				{
					alpha = green;
					green = a;
				}
				else if (rotation == 3u)
				{
					alpha = blue;
					blue = a;
				}
			}
			words[r][x] = red | (green << 8) | (blue << 16) | (alpha << 24);
		}
}

template <int ROWS>
GR_HD void bc7_block_rows(const Payload &p, int row0, uint32_t (*words)[ROW_WORDS_MAX])
{
	// the mode is the position of the lowest set bit of the first word; none in the low byte = reserved: all zero
	const uint32_t low = uint32_t(p.lo) & 0xffu;
	if (low & 1u)
		bc7_rows<0, ROWS>(p, row0, words);
	else if (low & 2u)
		bc7_rows<1, ROWS>(p, row0, words);
	else if (low & 4u)
		bc7_rows<2, ROWS>(p, row0, words);
	else if (low & 8u)
		bc7_rows<3, ROWS>(p, row0, words);
	else if (low & 16u)
		bc7_rows<4, ROWS>(p, row0, words);
	else if (low & 32u)
		bc7_rows<5, ROWS>(p, row0, words);
	else if (low & 64u)
		bc7_rows<6, ROWS>(p, row0, words);
	else if (low & 128u)
		bc7_rows<7, ROWS>(p, row0, words);
	else
		for (int r = 0; r < ROWS; r++)
			for (int x = 0; x < 4; x++)
				words[r][x] = 0u;
}

// ---- BC6H ---------------------------------------------------------------------------------------------------------------------

// Where the bits of the twelve endpoint fields lie.  Every mode keeps the low bits of a field in the same place -- base endpoint
// (r, g, b) at 5 / 15 / 25, first delta at 35 / 45 / 55, second-subset red pair at 65 / 71, four low bits of its green pair at
// 41 / 51 and of its first blue at 61 -- and scatters the rest, which `extra` lists.
struct Bc6Piece
{
	uint8_t field, shift, off, count; // field: 0..2 base rgb, 3..5 first delta, 6..8 and 9..11 the second subset's pair
	bool reversed;                    // most significant bit first
};

struct Bc6Mode
{
	bool valid, two_subsets, transformed;
	int endpoint_bits, delta_bits[3], extras;
	Bc6Piece extra[10];
};

constexpr Bc6Mode bc6_mode(int low5)
{
	constexpr uint8_t R0 = 0, G0 = 1, B0 = 2, G2 = 7, B2 = 8, G3 = 10, B3 = 11;
	if ((low5 & 3) == 0)
		return {true, true, true, 10, {5, 5, 5}, 8, {{G2, 4, 2, 1}, {B2, 4, 3, 1}, {G3, 4, 40, 1}, {B3, 0, 50, 1}, {B3, 1, 60, 1}, {B3, 2, 70, 1}, {B3, 3, 76, 1}, {B3, 4, 4, 1}}};
	if ((low5 & 3) == 1)
		return {true, true, true, 7, {6, 6, 6}, 10, {{G2, 4, 24, 1}, {G2, 5, 2, 1}, {B2, 4, 14, 1}, {B2, 5, 22, 1}, {G3, 4, 3, 2}, {B3, 0, 12, 2}, {B3, 2, 23, 1}, {B3, 3, 32, 1}, {B3, 4, 34, 1}, {B3, 5, 33, 1}}};
	switch (low5)
	{
	case 2: return {true, true, true, 11, {5, 4, 4}, 7, {{R0, 10, 40, 1}, {G0, 10, 49, 1}, {B0, 10, 59, 1}, {B3, 0, 50, 1}, {B3, 1, 60, 1}, {B3, 2, 70, 1}, {B3, 3, 76, 1}}};
	case 6: return {true, true, true, 11, {4, 5, 4}, 9, {{R0, 10, 39, 1}, {G0, 10, 50, 1}, {B0, 10, 59, 1}, {G2, 4, 75, 1}, {G3, 4, 40, 1}, {B3, 0, 69, 1}, {B3, 1, 60, 1}, {B3, 2, 70, 1}, {B3, 3, 76, 1}}};
	case 10: return {true, true, true, 11, {4, 4, 5}, 8, {{R0, 10, 39, 1}, {G0, 10, 49, 1}, {B0, 10, 60, 1}, {B2, 4, 40, 1}, {B3, 0, 50, 1}, {B3, 1, 69, 2}, {B3, 3, 76, 1}, {B3, 4, 75, 1}}};
	case 14: return {true, true, true, 9, {5, 5, 5}, 8, {{G2, 4, 24, 1}, {B2, 4, 14, 1}, {G3, 4, 40, 1}, {B3, 0, 50, 1}, {B3, 1, 60, 1}, {B3, 2, 70, 1}, {B3, 3, 76, 1}, {B3, 4, 34, 1}}};
	case 18: return {true, true, true, 8, {6, 5, 5}, 7, {{G2, 4, 24, 1}, {B2, 4, 14, 1}, {G3, 4, 13, 1}, {B3, 0, 50, 1}, {B3, 1, 60, 1}, {B3, 2, 23, 1}, {B3, 3, 33, 2}}};
	case 22: return {true, true, true, 8, {5, 6, 5}, 10, {{G2, 4, 24, 1}, {G2, 5, 23, 1}, {B2, 4, 14, 1}, {G3, 4, 40, 1}, {G3, 5, 33, 1}, {B3, 0, 13, 1}, {B3, 1, 60, 1}, {B3, 2, 70, 1}, {B3, 3, 76, 1}, {B3, 4, 34, 1}}};
	case 26: return {true, true, true, 8, {5, 5, 6}, 10, {{G2, 4, 24, 1}, {B2, 4, 14, 1}, {B2, 5, 23, 1}, {G3, 4, 40, 1}, {B3, 0, 50, 1}, {B3, 1, 13, 1}, {B3, 2, 70, 1}, {B3, 3, 76, 1}, {B3, 4, 34, 1}, {B3, 5, 33, 1}}};
	case 30: return {true, true, false, 6, {6, 6, 6}, 10, {{G2, 4, 24, 1}, {G2, 5, 21, 1}, {B2, 4, 14, 1}, {B2, 5, 22, 1}, {G3, 4, 11, 1}, {G3, 5, 31, 1}, {B3, 0, 12, 2}, {B3, 2, 23, 1}, {B3, 3, 32, 1}, {B3, 4, 33, 2, true}}};
	case 3: return {true, false, false, 10, {10, 10, 10}, 0, {}};
	case 7: return {true, false, true, 11, {9, 9, 9}, 3, {{R0, 10, 44, 1}, {G0, 10, 54, 1}, {B0, 10, 64, 1}}};
	case 11: return {true, false, true, 12, {8, 8, 8}, 3, {{R0, 10, 43, 2, true}, {G0, 10, 53, 2, true}, {B0, 10, 63, 2, true}}};
	case 15: return {true, false, true, 16, {4, 4, 4}, 3, {{R0, 10, 39, 6, true}, {G0, 10, 49, 6, true}, {B0, 10, 59, 6, true}}};
	default: return {false, false, false, 0, {0, 0, 0}, 0, {}};
	}
}

template <bool SIGNED>
GR_HD int bc6_unquantize(int v, int n)
{
	if (SIGNED)
	{
		v = sign_extend(uint32_t(v), n);
		if (n >= 16)
			return v;
		const int magnitude = v < 0 ? -v : v;
		int unq = ((magnitude << 15) + 0x4000) >> (n - 1);
		if (v == 0)
			unq = 0;
		if (magnitude >= (1 << (n - 1)) - 1)
			unq = 0x7fff;
		return v < 0 ? -unq : unq;
	}
	v = int(uint32_t(v) & ((1u << n) - 1u));
	if (n >= 15)
		return v;
	int unq = ((v << 15) + 0x4000) >> (n - 1);
	if (v == 0)
		unq = 0;
	if (v == (1 << n) - 1)
		unq = 0xffff;
	return unq;
}

// The interpolated 17-bit value to the bits of a half: scale by 31/64 (unsigned) or 31/32 with the sign in bit 15 (signed; no -0).
template <bool SIGNED>
GR_HD uint32_t bc6_finish(int v)
{
	if (!SIGNED)
		return uint32_t(v * 31) >> 6;
	if (v < 0)
	{
		const uint32_t half = 0x8000u | (uint32_t(-v * 31) >> 5);
		return half == 0x8000u ? 0u : half;
	}
	return uint32_t(v * 31) >> 5;
}

template <int LOW5, bool SIGNED, int ROWS>
GR_HD void bc6_rows(const Payload &p, int row0, uint32_t (*words)[ROW_WORDS_MAX])
{
	constexpr Bc6Mode m = bc6_mode(LOW5);
	constexpr int base_low = m.endpoint_bits < 10 ? m.endpoint_bits : 10;
	uint32_t f[12] = {};
	for (int c = 0; c < 3; c++)
	{
		f[c] = bits(p, 5 + 10 * c, base_low);
		f[3 + c] = bits(p, 35 + 10 * c, m.delta_bits[c]);
	}
	if (m.two_subsets)
	{
		f[6] = bits(p, 65, m.delta_bits[0]);
		f[9] = bits(p, 71, m.delta_bits[0]);
		f[7] = bits(p, 41, 4);
		f[10] = bits(p, 51, 4);
		f[8] = bits(p, 61, 4);
	}
	for (int i = 0; i < m.extras; i++)
	{
		const Bc6Piece piece = m.extra[i];
		uint32_t v = bits(p, piece.off, piece.count);
		if (piece.reversed)
		{
			uint32_t t = 0;
			for (int b = 0; b < piece.count; b++)
				t |= ((v >> b) & 1u) << (piece.count - 1 - b);
			v = t;
		}
		f[piece.field] |= v << piece.shift;
	}
	// endpoint[subset][which][channel]
	int e[2][2][3];
	for (int c = 0; c < 3; c++)
	{
		const int base = int(f[c]);
		for (int i = 1; i < 4; i++)
		{
			const int raw = m.transformed ? base + sign_extend(f[3 * i + c], m.delta_bits[c]) : int(f[3 * i + c]);
			e[i >> 1][i & 1][c] = bc6_unquantize<SIGNED>(raw, m.endpoint_bits);
		}
		e[0][0][c] = bc6_unquantize<SIGNED>(base, m.endpoint_bits);
	}
	const uint32_t shape = bits(p, 77, 5);
	const uint32_t subset_map = m.two_subsets ? partition2(shape) : 0u;
	const int anchor = m.two_subsets ? anchor2(shape) : 16;
	constexpr int index_bits = m.two_subsets ? 3 : 4;
	constexpr int index_off = m.two_subsets ? 82 : 65;
	for (int r = 0; r < ROWS; r++)
		for (int x = 0; x < 4; x++)
		{
			const int pixel = 4 * (row0 + r) + x;
			const bool second = ((subset_map >> pixel) & 1u) != 0u;
			const int at = index_off + index_bits * pixel - (pixel > 0) - (pixel > anchor);
			const int n = index_bits - ((pixel == 0 || pixel == anchor) ? 1 : 0);
			const int w = int(bptc_weight(index_bits, bits(p, at, n)));
			uint32_t half[3];
			for (int c = 0; c < 3; c++)
			{
				const int e0 = second ? e[1][0][c] : e[0][0][c], e1 = second ? e[1][1][c] : e[0][1][c];
				half[c] = bc6_finish<SIGNED>(((64 - w) * e0 + w * e1 + 32) >> 6) & 0xffffu;
			}
			words[r][2 * x] = half[0] | (half[1] << 16);
			words[r][2 * x + 1] = half[2] | (0x3c00u << 16);
		}
}

template <bool SIGNED, int ROWS>
GR_HD void bc6_block_rows(const Payload &p, int row0, uint32_t (*words)[ROW_WORDS_MAX])
{
	const uint32_t low5 = uint32_t(p.lo) & 31u;
	switch ((low5 & 2u) ? low5 : (low5 & 1u))
	{
	case 0: bc6_rows<0, SIGNED, ROWS>(p, row0, words); break;
	case 1: bc6_rows<1, SIGNED, ROWS>(p, row0, words); break;
	case 2: bc6_rows<2, SIGNED, ROWS>(p, row0, words); break;
	case 6: bc6_rows<6, SIGNED, ROWS>(p, row0, words); break;
	case 10: bc6_rows<10, SIGNED, ROWS>(p, row0, words); break;
	case 14: bc6_rows<14, SIGNED, ROWS>(p, row0, words); break;
	case 18: bc6_rows<18, SIGNED, ROWS>(p, row0, words); break;
	case 22: bc6_rows<22, SIGNED, ROWS>(p, row0, words); break;
	case 26: bc6_rows<26, SIGNED, ROWS>(p, row0, words); break;
	case 30: bc6_rows<30, SIGNED, ROWS>(p, row0, words); break;
	case 3: bc6_rows<3, SIGNED, ROWS>(p, row0, words); break;
	case 7: bc6_rows<7, SIGNED, ROWS>(p, row0, words); break;
	case 11: bc6_rows<11, SIGNED, ROWS>(p, row0, words); break;
	case 15: bc6_rows<15, SIGNED, ROWS>(p, row0, words); break;
	default:
		// reserved: zero endpoints, which finish as +0 in every channel
		for (int r = 0; r < ROWS; r++)
			for (int x = 0; x < 4; x++)
			{
				words[r][2 * x] = 0u;
				words[r][2 * x + 1] = 0x3c00u << 16;
			}
		break;
	}
}

// ---- one entry for every format -------------------------------------------------------------------------------------------------

// Rows [row0, row0 + ROWS) of the block, words[r] = the row's 4 texels as little-endian words (texel_bytes(KIND) each).
template <int KIND, int ROWS>
GR_HD void decode_rows(const Payload &p, int row0, uint32_t (*words)[ROW_WORDS_MAX])
{
	if (KIND == KIND_BC7)
		bc7_block_rows<ROWS>(p, row0, words);
	else if (KIND == KIND_BC6H_UFLOAT || KIND == KIND_BC6H_SFLOAT)
		bc6_block_rows<KIND == KIND_BC6H_SFLOAT, ROWS>(p, row0, words);
	else if (KIND == KIND_BC4 || KIND == KIND_BC5)
	{
		for (int r = 0; r < ROWS; r++)
		{
			uint32_t red = 0, green = 0;
			for (int x = 0; x < 4; x++)
			{
				const int pixel = 4 * (row0 + r) + x;
				red |= rgtc_texel(p.lo, pixel) << (8 * x);
				if (KIND == KIND_BC5)
					green |= rgtc_texel(p.hi, pixel) << (8 * x);
			}
			if (KIND == KIND_BC4)
				words[r][0] = red;
			else
			{
				// R and G bytes interleaved
				for (int h = 0; h < 2; h++)
				{
					const uint32_t r2 = (red >> (16 * h)) & 0xffffu, g2 = (green >> (16 * h)) & 0xffffu;
					words[r][h] = (r2 & 0xffu) | ((g2 & 0xffu) << 8) | ((r2 >> 8) << 16) | ((g2 >> 8) << 24);
				}
			}
		}
	}
	else
	{
		// BC1 keeps its colours in the only 8 bytes, BC2 / BC3 in the second 8 after the alpha
		const uint64_t colour = KIND == KIND_BC2 || KIND == KIND_BC3 ? p.hi : p.lo;
		uint32_t pal[4];
		bc1_palette(uint32_t(colour), KIND == KIND_BC2 || KIND == KIND_BC3, KIND == KIND_BC1_RGB ? 0xff000000u : 0u, pal);
		const uint32_t indices = uint32_t(colour >> 32);
		for (int r = 0; r < ROWS; r++)
			for (int x = 0; x < 4; x++)
			{
				const int pixel = 4 * (row0 + r) + x;
				uint32_t texel = select4((indices >> (2 * pixel)) & 3u, pal);
				if (KIND == KIND_BC2)
					texel = (texel & 0x00ffffffu) | ((uint32_t(p.lo >> (4 * pixel)) & 15u) * 17u << 24);
				else if (KIND == KIND_BC3)
					texel = (texel & 0x00ffffffu) | (rgtc_texel(p.lo, pixel) << 24);
				words[r][x] = texel;
			}
	}
}
} // namespace gr_bc
