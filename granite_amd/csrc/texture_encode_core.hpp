// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The rules of the texture encoder, stated once for the kernels of texture_encode.hip (hipcc) and for the stand-alone host program of the
// CPU tests (tests/cpp/texture_encode_core_host.cpp, g++): the RGTC (BC4 / BC5) block compressor of scene-export/rgtc_compressor.cpp and the
// UNORM8 mip rule of scene-export/texture_utils.cpp (generate_mipmaps<Ops>), in this project's own words.  Integer arithmetic for the blocks;
// for the mips every fp32 operation is one rounding, so a translation unit that includes this header is built with -ffp-contract=off.
//
// A channel block is the 16 values of one component of a 4 x 4 texel block, row by row, the block padded by clamping coordinates to the
// last texel (block_texel_offset).  Its 8 bytes are two endpoints and 16 codes of 3 bits, texel 0 in the lowest bits.  Three forms:
//   flat       range == 0: both endpoints the value, all codes 0;
//   7-weight   endpoints (max, min), byte 0 > byte 1: a decoder reads six values between them.  quantise() with divider7, remap7;
//   5-weight   endpoints (p_lo, p_hi), byte 0 <= byte 1: four values between them, code 6 is 0 and code 7 is 255.  code5().
// A block of range >= RANGE_THRESHOLD is searched: with the values sorted, each of the 120 pairs lo <= hi < 15 of sorted positions is a
// candidate (p_lo, p_hi) = (sorted[lo], sorted[hi]); its squared error is below_sum(lo) + inside_sum(lo, hi) + above_sum(hi).  A
// candidate replaces the best so far only with a strictly smaller error, the 7-weight form being the first best.  search_key() turns
// that rule into one unsigned minimum: error in the high bits, the position in the search order (0 the 7-weight form, c + 1 candidate c)
// in the low seven.
#pragma once
#include "core_base.hpp"

namespace gr_texenc
{
constexpr int RANGE_THRESHOLD = 16;
constexpr int DIV_7 = 0x100000 / 7;
constexpr int DIV_5 = 0x100000 / 5;
constexpr int CANDIDATES = 120; // lo in [0, 15), hi in [lo, 15)
constexpr int KEY_SLOT_BITS = 7; // 121 slots; the largest error, 16 * 255^2, is below 2^20

GR_HD int mini(int a, int b) { return a < b ? a : b; }

// ---- block fetch ---------------------------------------------------------------------------------------------------------------
// Texel `i` (0 .. 15, row by row) of the block at (bx, by): byte offset of its pixel in an image of `pitch` bytes a row and `stride` bytes
// a pixel.  Coordinates past the image read its last column / row.
GR_HD size_t block_texel_offset(uint32_t bx, uint32_t by, int i, uint32_t width, uint32_t height, uint32_t pitch, uint32_t stride)
{
	uint32_t x = 4u * bx + uint32_t(i & 3), y = 4u * by + uint32_t(i >> 2);
	x = x < width - 1u ? x : width - 1u;
	y = y < height - 1u ? y : height - 1u;
	return size_t(y) * pitch + size_t(x) * stride;
}

// ---- the 7-weight form -----------------------------------------------------------------------------------------------------------
GR_HD int divider7(int range) { return (0x700000 + (range >> 1)) / range; } // range >= 1
GR_HD int divider5(int range) { return range ? (0x500000 + (range >> 1)) / range : 0; }
// position of v between lo and lo + range in sevenths (divider7) or fifths (divider5), rounded
GR_HD int quantise(int v, int lo, int divider) { return ((v - lo) * divider + 0x80000) >> 20; }
// position 7 is endpoint 0 (the maximum), position 0 endpoint 1, the rest count down from endpoint 0
GR_HD int remap7(int position) { return position == 7 ? 0 : (position == 0 ? 1 : 8 - position); }
GR_HD int error7(int v, int lo, int range, int position)
{
	const int d = lo + ((range * position * DIV_7 + 0x80000) >> 20) - v;
	return d * d;
}

// ---- the search ------------------------------------------------------------------------------------------------------------------
// Position of texel i among the sorted values: values below it, and equal values before it.  A permutation of 0 .. 15.
GR_HD int rank_of(const uint8_t *texels, int i)
{
	const int v = texels[i];
	int rank = 0;
	GR_UNROLL
	for (int j = 0; j < 16; j++)
		rank += (texels[j] < v || (texels[j] == v && j < i)) ? 1 : 0;
	return rank;
}

// Sorted values below position lo: each goes to 0 or to p_lo, whichever is nearer.
GR_HD int below_sum(const uint8_t *sorted, int lo)
{
	const int p_lo = sorted[lo];
	int error = 0;
	GR_UNROLL
	for (int i = 0; i < 15; i++)
	{
		const int s = sorted[i], d = mini(s, p_lo - s);
		error += i < lo ? d * d : 0;
	}
	return error;
}

// Sorted values above position hi: each goes to 255 or to p_hi.
GR_HD int above_sum(const uint8_t *sorted, int hi)
{
	const int p_hi = sorted[hi];
	int error = 0;
	GR_UNROLL
	for (int i = 1; i < 16; i++)
	{
		const int s = sorted[i], d = mini(255 - s, s - p_hi);
		error += i > hi ? d * d : 0;
	}
	return error;
}

// Sorted values lo .. hi, quantised to fifths between the two.  `divider` is divider5(sorted[hi] - sorted[lo]).  The two ends are left
// out: they decode to themselves for every range (ends_cost_nothing, which the host program of the CPU tests runs over all 256 ranges).
GR_HD int inside_sum(const uint8_t *sorted, int lo, int hi, int divider)
{
	const int p_lo = sorted[lo], range = sorted[hi] - p_lo;
	int error = 0;
	for (int i = lo + 1; i < hi; i++)
	{
		const int s = sorted[i];
		const int d = p_lo + ((range * quantise(s, p_lo, divider) * DIV_5 + 0x80000) >> 20) - s;
		error += d * d;
	}
	return error;
}

// p_lo quantises to position 0 and decodes to p_lo; p_hi = p_lo + range quantises to position 5 and decodes to p_lo + range.
GR_HD bool ends_cost_nothing(int range)
{
	const int position = quantise(range, 0, divider5(range));
	return quantise(0, 0, divider5(range)) == 0 && ((range * position * DIV_5 + 0x80000) >> 20) == range && (range == 0 || position == 5);
}

// Position of the partition (lo, hi) in the search order, `for lo in [0, 15) for hi in [lo, 15)`: 0 .. 119.
GR_HD int candidate_index(int lo, int hi) { return lo * 15 - lo * (lo - 1) / 2 + (hi - lo); }

// The inverse: candidate c of the search order.
GR_HD void candidate_partition(int c, int &lo, int &hi)
{
	lo = 0;
	while (c >= 15 - lo)
	{
		c -= 15 - lo;
		lo++;
	}
	hi = lo + c;
}

// The 120 partitions in another order, widest first: k = 0 is (0, 14), then the two of width 13, ... the last 15 have lo == hi.
// inside_sum costs hi - lo + 1 terms, so lanes that take neighbouring k in the same turn run loops of nearly the same length.  The
// order of evaluation does not matter to the result: search_key carries candidate_index.
GR_HD void partition_by_width(int k, int &lo, int &hi)
{
	int n = 0;
	while (k > n)
	{
		n++;
		k -= n;
	}
	lo = k;
	hi = k + 14 - n;
}

// Smaller key = better; of equal errors the earlier slot.  Slot 0 is the 7-weight form, slot c + 1 candidate c.
GR_HD uint32_t search_key(int error, int slot) { return (uint32_t(error) << KEY_SLOT_BITS) | uint32_t(slot); }
GR_HD int key_slot(uint32_t key) { return int(key & ((1u << KEY_SLOT_BITS) - 1u)); }

// ---- the 5-weight form -----------------------------------------------------------------------------------------------------------
// Code of value v for endpoints (p_lo, p_hi): outside them 0 / 255 (codes 6 / 7) only where strictly nearer than the endpoint.
GR_HD int code5(int v, int p_lo, int p_hi, int divider)
{
	if (v < p_lo)
		return v < p_lo - v ? 6 : 0;
	if (v > p_hi)
		return 255 - v < v - p_hi ? 7 : 1;
	const int position = quantise(v, p_lo, divider);
	return position == 5 ? 1 : (position ? position + 1 : 0);
}

// ---- a whole channel block, one step after the other -----------------------------------------------------------------------------
// What the kernel spreads over the lanes of a group (texture_encode.hip) in the order a single thread does it: the host program and the
// timing tool's class counts go through here.  `form`, where given: 0 flat, 1 range below the threshold, 2 searched and the 7-weight form
// kept, 3 searched and replaced.
GR_HD void encode_channel_block(const uint8_t *texels, uint8_t *out, int *form = nullptr)
{
	int lo = 255, hi = 0;
	for (int i = 0; i < 16; i++)
	{
		lo = texels[i] < lo ? texels[i] : lo;
		hi = texels[i] > hi ? texels[i] : hi;
	}
	const int range = hi - lo;
	uint64_t bits = 0;
	int e0 = hi, e1 = lo, kind = 0;
	if (range)
	{
		const int divider = divider7(range);
		int error = 0;
		for (int i = 0; i < 16; i++)
		{
			const int position = quantise(texels[i], lo, divider);
			error += error7(texels[i], lo, range, position);
			bits |= uint64_t(remap7(position)) << (3 * i);
		}
		kind = 1;
		if (range >= RANGE_THRESHOLD)
		{
			uint8_t sorted[16];
			for (int i = 0; i < 16; i++)
				sorted[rank_of(texels, i)] = texels[i];
			uint32_t best = search_key(error, 0);
			for (int c = 0; c < CANDIDATES; c++)
			{
				int p, q;
				candidate_partition(c, p, q);
				const uint32_t key = search_key(below_sum(sorted, p) + inside_sum(sorted, p, q, divider5(sorted[q] - sorted[p])) + above_sum(sorted, q), c + 1);
				best = key < best ? key : best;
			}
			kind = 2;
			if (key_slot(best))
			{
				int p, q;
				candidate_partition(key_slot(best) - 1, p, q);
				e0 = sorted[p];
				e1 = sorted[q];
				const int divider_5 = divider5(e1 - e0);
				bits = 0;
				for (int i = 0; i < 16; i++)
					bits |= uint64_t(code5(texels[i], e0, e1, divider_5)) << (3 * i);
				kind = 3;
			}
		}
	}
	out[0] = uint8_t(e0);
	out[1] = uint8_t(e1);
	for (int i = 0; i < 6; i++)
		out[2 + i] = uint8_t(bits >> (8 * i));
	if (form)
		*form = kind;
}

// ---- mip generation (UNORM8, 1 / 2 / 4 components) -------------------------------------------------------------------------------
// Destination level of max(src >> 1, 1) texels an axis, each a bilinear tap of the level above at its own centre.
GR_HD float mip_rescale(uint32_t src, uint32_t dst) { return float(src) / float(dst); }

// One axis: the two source indices and the weight of the second.
GR_HD void mip_axis(uint32_t x, float rescale, uint32_t src_extent, uint32_t &i0, uint32_t &i1, float &weight)
{
	const float coord = (float(x) + 0.5f) * rescale - 0.5f;
	const float base = floorf(coord);
	weight = coord - base;
	i0 = uint32_t(base);
	i1 = i0 + 1u < src_extent - 1u ? i0 + 1u : src_extent - 1u;
}

GR_HD float mip_texel(uint32_t v) { return float(v) * (1.0f / 255.0f); }
GR_HD float mip_mix(float a, float b, float t) { return a * (1.0f - t) + b * t; }
// x first, then y; round half away from zero
GR_HD uint32_t mip_filter(uint32_t v00, uint32_t v10, uint32_t v01, uint32_t v11, float wx, float wy)
{
	const float top = mip_mix(mip_texel(v00), mip_texel(v10), wx), bottom = mip_mix(mip_texel(v01), mip_texel(v11), wx);
	float q = roundf(mip_mix(top, bottom, wy) * 255.0f);
	q = q < 0.0f ? 0.0f : (q > 255.0f ? 255.0f : q);
	return uint32_t(q);
}
} // namespace gr_texenc
