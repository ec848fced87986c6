// Video frame conversion for gfx950: VideoScaler::rescale (video/scaler.cpp) + assets/shaders/util/scaler.comp.  An RGB frame
// (RGBA8 UNORM / sRGB, A2B10G10R10, RGBA16F) goes through EOTF -> [polyphase rescale] -> primary conversion -> OETF and is stored
// as one RGBA8 / BGRA8 plane (ordered dither) or as full-range YCbCr planes: NV12 / P010 / P016 (Y + interleaved CbCr) or
// three planes, 4:2:0 (chroma = mean of each 2 x 2 luma block) or 4:4:4, 8 or 16 bits (UNORM16).
//
// Two kernels instead of the reference's one 64-thread group per 8 x 8 output tile:
//   k_video_direct  (SKIP_RESCALE: the encode size is the frame size, what a recorder uses): a pure stream.  One lane converts
//                   4 x 2 pixels: two 16-B loads (32 B for RGBA16F), the 2 x 2 chroma means inside the lane, one 4-B luma store
//                   per row (8 B at 16 bits; store_run) and one store per chroma plane (store_chroma).  Everything in fp32.
//   k_video_rescale (the separable 8-tap, 256-phase filter, 16 x 16 outputs per 256-thread group): the EOTF'd input halo of the
//                   tile is staged once in LDS as fp16 (as the reference stages it), filtered vertically into a second fp16 tile,
//                   then horizontally; accumulation in fp32 with the fp16 weight table.  Sample positions are the reference's
//                   8.8 fixed-point ones, computed from the same 8 x 8 tile bases, so phases and taps are the same.  With
//                   SAMPLED_DOWNSCALING the staged texels are LinearClamp samples of the input at twice the target size.
//                   The 2 x 2 chroma mean is taken across the quad by DPP; every lane stores its own samples.
// Both end in the same tails: dither_term, then pack_rgba8 for the single plane or unorm_code per sample.
// Stores outside a plane are dropped (imageStore out of bounds).  Input texels outside the frame read as zero on the direct path
// (texelFetch with robust image access; the reference fetches unclamped there) and are clamped to the edge on the rescale path
// (CLAMP_COORD).
#include "ctx.hpp"
#include "device_common.hpp"
#include <cmath>

namespace
{
enum : uint32_t
{
	VIDEO_SKIP_RESCALE = GR_VIDEO_CONTROL_SKIP_RESCALE_BIT,
	VIDEO_SAMPLED = GR_VIDEO_CONTROL_SAMPLED_DOWNSCALING_BIT,
	VIDEO_CHROMA_SUBSAMPLE = GR_VIDEO_CONTROL_CHROMA_SUBSAMPLE_BIT,
	VIDEO_PRIMARY = GR_VIDEO_CONTROL_PRIMARY_CONVERSION_BIT,
	VIDEO_DITHER = GR_VIDEO_CONTROL_DITHER_BIT,
};

enum InputKind : uint32_t
{
	IN_RGBA8 = 0,
	IN_RGBA8_SRGB = 1,
	IN_A2B10G10R10 = 2,
	IN_RGBA16F = 3,
};

constexpr int PHASES = 256;
constexpr int TAPS = 8;

struct VideoArgs
{
	const uint8_t *in;
	int in_w, in_h;
	uint32_t in_pitch, in_kind;
	uint8_t *plane[3];
	uint32_t pitch[3];
	int out_w, out_h; // plane 0
	int chroma_w, chroma_h;
	uint32_t aligned;    // bit i: plane i's pointer and pitch are multiples of 16 B (vector stores); bit 3: the input's (vector loads)
	uint32_t flags, eotf, oetf;
	uint32_t swap_rb;    // BGRA8 single plane
	float gst[12];       // gamma_space_transform, row major 3 x 4: Cr, Y, Cb
	float prim[9];       // primary_transform, column major
	float scaling_to_input[2], inv_input_resolution[2];
	float dither_strength;
	const uint16_t *weights; // fp16 [2][PHASES][TAPS]: horizontal, vertical
	const float *srgb_lut;
};

__device__ __forceinline__ float pow_pos(float x, float e) { return x > 0.0f ? __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)) : 0.0f; }

// inc/srgb.h, the piece-wise forms
__device__ __forceinline__ float decode_srgb(float c)
{
	const float r = c <= 0.0404482362771082f ? c * (1.0f / 12.92f) : pow_pos((c + 0.055f) * (1.0f / 1.055f), 2.4f);
	return saturatef(r);
}

__device__ __forceinline__ float encode_srgb(float c)
{
	c = fmaxf(c, 0.0f);
	const float r = c <= 0.0031308f ? c * 12.92f : fmaf(1.055f, pow_pos(c, 1.0f / 2.4f), -0.055f);
	return saturatef(r);
}

// scaler.comp apply_eotf / apply_oetf (ST 2084)
__device__ __forceinline__ float pq_eotf(float v)
{
	const float m1 = 0.1593017578125f, m2 = 78.84375f, c2 = 18.8515625f, c3 = 18.6875f, c1 = c3 - c2 + 1.0f;
	const float e = pow_pos(v, 1.0f / m2);
	const float num = fmaxf(e - c1, 0.0f);
	const float den = c2 - c3 * e;
	return pow_pos(num / den, 1.0f / m1) * 10000.0f;
}

__device__ __forceinline__ float pq_oetf(float v)
{
	const float c1 = 0.8359375f, c2 = 18.8515625f, c3 = 18.6875f, m1 = 0.1593017578125f, m2 = 78.84375f;
	const float y = saturatef(v * (1.0f / 10000.0f));
	const float p = pow_pos(y, m1);
	return pow_pos((c1 + c2 * p) / (1.0f + c3 * p), m2);
}

__device__ __forceinline__ float apply_transfer(uint32_t kind, bool decode, float v)
{
	if (kind == GR_VIDEO_TRANSFER_SRGB)
		return decode ? decode_srgb(v) : encode_srgb(v);
	if (kind == GR_VIDEO_TRANSFER_PQ)
		return decode ? pq_eotf(v) : pq_oetf(v);
	return v;
}

__device__ __forceinline__ float4 apply_eotf(const VideoArgs &a, float4 v)
{
	return make_float4(apply_transfer(a.eotf, true, v.x), apply_transfer(a.eotf, true, v.y), apply_transfer(a.eotf, true, v.z), v.w);
}

// primary conversion, then OETF
__device__ __forceinline__ float4 finish_rgb(const VideoArgs &a, float4 v)
{
	if (a.flags & VIDEO_PRIMARY)
	{
		const float r = a.prim[0] * v.x + a.prim[3] * v.y + a.prim[6] * v.z;
		const float g = a.prim[1] * v.x + a.prim[4] * v.y + a.prim[7] * v.z;
		const float b = a.prim[2] * v.x + a.prim[5] * v.y + a.prim[8] * v.z;
		v = make_float4(r, g, b, v.w);
	}
	return make_float4(apply_transfer(a.oetf, false, v.x), apply_transfer(a.oetf, false, v.y), apply_transfer(a.oetf, false, v.z), v.w);
}

__device__ __forceinline__ float4 decode_word(const VideoArgs &a, uint32_t u)
{
	if (a.in_kind == IN_A2B10G10R10)
		return make_float4(float(u & 1023u) * (1.0f / 1023.0f), float((u >> 10) & 1023u) * (1.0f / 1023.0f),
		                   float((u >> 20) & 1023u) * (1.0f / 1023.0f), float(u >> 30) * (1.0f / 3.0f));
	if (a.in_kind == IN_RGBA8_SRGB) // what a sampled *_SRGB view returns
		return make_float4(a.srgb_lut[u & 255u], a.srgb_lut[(u >> 8) & 255u], a.srgb_lut[(u >> 16) & 255u], unorm8_to_float(u >> 24));
	return make_float4(unorm8_to_float(u & 255u), unorm8_to_float((u >> 8) & 255u), unorm8_to_float((u >> 16) & 255u), unorm8_to_float(u >> 24));
}

// RGBA16F texel from its two dwords (R G, B A)
__device__ __forceinline__ float4 decode_half4(uint32_t rg, uint32_t ba)
{
	const f16x2 lo = __builtin_bit_cast(f16x2, rg), hi = __builtin_bit_cast(f16x2, ba);
	return make_float4(float(lo.x), float(lo.y), float(hi.x), float(hi.y));
}

// one texel, coordinates inside the frame
__device__ __forceinline__ float4 fetch_texel(const VideoArgs &a, int x, int y)
{
	const uint8_t *row = a.in + size_t(y) * a.in_pitch;
	if (a.in_kind == IN_RGBA16F)
	{
		const uint2 q = *reinterpret_cast<const uint2 *>(row + size_t(x) * 8u);
		return decode_half4(q.x, q.y);
	}
	return decode_word(a, *reinterpret_cast<const uint32_t *>(row + size_t(x) * 4u));
}

// 4x4 ordered dither of scaler.comp: D(n / 16) = n / 16 - 0.5 with n = 1, 9, 3, 11 / 13, 5, 15, 7 / 4, 12, 2, 10 / 16, 8, 14, 6, kept as n - 1
// in the nibble (y & 3) * 4 + (x & 3)
__device__ __forceinline__ float dither_at(int x, int y)
{
	const uint32_t index = uint32_t((y & 3) * 4 + (x & 3));
	const uint32_t n = uint32_t((0x5d7f91b36e4ca280ull >> (4u * index)) & 15u) + 1u;
	return float(n) * 0.0625f - 0.5f;
}

__device__ __forceinline__ uint32_t unorm_code(float v, float scale) { return uint32_t(saturatef(v) * scale + 0.5f); }

// what the dither adds to the sample at (x, y) of a plane
__device__ __forceinline__ float dither_term(const VideoArgs &a, bool dither, int x, int y) { return dither ? dither_at(x, y) * a.dither_strength : 0.0f; }

// the single plane's word at (x, y): the dither on all four channels, R and B swapped for BGRA8
__device__ __forceinline__ uint32_t pack_rgba8(const VideoArgs &a, float4 v, bool dither, int x, int y)
{
	if (dither)
	{
		const float d = dither_term(a, true, x, y);
		v = make_float4(v.x + d, v.y + d, v.z + d, v.w + d);
	}
	const uint32_t c0 = unorm_code(a.swap_rb ? v.z : v.x, 255.0f), c2 = unorm_code(a.swap_rb ? v.x : v.z, 255.0f);
	return c0 | (unorm_code(v.y, 255.0f) << 8) | (c2 << 16) | (unorm_code(v.w, 255.0f) << 24);
}

// Y / Cb / Cr of one pixel, clamped, fp32 (scaler.comp: clamp, then gamma_space_transform * vec4(rgb, 1))
__device__ __forceinline__ float3 to_ycbcr(const VideoArgs &a, float4 v)
{
	const float r = saturatef(v.x), g = saturatef(v.y), b = saturatef(v.z);
	const float cr = fmaf(a.gst[0], r, fmaf(a.gst[1], g, fmaf(a.gst[2], b, a.gst[3])));
	const float y = fmaf(a.gst[4], r, fmaf(a.gst[5], g, fmaf(a.gst[6], b, a.gst[7])));
	const float cb = fmaf(a.gst[8], r, fmaf(a.gst[9], g, fmaf(a.gst[10], b, a.gst[11])));
	return make_float3(cb, y, cr);
}

template <int BYTES> struct VecOf;
template <> struct VecOf<2> { typedef uint16_t type; };
template <> struct VecOf<4> { typedef uint32_t type; };
template <> struct VecOf<8> { typedef u32x2 type; };
template <> struct VecOf<16> { typedef u32x4 type; };

// N consecutive samples of type T at element x of one row; elements at or beyond `limit` are dropped.  x is a multiple of N, so
// with a 16-B aligned plane the run is naturally aligned and goes out as one store.
template <typename T, int N>
__device__ __forceinline__ void store_run(uint8_t *row, int x, int limit, const T (&v)[N], bool aligned)
{
	T *p = reinterpret_cast<T *>(row) + x;
	if (aligned && x + N <= limit)
	{
		typename VecOf<sizeof(T) * N>::type pack;
		__builtin_memcpy(&pack, v, sizeof(pack));
		*reinterpret_cast<typename VecOf<sizeof(T) * N>::type *>(p) = pack;
		return;
	}
#pragma unroll
	for (int i = 0; i < N; i++)
		if (x + i < limit)
			p[i] = v[i];
}

template <bool WIDE> struct Sample { typedef uint8_t type; static constexpr float scale = 255.0f; };
template <> struct Sample<true> { typedef uint16_t type; static constexpr float scale = 65535.0f; };

// N Cb / Cr pairs from chroma texel x of row y: interleaved into plane 1 (two planes), or a run into each of planes 1 and 2
template <int PLANES, typename T, int N>
__device__ __forceinline__ void store_chroma(const VideoArgs &a, int x, int y, const T (&cb)[N], const T (&cr)[N])
{
	if (PLANES == 2)
	{
		T cbcr[2 * N];
#pragma unroll
		for (int i = 0; i < N; i++)
		{
			cbcr[2 * i] = cb[i];
			cbcr[2 * i + 1] = cr[i];
		}
		store_run<T, 2 * N>(a.plane[1] + size_t(y) * a.pitch[1], 2 * x, 2 * a.chroma_w, cbcr, a.aligned & 2u);
	}
	else
	{
		store_run<T, N>(a.plane[1] + size_t(y) * a.pitch[1], x, a.chroma_w, cb, a.aligned & 2u);
		store_run<T, N>(a.plane[2] + size_t(y) * a.pitch[2], x, a.chroma_w, cr, a.aligned & 4u);
	}
}

// ---- same size -------------------------------------------------------------------------------------------------------------
constexpr int DIRECT_PX = 4;    // pixels per lane along x
constexpr int DIRECT_ROWS = 4;  // lane rows per group (each lane does two pixel rows)

__device__ __forceinline__ void load_row4(const VideoArgs &a, int x0, int y, float4 (&px)[DIRECT_PX])
{
	if (y >= a.in_h)
	{
#pragma unroll
		for (int i = 0; i < DIRECT_PX; i++)
			px[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		return;
	}
	const uint8_t *row = a.in + size_t(y) * a.in_pitch;
	const bool vec = (a.aligned & 8u) && x0 + DIRECT_PX <= a.in_w;
	if (a.in_kind == IN_RGBA16F)
	{
		if (vec)
		{
			const u32x4 q0 = *reinterpret_cast<const u32x4 *>(row + size_t(x0) * 8u);
			const u32x4 q1 = *reinterpret_cast<const u32x4 *>(row + size_t(x0) * 8u + 16u);
			px[0] = decode_half4(q0.x, q0.y);
			px[1] = decode_half4(q0.z, q0.w);
			px[2] = decode_half4(q1.x, q1.y);
			px[3] = decode_half4(q1.z, q1.w);
			return;
		}
	}
	else if (vec)
	{
		const u32x4 q = *reinterpret_cast<const u32x4 *>(row + size_t(x0) * 4u);
		px[0] = decode_word(a, q.x);
		px[1] = decode_word(a, q.y);
		px[2] = decode_word(a, q.z);
		px[3] = decode_word(a, q.w);
		return;
	}
#pragma unroll
	for (int i = 0; i < DIRECT_PX; i++)
		px[i] = x0 + i < a.in_w ? fetch_texel(a, x0 + i, y) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <int PLANES, bool SUB, bool WIDE>
__global__ __launch_bounds__(256) void k_video_direct(VideoArgs a)
{
	typedef typename Sample<WIDE>::type S;
	constexpr float SCALE = Sample<WIDE>::scale;
	const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * DIRECT_PX;
	const int y0 = (blockIdx.y * DIRECT_ROWS + (threadIdx.x >> 6)) * 2;
	if (x0 >= a.out_w || y0 >= a.out_h)
		return;
	const bool dither = (a.flags & VIDEO_DITHER) != 0;
	float4 px[2][DIRECT_PX];
	load_row4(a, x0, y0, px[0]);
	load_row4(a, x0, y0 + 1, px[1]);
#pragma unroll
	for (int r = 0; r < 2; r++)
#pragma unroll
		for (int i = 0; i < DIRECT_PX; i++)
			px[r][i] = finish_rgb(a, apply_eotf(a, px[r][i]));

	if (PLANES == 1)
	{
#pragma unroll
		for (int r = 0; r < 2; r++)
		{
			if (y0 + r >= a.out_h)
				break;
			uint32_t words[DIRECT_PX];
#pragma unroll
			for (int i = 0; i < DIRECT_PX; i++)
				words[i] = pack_rgba8(a, px[r][i], dither, x0 + i, y0 + r);
			store_run<uint32_t, DIRECT_PX>(a.plane[0] + size_t(y0 + r) * a.pitch[0], x0, a.out_w, words, a.aligned & 1u);
		}
		return;
	}

	float3 ycc[2][DIRECT_PX];
#pragma unroll
	for (int r = 0; r < 2; r++)
#pragma unroll
		for (int i = 0; i < DIRECT_PX; i++)
			ycc[r][i] = to_ycbcr(a, px[r][i]);

#pragma unroll
	for (int r = 0; r < 2; r++)
	{
		if (y0 + r >= a.out_h)
			break;
		S luma[DIRECT_PX];
#pragma unroll
		for (int i = 0; i < DIRECT_PX; i++)
			luma[i] = S(unorm_code(ycc[r][i].y + dither_term(a, dither, x0 + i, y0 + r), SCALE));
		store_run<S, DIRECT_PX>(a.plane[0] + size_t(y0 + r) * a.pitch[0], x0, a.out_w, luma, a.aligned & 1u);
	}

	if (SUB)
	{
		// mean of each 2 x 2 block, summed as the reference's two quad swaps: (p + horizontal) + vertical
		constexpr int NC = DIRECT_PX / 2;
		const int cx0 = x0 >> 1, cy = y0 >> 1;
		S cb[NC], cr[NC];
#pragma unroll
		for (int k = 0; k < NC; k++)
		{
			float sb = (ycc[0][2 * k].x + ycc[0][2 * k + 1].x) + (ycc[1][2 * k].x + ycc[1][2 * k + 1].x);
			float sr = (ycc[0][2 * k].z + ycc[0][2 * k + 1].z) + (ycc[1][2 * k].z + ycc[1][2 * k + 1].z);
			sb *= 0.25f;
			sr *= 0.25f;
			if (dither)
			{
				const float d = dither_term(a, true, cx0 + k, cy);
				sb += d;
				sr += d;
			}
			cb[k] = S(unorm_code(sb, SCALE));
			cr[k] = S(unorm_code(sr, SCALE));
		}
		store_chroma<PLANES, S, NC>(a, cx0, cy, cb, cr);
		return;
	}

#pragma unroll
	for (int r = 0; r < 2; r++)
	{
		if (y0 + r >= a.out_h)
			break;
		S cb[DIRECT_PX], cr[DIRECT_PX];
#pragma unroll
		for (int i = 0; i < DIRECT_PX; i++)
		{
			const float d = dither_term(a, dither, x0 + i, y0 + r);
			cb[i] = S(unorm_code(ycc[r][i].x + d, SCALE));
			cr[i] = S(unorm_code(ycc[r][i].z + d, SCALE));
		}
		store_chroma<PLANES, S, DIRECT_PX>(a, x0, y0 + r, cb, cr);
	}
}

// ---- polyphase rescale -----------------------------------------------------------------------------------------------------
constexpr int TILE = 16;   // outputs per group along each axis
constexpr int STAGE = 41;  // staged input texels per axis: 15 * 2 (scaling_to_input <= 2) + 1 + 8 taps + 2 of rounding slack

// scaler.comp rescale_image: the 8.8 fixed-point input position of output `o`, from the base of its 8 x 8 tile, every
// operation rounded separately ("precise"), int() truncating toward zero.
__device__ __forceinline__ int sample_pos(int o, float s)
{
	const int base = o & ~7;
	const float base_input = __fsub_rn(__fmul_rn(__fadd_rn(float(base), 0.5f), s), 0.5f);
	return int(__fadd_rn(__fmul_rn(float(PHASES), __fadd_rn(base_input, __fmul_rn(s, float(o - base)))), 0.5f));
}

__device__ __forceinline__ float quad_swap(float v, int pattern)
{
	const int bits = __builtin_bit_cast(int, v);
	// quad_perm [1,0,3,2] swaps horizontal neighbours, [2,3,0,1] vertical ones (lane bit 0 = x, bit 1 = y)
	const int r = pattern == 0 ? __builtin_amdgcn_mov_dpp(bits, 0xb1, 0xf, 0xf, false) : __builtin_amdgcn_mov_dpp(bits, 0x4e, 0xf, 0xf, false);
	return __builtin_bit_cast(float, r);
}

__device__ __forceinline__ void load_weights(const uint16_t *table, float (&w)[TAPS])
{
	const u32x4 q = *reinterpret_cast<const u32x4 *>(table);
	const uint32_t words[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
	for (int i = 0; i < 4; i++)
	{
		const f16x2 h = __builtin_bit_cast(f16x2, words[i]);
		w[2 * i] = float(h.x);
		w[2 * i + 1] = float(h.y);
	}
}

__device__ __forceinline__ f16x4 to_half4(float4 v) { return f16x4{_Float16(v.x), _Float16(v.y), _Float16(v.z), _Float16(v.w)}; }

template <int PLANES, bool SUB, bool WIDE>
__global__ __launch_bounds__(256) void k_video_rescale(VideoArgs a)
{
	typedef typename Sample<WIDE>::type S;
	constexpr float SCALE = Sample<WIDE>::scale;
	__shared__ f16x4 staged[STAGE][STAGE + 1];
	__shared__ f16x4 mid[TILE][STAGE + 1];

	const int t = threadIdx.x;
	const int ox0 = blockIdx.x * TILE, oy0 = blockIdx.y * TILE;
	const float sx = a.scaling_to_input[0], sy = a.scaling_to_input[1];
	// the staged window: from 3 taps before the first output's position to 4 after the last one's
	const int first_x = (sample_pos(ox0, sx) >> 8) - 3, first_y = (sample_pos(oy0, sy) >> 8) - 3;
	const int nx = min((sample_pos(ox0 + TILE - 1, sx) >> 8) + 4 - first_x + 1, STAGE);
	const int ny = min((sample_pos(oy0 + TILE - 1, sy) >> 8) + 4 - first_y + 1, STAGE);
	// the width and height of the image the filter reads: the frame, or the virtual prefiltered one at twice the target size
	const bool sampled = (a.flags & VIDEO_SAMPLED) != 0;

	// every lane stages texels (nx * ny <= 41 * 41, at most seven per lane): all loads of a lane are independent and issued together
	for (int i = t; i < nx * ny; i += 256)
	{
		const int r = i / nx, c = i - r * nx;
		const int gx = first_x + c, gy = first_y + r;
		float4 v;
		if (sampled)
		{
			const float u = (float(gx) + 0.5f) * a.inv_input_resolution[0], w = (float(gy) + 0.5f) * a.inv_input_resolution[1];
			v = sample_linear_with([&a](int x, int y) { return fetch_texel(a, x, y); }, a.in_w, a.in_h, u, w);
		}
		else
			v = fetch_texel(a, clampi(gx, 0, a.in_w - 1), clampi(gy, 0, a.in_h - 1));
		staged[r][c] = to_half4(apply_eotf(a, v));
	}
	__syncthreads();

	// vertical: TILE output rows x nx staged columns
	for (int i = t; i < TILE * 64; i += 256)
	{
		const int c = i & 63, r = i >> 6;
		if (c >= nx)
			continue;
		const int pos = sample_pos(oy0 + r, sy);
		float w[TAPS];
		load_weights(a.weights + PHASES * TAPS + (pos & (PHASES - 1)) * TAPS, w);
		const int row0 = (pos >> 8) - 3 - first_y;
		float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
		for (int k = 0; k < TAPS; k++)
		{
			const f16x4 h = staged[clampi(row0 + k, 0, STAGE - 1)][c];
			acc = make_float4(fmaf(float(h.x), w[k], acc.x), fmaf(float(h.y), w[k], acc.y), fmaf(float(h.z), w[k], acc.z), fmaf(float(h.w), w[k], acc.w));
		}
		mid[r][c] = to_half4(acc);
	}
	__syncthreads();

	// horizontal: one output per lane, the four lanes of a quad a 2 x 2 block
	const int q = t >> 2;
	const int lx = 2 * (q & 7) + (t & 1), ly = 2 * (q >> 3) + ((t >> 1) & 1);
	const int ox = ox0 + lx, oy = oy0 + ly;
	const int pos = sample_pos(ox, sx);
	float w[TAPS];
	load_weights(a.weights + (pos & (PHASES - 1)) * TAPS, w);
	const int col0 = (pos >> 8) - 3 - first_x;
	float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
	for (int k = 0; k < TAPS; k++)
	{
		const f16x4 h = mid[ly][clampi(col0 + k, 0, STAGE - 1)];
		v = make_float4(fmaf(float(h.x), w[k], v.x), fmaf(float(h.y), w[k], v.y), fmaf(float(h.z), w[k], v.z), fmaf(float(h.w), w[k], v.w));
	}
	v = finish_rgb(a, v);

	const bool dither = (a.flags & VIDEO_DITHER) != 0;
	const bool inside = ox < a.out_w && oy < a.out_h;
	if (PLANES == 1)
	{
		const uint32_t word = pack_rgba8(a, v, dither, ox, oy);
		if (inside)
			*reinterpret_cast<uint32_t *>(a.plane[0] + size_t(oy) * a.pitch[0] + size_t(ox) * 4u) = word;
		return;
	}

	const float3 ycc = to_ycbcr(a, v);
	if (inside)
	{
		*reinterpret_cast<S *>(a.plane[0] + size_t(oy) * a.pitch[0] + size_t(ox) * sizeof(S)) = S(unorm_code(ycc.y + dither_term(a, dither, ox, oy), SCALE));
	}
	float cb = ycc.x, cr = ycc.z;
	int cx = ox, cy = oy;
	bool write_chroma = true;
	if (SUB)
	{
		cb += quad_swap(cb, 0);
		cr += quad_swap(cr, 0);
		cb += quad_swap(cb, 1);
		cr += quad_swap(cr, 1);
		cb *= 0.25f;
		cr *= 0.25f;
		cx >>= 1;
		cy >>= 1;
		write_chroma = (t & 3) == 0;
	}
	if (!write_chroma || cx >= a.chroma_w || cy >= a.chroma_h)
		return;
	if (dither)
	{
		const float d = dither_term(a, true, cx, cy);
		cb += d;
		cr += d;
	}
	if (PLANES == 2)
	{
		S *p = reinterpret_cast<S *>(a.plane[1] + size_t(cy) * a.pitch[1]) + 2 * cx;
		p[0] = S(unorm_code(cb, SCALE));
		p[1] = S(unorm_code(cr, SCALE));
	}
	else
	{
		*(reinterpret_cast<S *>(a.plane[1] + size_t(cy) * a.pitch[1]) + cx) = S(unorm_code(cb, SCALE));
		*(reinterpret_cast<S *>(a.plane[2] + size_t(cy) * a.pitch[2]) + cx) = S(unorm_code(cr, SCALE));
	}
}

// ---- host: the decisions of VideoScaler::rescale ----------------------------------------------------------------------------
// muglm::floatToHalf: round to nearest, ties away from zero; subnormals; overflow to infinity; NaN kept
uint16_t float_to_half_away(float v)
{
	uint32_t bits;
	memcpy(&bits, &v, 4);
	const uint32_t sign = (bits >> 16) & 0x8000u;
	const int exponent = int((bits >> 23) & 0xffu) - 112;
	uint32_t mantissa = bits & 0x7fffffu;
	if (exponent == 143)
		return uint16_t(sign | 0x7c00u | (mantissa ? ((mantissa >> 13) | ((mantissa >> 13) == 0)) : 0u));
	if (exponent <= 0)
	{
		if (exponent < -10)
			return uint16_t(sign);
		mantissa = (mantissa | 0x800000u) >> (1 - exponent);
		return uint16_t(sign | ((mantissa + 0x1000u) >> 13));
	}
	const uint32_t rounded = ((uint32_t(exponent) << 23) | mantissa) + 0x1000u; // the carry moves into the exponent
	if ((rounded >> 23) > 30)
		return uint16_t(sign | 0x7c00u);
	return uint16_t(sign | (rounded >> 13));
}

float sinc(float v)
{
	v *= 3.14159265358979323846f;
	return fabsf(v) < 0.0001f ? 1.0f : sinf(v) / v;
}

float hann(float v)
{
	v = cosf(0.5f * v * 3.14159265358979323846f);
	return v * v;
}

// VideoScaler::update_weights (scaler.cpp:90-149): Hann-windowed sinc, bandwidth min(1, max(0.5, out / in)) per axis
void build_weights(uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h, uint16_t *out)
{
	const float bw = fminf(fmaxf(float(out_w) / float(in_w), 0.5f), 1.0f);
	const float bh = fminf(fmaxf(float(out_h) / float(in_h), 0.5f), 1.0f);
	for (int phase = 0; phase < PHASES; phase++)
	{
		float wh[TAPS], wv[TAPS], total_h = 0.0f, total_v = 0.0f;
		for (int tap = 0; tap < TAPS; tap++)
		{
			const float l = float(tap - (TAPS / 2 - 1)) - float(phase) / float(PHASES);
			wh[tap] = hann(l / float(TAPS / 2)) * sinc(bw * l);
			wv[tap] = hann(l / float(TAPS / 2)) * sinc(bh * l);
			total_h += wh[tap];
			total_v += wv[tap];
		}
		for (int tap = 0; tap < TAPS; tap++)
		{
			out[phase * TAPS + tap] = float_to_half_away(wh[tap] / total_h);
			out[PHASES * TAPS + phase * TAPS + tap] = float_to_half_away(wv[tap] / total_v);
		}
	}
}

struct Mat3
{
	float c[3][3]; // column major
};

Mat3 mul3(const Mat3 &a, const Mat3 &b)
{
	Mat3 r;
	for (int col = 0; col < 3; col++)
		for (int row = 0; row < 3; row++)
			r.c[col][row] = a.c[0][row] * b.c[col][0] + a.c[1][row] * b.c[col][1] + a.c[2][row] * b.c[col][2];
	return r;
}

Mat3 inverse3(const Mat3 &m)
{
	const float (&a)[3][3] = m.c;
	Mat3 r;
	r.c[0][0] = a[1][1] * a[2][2] - a[2][1] * a[1][2];
	r.c[0][1] = a[2][1] * a[0][2] - a[0][1] * a[2][2];
	r.c[0][2] = a[0][1] * a[1][2] - a[1][1] * a[0][2];
	r.c[1][0] = a[2][0] * a[1][2] - a[1][0] * a[2][2];
	r.c[1][1] = a[0][0] * a[2][2] - a[2][0] * a[0][2];
	r.c[1][2] = a[1][0] * a[0][2] - a[0][0] * a[1][2];
	r.c[2][0] = a[1][0] * a[2][1] - a[2][0] * a[1][1];
	r.c[2][1] = a[2][0] * a[0][1] - a[0][0] * a[2][1];
	r.c[2][2] = a[0][0] * a[1][1] - a[1][0] * a[0][1];
	const float det = a[0][0] * r.c[0][0] + a[1][0] * r.c[0][1] + a[2][0] * r.c[0][2];
	for (auto &col : r.c)
		for (float &e : col)
			e /= det;
	return r;
}

// RGB -> XYZ for chromaticities (x, y) of the primaries and the white point: the construction of host/post/hdr.cpp's
// compute_xyz_matrix.  Not shared with it: that file's inverse multiplies by 1 / det where inverse3 divides by det, the results differ
// in the last bit, and each is pinned by its own CPU test.
Mat3 xyz_matrix(const float (&xy)[4][2])
{
	Mat3 primaries;
	float white[3];
	for (int i = 0; i < 4; i++)
	{
		float *dst = i < 3 ? primaries.c[i] : white;
		dst[0] = xy[i][0] / xy[i][1];
		dst[1] = 1.0f;
		dst[2] = (1.0f - xy[i][0] - xy[i][1]) / xy[i][1];
	}
	const Mat3 inv = inverse3(primaries);
	Mat3 r;
	for (int col = 0; col < 3; col++)
	{
		const float scale = inv.c[0][col] * white[0] + inv.c[1][col] * white[1] + inv.c[2][col] * white[2];
		for (int row = 0; row < 3; row++)
			r.c[col][row] = primaries.c[col][row] * scale;
	}
	return r;
}

// chromaticities of R, G, B and the white point (D65)
const float prim709[4][2] = {{0.640f, 0.330f}, {0.300f, 0.600f}, {0.150f, 0.060f}, {0.3127f, 0.3290f}};
const float prim2020[4][2] = {{0.708f, 0.292f}, {0.170f, 0.797f}, {0.131f, 0.046f}, {0.3127f, 0.3290f}};
const float prim601_625[4][2] = {{0.640f, 0.330f}, {0.290f, 0.600f}, {0.150f, 0.060f}, {0.3127f, 0.3290f}};
const float prim601_525[4][2] = {{0.630f, 0.340f}, {0.310f, 0.595f}, {0.155f, 0.070f}, {0.3127f, 0.3290f}};

bool recognized_color_space(uint32_t space)
{
	return space == GR_COLOR_SPACE_SRGB_NONLINEAR || space == GR_COLOR_SPACE_HDR10_ST2084 || space == GR_COLOR_SPACE_EXTENDED_SRGB_LINEAR;
}

bool is_rgba8_output(uint32_t f)
{
	return f == GR_FORMAT_R8G8B8A8_UNORM || f == GR_FORMAT_R8G8B8A8_SRGB || f == GR_FORMAT_B8G8R8A8_UNORM || f == GR_FORMAT_B8G8R8A8_SRGB;
}

// The plane layout of a YCbCr frame, for plan_video and plan_yuv: chroma planes of the luma plane's size or, with `sub` (each caller's own
// reading of the sizes), half of it rounded up; one interleaved or two of the luma's format; pitches hold a row.  The reason of a refusal, or nullptr.
const char *check_plane_layout(const gr_image *planes, uint32_t num_planes, bool wide, bool sub)
{
	const gr_image &y = planes[0];
	if (num_planes > 1)
	{
		const gr_image &c = planes[1];
		if (sub ? (c.width != (y.width + 1) / 2 || c.height != (y.height + 1) / 2) : (c.width != y.width || c.height != y.height))
			return "chroma planes must have the luma plane's size or half of it, rounded up";
		const uint32_t want = num_planes == 2 ? (wide ? GR_FORMAT_R16G16_UNORM : GR_FORMAT_R8G8_UNORM) : y.format;
		for (uint32_t i = 1; i < num_planes; i++)
			if (planes[i].format != want || planes[i].width != c.width || planes[i].height != c.height)
				return "chroma plane format or size does not match the luma plane";
	}
	for (uint32_t i = 0; i < num_planes; i++)
		if (gr_image_layout_rule(&planes[i], planes[i].format))
			return "a plane's pitch_bytes does not hold its rows";
	return nullptr;
}

// Checks the arguments and fills the plan; returns the reason of a refusal, or nullptr.
const char *plan_video(const gr_image *in, const gr_image *planes, uint32_t num_planes, uint32_t in_space, uint32_t out_space, gr_video_plan *p)
{
	if (!in || !planes || !p)
		return "null argument";
	if (!recognized_color_space(in_space) || !recognized_color_space(out_space))
		return "unrecognised color space";
	if (num_planes < 1 || num_planes > 3)
		return "num_planes must be 1, 2 or 3";
	if (num_planes > 1 && out_space == GR_COLOR_SPACE_EXTENDED_SRGB_LINEAR)
		return "only nonlinear output color spaces are supported for YCbCr";
	if (in->format != GR_FORMAT_R8G8B8A8_UNORM && in->format != GR_FORMAT_R8G8B8A8_SRGB && in->format != GR_FORMAT_A2B10G10R10_UNORM_PACK32 &&
	    in->format != GR_FORMAT_R16G16B16A16_SFLOAT)
		return "input format must be R8G8B8A8_{UNORM,SRGB}, A2B10G10R10_UNORM_PACK32 or R16G16B16A16_SFLOAT";
	if (in->width > 65535 || in->height > 65535 || gr_image_layout_rule(in, in->format))
		return "bad input extent or pitch";
	const gr_image &y = planes[0];
	if (!y.width || !y.height || y.width > 65535 || y.height > 65535)
		return "bad output extent";
	if (num_planes == 1 && !is_rgba8_output(y.format))
		return "a single output plane must be R8G8B8A8 or B8G8R8A8";
	const bool wide = y.format == GR_FORMAT_R16_UNORM;
	if (num_planes > 1 && y.format != GR_FORMAT_R8_UNORM && !wide)
		return "the luma plane must be R8_UNORM or R16_UNORM";
	// 4:2:0 by the width alone, as VideoScaler::rescale: a frame one pixel wide is refused, which plan_yuv accepts, on purpose
	// (test_plan_refuses_invalid_conversions in tests/test_video_scaler_cpu.py, assert_refused in tests/test_gpu_video_scaler.py).
	const bool sub = num_planes > 1 && planes[1].width < y.width;
	if (const char *why = check_plane_layout(planes, num_planes, wide, sub))
		return why;

	memset(p, 0, sizeof(*p));
	p->num_planes = num_planes;
	gr_push_video &push = p->push;
	push.resolution[0] = int32_t(in->width);
	push.resolution[1] = int32_t(in->height);
	push.scaling_to_input[0] = float(in->width) / float(y.width);
	push.scaling_to_input[1] = float(in->height) / float(y.height);
	const bool sampled = push.scaling_to_input[0] > 2.0f || push.scaling_to_input[1] > 2.0f;
	push.scaling_to_input[0] = fminf(push.scaling_to_input[0], 2.0f);
	push.scaling_to_input[1] = fminf(push.scaling_to_input[1], 2.0f);
	push.inv_input_resolution[0] = 1.0f / (float(y.width) * push.scaling_to_input[0]);
	push.inv_input_resolution[1] = 1.0f / (float(y.height) * push.scaling_to_input[1]);

	uint32_t flags = 0, eotf = GR_VIDEO_TRANSFER_IDENTITY, oetf = GR_VIDEO_TRANSFER_IDENTITY;
	if (in_space == GR_COLOR_SPACE_SRGB_NONLINEAR && in->format != GR_FORMAT_R8G8B8A8_SRGB)
		eotf = GR_VIDEO_TRANSFER_SRGB;
	else if (in_space == GR_COLOR_SPACE_HDR10_ST2084)
		eotf = GR_VIDEO_TRANSFER_PQ;
	if (out_space == GR_COLOR_SPACE_SRGB_NONLINEAR)
		oetf = GR_VIDEO_TRANSFER_SRGB;
	else if (out_space == GR_COLOR_SPACE_HDR10_ST2084)
		oetf = GR_VIDEO_TRANSFER_PQ;
	if (in->width == y.width && in->height == y.height)
		flags |= GR_VIDEO_CONTROL_SKIP_RESCALE_BIT;
	if (push.scaling_to_input[0] > 1.0f || push.scaling_to_input[1] > 1.0f)
		flags |= GR_VIDEO_CONTROL_DOWNSCALING_BIT;
	if (sampled)
		flags |= GR_VIDEO_CONTROL_SAMPLED_DOWNSCALING_BIT;
	if (in_space != out_space)
		flags |= GR_VIDEO_CONTROL_PRIMARY_CONVERSION_BIT;
	flags |= GR_VIDEO_CONTROL_CLAMP_COORD_BIT;
	if (sub)
		flags |= GR_VIDEO_CONTROL_CHROMA_SUBSAMPLE_BIT;
	if (is_rgba8_output(y.format))
	{
		flags |= GR_VIDEO_CONTROL_DITHER_BIT;
		push.dither_strength = 1.0f / 255.0f;
	}
	if (oetf == eotf && (flags & GR_VIDEO_CONTROL_SKIP_RESCALE_BIT))
		eotf = oetf = GR_VIDEO_TRANSFER_IDENTITY;
	p->flags = flags;
	p->eotf = eotf;
	p->oetf = oetf;

	// full-range BT.2020 for an HDR10 output, BT.709 for everything else (scaler.cpp:306-318); rows Cr, Y, Cb
	static const float bt2020[12] = {0.5f, -0.459786f, -0.0402143f, 0.5f, 0.2627f, 0.678f, 0.0593f, 0.0f, -0.13963f, -0.36037f, 0.5f, 0.5f};
	static const float bt709[12] = {0.5f, -0.454153f, -0.0458471f, 0.5f, 0.2126f, 0.7152f, 0.0722f, 0.0f, -0.114572f, -0.385428f, 0.5f, 0.5f};
	memcpy(p->gamma_space_transform, out_space == GR_COLOR_SPACE_HDR10_ST2084 ? bt2020 : bt709, sizeof(bt709));

	if (in_space != out_space)
	{
		const Mat3 to_out = inverse3(xyz_matrix(out_space == GR_COLOR_SPACE_HDR10_ST2084 ? prim2020 : prim709));
		const Mat3 from_in = xyz_matrix(in_space == GR_COLOR_SPACE_HDR10_ST2084 ? prim2020 : prim709);
		const Mat3 conv = mul3(to_out, from_in);
		float sdr_scale = 1.0f;
		if (in_space == GR_COLOR_SPACE_SRGB_NONLINEAR)
			sdr_scale = 200.0f;
		else if (in_space == GR_COLOR_SPACE_EXTENDED_SRGB_LINEAR)
			sdr_scale = 80.0f;
		if (out_space == GR_COLOR_SPACE_EXTENDED_SRGB_LINEAR)
			sdr_scale /= 80.0f;
		for (int col = 0; col < 3; col++)
			for (int row = 0; row < 3; row++)
				p->primary_transform[3 * col + row] = sdr_scale * conv.c[col][row];
	}
	else
	{
		p->primary_transform[0] = p->primary_transform[4] = p->primary_transform[8] = 1.0f;
	}
	return nullptr;
}

// launch(<PLANES>, <SUB>, <WIDE>) with the constants of k_video_direct / k_video_rescale: nine instantiations per kernel, a single plane
// (RGBA8) being neither subsampled nor wide.  False, and no call, for any other combination.
template <typename F> bool with_plane_layout(uint32_t num_planes, bool sub, bool wide, F &&launch)
{
	switch (num_planes)
	{
	case 1: return !sub && !wide && (launch(std::integral_constant<int, 1>{}, std::false_type{}, std::false_type{}), true);
	case 2: return with_flags([&](auto s, auto w) { launch(std::integral_constant<int, 2>{}, s, w); }, sub, wide), true;
	case 3: return with_flags([&](auto s, auto w) { launch(std::integral_constant<int, 3>{}, s, w); }, sub, wide), true;
	default: return false;
	}
}
} // namespace

extern "C" int gr_video_scaler_weights(uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h, uint16_t *out)
{
	if (!out || !in_w || !in_h || !out_w || !out_h)
		return GR_ERR_INVALID_ARGUMENT;
	build_weights(in_w, in_h, out_w, out_h, out);
	return GR_OK;
}

extern "C" int gr_video_scale_plan(const gr_image *input, const gr_image *planes, uint32_t num_planes, uint32_t input_color_space,
                                   uint32_t output_color_space, gr_video_plan *plan)
{
	return plan_video(input, planes, num_planes, input_color_space, output_color_space, plan) ? GR_ERR_INVALID_ARGUMENT : GR_OK;
}

extern "C" int gr_video_scale(gr_ctx *ctx, gr_stream stream, const gr_image *input, const gr_image *planes, uint32_t num_planes,
                              uint32_t input_color_space, uint32_t output_color_space)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	gr_video_plan plan;
	if (const char *why = plan_video(input, planes, num_planes, input_color_space, output_color_space, &plan))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_video_scale: %s", why);
	GR_CHECK_ARG(ctx, input->ptr);
	for (uint32_t i = 0; i < num_planes; i++)
		GR_CHECK_ARG(ctx, planes[i].ptr);

	VideoArgs a = {};
	a.in = static_cast<const uint8_t *>(input->ptr);
	a.in_w = int(input->width);
	a.in_h = int(input->height);
	a.in_pitch = input->pitch_bytes;
	a.in_kind = input->format == GR_FORMAT_R8G8B8A8_SRGB ? IN_RGBA8_SRGB
	            : input->format == GR_FORMAT_A2B10G10R10_UNORM_PACK32 ? IN_A2B10G10R10
	            : input->format == GR_FORMAT_R16G16B16A16_SFLOAT ? IN_RGBA16F : IN_RGBA8;
	for (uint32_t i = 0; i < num_planes; i++)
	{
		a.plane[i] = static_cast<uint8_t *>(planes[i].ptr);
		a.pitch[i] = planes[i].pitch_bytes;
		a.aligned |= is_aligned(&planes[i], 16u) ? 1u << i : 0u;
	}
	a.aligned |= is_aligned(input, 16u) ? 8u : 0u;
	a.out_w = int(planes[0].width);
	a.out_h = int(planes[0].height);
	a.chroma_w = num_planes > 1 ? int(planes[1].width) : 0;
	a.chroma_h = num_planes > 1 ? int(planes[1].height) : 0;
	a.flags = plan.flags;
	a.eotf = plan.eotf;
	a.oetf = plan.oetf;
	a.swap_rb = planes[0].format == GR_FORMAT_B8G8R8A8_UNORM || planes[0].format == GR_FORMAT_B8G8R8A8_SRGB;
	memcpy(a.gst, plan.gamma_space_transform, sizeof(a.gst));
	memcpy(a.prim, plan.primary_transform, sizeof(a.prim));
	memcpy(a.scaling_to_input, plan.push.scaling_to_input, sizeof(a.scaling_to_input));
	memcpy(a.inv_input_resolution, plan.push.inv_input_resolution, sizeof(a.inv_input_resolution));
	a.dither_strength = plan.push.dither_strength;
	a.srgb_lut = ctx->srgb_decode_lut;

	const bool sub = (plan.flags & GR_VIDEO_CONTROL_CHROMA_SUBSAMPLE_BIT) != 0;
	const bool wide = planes[0].format == GR_FORMAT_R16_UNORM;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "video_scale"};
	bool launched;
	if (plan.flags & GR_VIDEO_CONTROL_SKIP_RESCALE_BIT)
	{
		const dim3 grid(gr_div_up(planes[0].width, 64 * DIRECT_PX), gr_div_up(planes[0].height, 2 * DIRECT_ROWS)), block(256);
		launched = with_plane_layout(num_planes, sub, wide, [&](auto n, auto sb, auto wd) {
			hipLaunchKernelGGL((k_video_direct<n.value, sb.value, wd.value>), grid, block, 0, s, a);
		});
	}
	else
	{
		// the fp16 weight table of these sizes (update_weights): built once per size combination and kept for the context's lifetime,
		// so that a launch still in flight on another stream never sees its table rewritten.  Lookup and build happen under the lock
		// (one table per key); the upload is a copy on this stream from pinned memory, and a launch on another stream waits for it.
		const uint64_t key = (uint64_t(input->width) << 48) | (uint64_t(input->height) << 32) | (uint64_t(planes[0].width) << 16) | planes[0].height;
		void *table = nullptr;
		hipEvent_t ready = nullptr;
		bool built = false;
		{
			std::unique_lock<std::mutex> holder{ctx->lock};
			auto it = ctx->video_weights.find(key);
			if (it == ctx->video_weights.end())
			{
				gr_ctx::VideoWeights w;
				const size_t bytes = 2 * PHASES * TAPS * sizeof(uint16_t);
				if (hipMalloc(&w.device, bytes) != hipSuccess || hipHostMalloc(&w.host, bytes, hipHostMallocDefault) != hipSuccess ||
				    hipEventCreateWithFlags(&w.ready, hipEventDisableTiming) != hipSuccess)
				{
					(void)hipFree(w.device);
					(void)hipHostFree(w.host);
					holder.unlock();
					return ctx->fail(GR_ERR_OUT_OF_MEMORY, "gr_video_scale: weight table allocation failed");
				}
				build_weights(input->width, input->height, planes[0].width, planes[0].height, static_cast<uint16_t *>(w.host));
				if (hipMemcpyAsync(w.device, w.host, bytes, hipMemcpyHostToDevice, s) != hipSuccess || hipEventRecord(w.ready, s) != hipSuccess)
				{
					holder.unlock();
					return ctx->fail(GR_ERR_HIP, "gr_video_scale: weight table upload failed");
				}
				it = ctx->video_weights.emplace(key, w).first;
				built = true;
			}
			table = it->second.device;
			ready = it->second.ready;
		}
		if (!built && hipEventQuery(ready) != hipSuccess)
			GR_CHECK_HIP(ctx, hipStreamWaitEvent(s, ready, 0));
		a.weights = static_cast<const uint16_t *>(table);
		const dim3 grid(gr_div_up(planes[0].width, TILE), gr_div_up(planes[0].height, TILE)), block(256);
		launched = with_plane_layout(num_planes, sub, wide, [&](auto n, auto sb, auto wd) {
			hipLaunchKernelGGL((k_video_rescale<n.value, sb.value, wd.value>), grid, block, 0, s, a);
		});
	}
	if (!launched)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_video_scale: unsupported plane layout");
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

// ---- playback: YCbCr planes -> RGB -------------------------------------------------------------------------------------------
// VideoDecoder::Impl::init_yuv_to_rgb / dispatch_conversion (video/ffmpeg_decode.cpp) + assets/shaders/util/yuv_to_rgb.comp.  The
// reference runs one invocation per output pixel with a nearest sampler on the luma plane and LinearClamp ones on the chroma planes;
// here k_yuv_to_rgb is a pure stream shaped like k_video_direct: one lane converts 4 x 2 pixels, i.e. whole 2 x 2 chroma footprints
// of a 4:2:0 frame: one 4-B luma load per row (8 B at 16 bits), the chroma taps filtered in software over the linear planes with
// the library's sampler model (sample_linear_with: exact fp32 weights, 2^-8 texel snap), and one 16-B store per row (two for
// RGBA16F).  The chroma coordinate keeps the shader's order -- min((coord + siting) * inv_resolution, chroma_clamp), then times the
// plane's own size -- because the chroma plane of an odd-sized 4:2:0 frame is ceil(n / 2) texels wide: the ratio is not 0.5.
// Unaligned pointers or pitches, and the last columns of a row, go element by element.  Everything in fp32; no LDS.
namespace
{
enum YuvOut : int
{
	YUV_OUT_RGBA8 = 0,
	YUV_OUT_A2B10G10R10 = 1,
	YUV_OUT_RGBA16F = 2, // with the PQ specialization: EOTF + primary conversion instead of the dither
};

struct YuvArgs
{
	const uint8_t *plane[3];
	uint32_t pitch[3];
	int w, h;           // resolution: the luma plane's and the output's size
	int cw, ch;         // chroma plane size
	uint8_t *out;
	uint32_t out_pitch;
	uint32_t aligned;   // bit 0: the luma plane's pointer and pitch are multiples of 16 B (vector loads); bit 3: the output's (vector stores)
	uint32_t nv21;
	float m[12];        // yuv_to_rgb, row major 3 x 4: R, G, B of [Y Cb Cr 1]
	float prim[9];      // primary_conversion, column major 3 x 3
	float inv_resolution[2], chroma_siting[2], chroma_clamp[2];
	float unorm_rescale;
};

template <bool WIDE> __device__ __forceinline__ float unorm_sample(uint32_t v)
{
	return WIDE ? float(v) * (1.0f / 65535.0f) : unorm8_to_float(v);
}

// four luma samples of one row from x0 (a multiple of 4); samples beyond the row read as zero and are never stored
template <bool WIDE>
__device__ __forceinline__ void load_luma4(const YuvArgs &a, int x0, int y, float (&v)[DIRECT_PX])
{
	typedef typename Sample<WIDE>::type S;
	const S *row = reinterpret_cast<const S *>(a.plane[0] + size_t(y) * a.pitch[0]);
	if ((a.aligned & 1u) && x0 + DIRECT_PX <= a.w)
	{
		if (WIDE)
		{
			const u32x2 q = *reinterpret_cast<const u32x2 *>(row + x0);
			v[0] = unorm_sample<true>(q.x & 0xffffu);
			v[1] = unorm_sample<true>(q.x >> 16);
			v[2] = unorm_sample<true>(q.y & 0xffffu);
			v[3] = unorm_sample<true>(q.y >> 16);
		}
		else
		{
			const uint32_t q = *reinterpret_cast<const uint32_t *>(row + x0);
#pragma unroll
			for (int i = 0; i < DIRECT_PX; i++)
				v[i] = unorm_sample<false>((q >> (8 * i)) & 255u);
		}
		return;
	}
#pragma unroll
	for (int i = 0; i < DIRECT_PX; i++)
		v[i] = x0 + i < a.w ? unorm_sample<WIDE>(row[x0 + i]) : 0.0f;
}

// one chroma texel (x, y inside the plane) as (first channel, second channel): the two planes of a three-plane frame, or the pair of
// an interleaved one
template <int PLANES, bool WIDE>
__device__ __forceinline__ float4 fetch_chroma(const YuvArgs &a, int x, int y)
{
	typedef typename Sample<WIDE>::type S;
	if (PLANES == 3)
	{
		const S u = reinterpret_cast<const S *>(a.plane[1] + size_t(y) * a.pitch[1])[x];
		const S v = reinterpret_cast<const S *>(a.plane[2] + size_t(y) * a.pitch[2])[x];
		return make_float4(unorm_sample<WIDE>(u), unorm_sample<WIDE>(v), 0.0f, 0.0f);
	}
	const S *p = reinterpret_cast<const S *>(a.plane[1] + size_t(y) * a.pitch[1]) + 2 * x;
	return make_float4(unorm_sample<WIDE>(p[0]), unorm_sample<WIDE>(p[1]), 0.0f, 0.0f);
}

// yuv_to_rgb.comp's EOTF: ST 2084 to scRGB units (80 nits = 1)
__device__ __forceinline__ float pq_to_scrgb(float v) { return pq_eotf(v) * (1.0f / 80.0f); }

// R, G, B + d as BITS-wide codes from bit 0 up, `alpha` in the bits above them: an RGBA8 (8) or A2B10G10R10 (10) word
template <int BITS>
__device__ __forceinline__ uint32_t pack_unorm_rgb(const float (&rgb)[3], float d, uint32_t alpha)
{
	constexpr float SCALE = float((1 << BITS) - 1);
	return unorm_code(rgb[0] + d, SCALE) | (unorm_code(rgb[1] + d, SCALE) << BITS) | (unorm_code(rgb[2] + d, SCALE) << (2 * BITS)) | (alpha << (3 * BITS));
}

template <int PLANES, bool WIDE, int OUT>
__global__ __launch_bounds__(256) void k_yuv_to_rgb(YuvArgs a)
{
	const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * DIRECT_PX;
	const int y0 = (blockIdx.y * DIRECT_ROWS + (threadIdx.x >> 6)) * 2;
	if (x0 >= a.w || y0 >= a.h)
		return;

	float luma[2][DIRECT_PX];
	load_luma4<WIDE>(a, x0, y0, luma[0]);
	if (y0 + 1 < a.h)
		load_luma4<WIDE>(a, x0, y0 + 1, luma[1]);

#pragma unroll
	for (int r = 0; r < 2; r++)
	{
		const int y = y0 + r;
		if (y >= a.h)
			break;
		uint32_t words[DIRECT_PX], words_hi[DIRECT_PX]; // RGBA16F: R G / B A
#pragma unroll
		for (int i = 0; i < DIRECT_PX; i++)
		{
			const int x = min(x0 + i, a.w - 1); // columns beyond the row repeat the last one and are dropped by the store
			float cb = 128.0f / 255.0f, cr = 128.0f / 255.0f;
			if (PLANES > 1)
			{
				const float u = fminf((float(x) + a.chroma_siting[0]) * a.inv_resolution[0], a.chroma_clamp[0]);
				const float v = fminf((float(y) + a.chroma_siting[1]) * a.inv_resolution[1], a.chroma_clamp[1]);
				const float4 c = sample_linear_with([&a](int cx, int cy) { return fetch_chroma<PLANES, WIDE>(a, cx, cy); }, a.cw, a.ch, u, v);
				cb = a.nv21 ? c.y : c.x;
				cr = a.nv21 ? c.x : c.y;
			}
			const float yy = luma[r][i] * a.unorm_rescale;
			cb *= a.unorm_rescale;
			cr *= a.unorm_rescale;
			float rgb[3];
#pragma unroll
			for (int k = 0; k < 3; k++)
				rgb[k] = saturatef(fmaf(a.m[4 * k], yy, fmaf(a.m[4 * k + 1], cb, fmaf(a.m[4 * k + 2], cr, a.m[4 * k + 3]))));

			if (OUT == YUV_OUT_RGBA16F)
			{
				const float lr = pq_to_scrgb(rgb[0]), lg = pq_to_scrgb(rgb[1]), lb = pq_to_scrgb(rgb[2]);
				const float4 o = make_float4(a.prim[0] * lr + a.prim[3] * lg + a.prim[6] * lb, a.prim[1] * lr + a.prim[4] * lg + a.prim[7] * lb,
				                             a.prim[2] * lr + a.prim[5] * lg + a.prim[8] * lb, 1.0f);
				const u32x2 h = __builtin_bit_cast(u32x2, pack_rgba16f(o));
				words[i] = h.x;
				words_hi[i] = h.y;
			}
			else
			{
				const float d = dither_at(x, y) * (1.0f / 255.0f);
				words[i] = OUT == YUV_OUT_A2B10G10R10 ? pack_unorm_rgb<10>(rgb, d, 3u) : pack_unorm_rgb<8>(rgb, d, 255u);
			}
		}
		uint8_t *row = a.out + size_t(y) * a.out_pitch;
		if (OUT == YUV_OUT_RGBA16F)
		{
			const uint32_t lo[4] = {words[0], words_hi[0], words[1], words_hi[1]}, hi[4] = {words[2], words_hi[2], words[3], words_hi[3]};
			store_run<uint32_t, 4>(row, 2 * x0, 2 * a.w, lo, a.aligned & 8u);
			store_run<uint32_t, 4>(row, 2 * x0 + 4, 2 * a.w, hi, a.aligned & 8u);
		}
		else
			store_run<uint32_t, DIRECT_PX>(row, x0, a.w, words, a.aligned & 8u);
	}
}

// ---- host: the decisions of init_yuv_to_rgb and dispatch_conversion -----------------------------------------------------------------
struct Mat4
{
	float c[4][4]; // column major
};

Mat4 identity4()
{
	Mat4 r = {};
	for (int i = 0; i < 4; i++)
		r.c[i][i] = 1.0f;
	return r;
}

// columns of a * b summed in column order, one rounding per operation (the order of muglm's mat4 * vec4)
Mat4 mul4(const Mat4 &a, const Mat4 &b)
{
	Mat4 r;
	for (int col = 0; col < 4; col++)
		for (int row = 0; row < 4; row++)
			r.c[col][row] = a.c[0][row] * b.c[col][0] + a.c[1][row] * b.c[col][1] + a.c[2][row] * b.c[col][2] + a.c[3][row] * b.c[col][3];
	return r;
}

Mat4 widen(const Mat3 &m)
{
	Mat4 r = identity4();
	for (int col = 0; col < 3; col++)
		for (int row = 0; row < 3; row++)
			r.c[col][row] = m.c[col][row];
	return r;
}

const char *plan_yuv(const gr_image *planes, uint32_t num_planes, const gr_image *out, const gr_video_yuv_info *info, struct gr_video_yuv_plan *p)
{
	if (!planes || !out || !info || !p)
		return "null argument";
	if (num_planes < 1 || num_planes > 3)
		return "num_planes must be 1, 2 or 3";
	const gr_image &y = planes[0];
	if (!y.width || !y.height || y.width > 65535 || y.height > 65535)
		return "bad luma extent";
	const bool wide = y.format == GR_FORMAT_R16_UNORM;
	if (y.format != GR_FORMAT_R8_UNORM && !wide)
		return "the luma plane must be R8_UNORM or R16_UNORM";
	if (info->bit_depth != 8 && info->bit_depth != 10 && info->bit_depth != 16)
		return "bit_depth must be 8, 10 or 16";
	if ((info->bit_depth == 8) == wide)
		return "8 bits need R8 planes, 10 and 16 bits R16 planes";
	if (info->matrix > GR_VIDEO_MATRIX_SMPTE240M)
		return "unknown matrix";
	if (info->chroma_location > GR_VIDEO_CHROMA_BOTTOM)
		return "unknown chroma location";
	if (info->nv21 && num_planes != 2)
		return "nv21 needs two planes";
	// 4:2:0 by the width or the height: a frame one pixel wide is accepted, which plan_video refuses, on purpose
	// (test_plan_accepts_one_pixel_wide_420 in tests/test_yuv_ref_cpu.py, the 1 x 2 cases of test_edge_sizes in tests/test_gpu_yuv_to_rgb.py).
	const bool sub = num_planes > 1 && (planes[1].width < y.width || planes[1].height < y.height);
	if (const char *why = check_plane_layout(planes, num_planes, wide, sub))
		return why;
	const bool rgba8 = out->format == GR_FORMAT_R8G8B8A8_UNORM || out->format == GR_FORMAT_R8G8B8A8_SRGB;
	if (!rgba8 && out->format != GR_FORMAT_A2B10G10R10_UNORM_PACK32 && out->format != GR_FORMAT_R16G16B16A16_SFLOAT)
		return "output format must be R8G8B8A8_{UNORM,SRGB}, A2B10G10R10_UNORM_PACK32 or R16G16B16A16_SFLOAT";
	if (rgba8 == (info->pq != 0))
		return "PQ content goes to A2B10G10R10 (left encoded) or R16G16B16A16_SFLOAT, everything else to R8G8B8A8";
	if (out->width != y.width || out->height != y.height)
		return "the output must have the luma plane's size";
	if (gr_image_layout_rule(out, out->format))
		return "output pitch_bytes does not hold its rows";

	memset(p, 0, sizeof(*p));
	p->spec_pq = out->format == GR_FORMAT_R16G16B16A16_SFLOAT;
	p->spec_num_planes = num_planes;
	p->spec_nv21 = info->nv21 != 0;
	gr_push_yuv_to_rgb &push = p->push;
	push.resolution[0] = y.width;
	push.resolution[1] = y.height;
	push.inv_resolution[0] = 1.0f / float(y.width);
	push.inv_resolution[1] = 1.0f / float(y.height);
	const float half_texel = 0.5f * float(1u << (sub ? 1 : 0));
	push.chroma_clamp[0] = (float(y.width) - half_texel) * push.inv_resolution[0];
	push.chroma_clamp[1] = (float(y.height) - half_texel) * push.inv_resolution[1];
	static const float sitings[6][2] = {{0.5f, 0.5f}, {1.0f, 0.5f}, {1.0f, 1.0f}, {0.5f, 1.0f}, {1.0f, 0.0f}, {0.5f, 0.0f}};
	push.chroma_siting[0] = sitings[info->chroma_location][0];
	push.chroma_siting[1] = sitings[info->chroma_location][1];
	push.unorm_rescale = info->bit_depth != 10 ? 1.0f : info->msb_aligned ? float(0xffff) / float(1023 << 6) : float(0xffff) / float(1023);

	// Vulkan 16.3.9 / Khronos Data Format Specification 15.1.1: bias and narrow-range scale for the bit depth
	const int depth = int(info->bit_depth);
	const int luma_offset = (info->full_range ? 0 : 16) << (depth - 8);
	const int luma_narrow_range = 219 << (depth - 8), chroma_narrow_range = 224 << (depth - 8);
	const float midpoint = float(1 << (depth - 1));
	const float unorm_range = float((1 << depth) - 1);
	const float unorm_divider = 1.0f / unorm_range;
	const float chroma_shift = -midpoint * unorm_divider;
	const float luma_scale = unorm_range / float(luma_narrow_range), chroma_scale = unorm_range / float(chroma_narrow_range);
	const float bias[3] = {float(-luma_offset) * unorm_divider, chroma_shift, chroma_shift};
	const float scale[3] = {info->full_range ? 1.0f : luma_scale, info->full_range ? 1.0f : chroma_scale, info->full_range ? 1.0f : chroma_scale};

	uint32_t matrix = info->matrix;
	if (matrix == GR_VIDEO_MATRIX_UNSPECIFIED)
		matrix = y.height < 625 ? GR_VIDEO_MATRIX_BT601_525 : y.height < 720 ? GR_VIDEO_MATRIX_BT601_625 : y.height < 2160 ? GR_VIDEO_MATRIX_BT709 : GR_VIDEO_MATRIX_BT2020;
	p->matrix = matrix;

	// columns: what Y, Cb and Cr contribute to (R, G, B)
	Mat3 m = {};
	const float (*source)[4][2] = nullptr;
	m.c[0][0] = m.c[0][1] = m.c[0][2] = 1.0f;
	switch (matrix)
	{
	case GR_VIDEO_MATRIX_BT2020:
		m.c[1][1] = -0.11156702f / 0.6780f;
		m.c[1][2] = 1.8814f;
		m.c[2][0] = 1.4746f;
		m.c[2][1] = -0.38737742f / 0.6780f;
		source = &prim2020;
		break;
	case GR_VIDEO_MATRIX_BT601_525:
	case GR_VIDEO_MATRIX_BT601_625:
		m.c[1][1] = -0.202008f / 0.587f;
		m.c[1][2] = 1.772f;
		m.c[2][0] = 1.402f;
		m.c[2][1] = -0.419198f / 0.587f;
		source = matrix == GR_VIDEO_MATRIX_BT601_625 ? &prim601_625 : &prim601_525;
		break;
	case GR_VIDEO_MATRIX_SMPTE240M:
		m.c[1][1] = -0.58862f / 0.701f;
		m.c[1][2] = 1.826f;
		m.c[2][0] = 1.576f;
		m.c[2][1] = -0.334112f / 0.701f;
		source = &prim601_525;
		break;
	default: // BT.709: sRGB shares its primaries
		m.c[1][1] = -0.13397432f / 0.7152f;
		m.c[1][2] = 1.8556f;
		m.c[2][0] = 1.5748f;
		m.c[2][1] = -0.33480248f / 0.7152f;
		break;
	}
	const Mat4 conversion = source ? widen(mul3(inverse3(xyz_matrix(prim709)), xyz_matrix(*source))) : identity4();
	Mat4 scaling = identity4(), translation = identity4();
	for (int i = 0; i < 3; i++)
	{
		scaling.c[i][i] = scale[i];
		translation.c[3][i] = bias[i];
	}
	const Mat4 to_rgb = mul4(mul4(widen(m), scaling), translation);
	memcpy(push.yuv_to_rgb, to_rgb.c, sizeof(push.yuv_to_rgb));
	memcpy(push.primary_conversion, conversion.c, sizeof(push.primary_conversion));
	return nullptr;
}
} // namespace

extern "C" int gr_video_yuv_plan(const gr_image *planes, uint32_t num_planes, const gr_image *out, const gr_video_yuv_info *info,
                                 struct gr_video_yuv_plan *plan)
{
	return plan_yuv(planes, num_planes, out, info, plan) ? GR_ERR_INVALID_ARGUMENT : GR_OK;
}

extern "C" int gr_video_yuv_to_rgb(gr_ctx *ctx, gr_stream stream, const gr_image *planes, uint32_t num_planes, const gr_image *out,
                                   const gr_video_yuv_info *info)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	struct gr_video_yuv_plan plan;
	if (const char *why = plan_yuv(planes, num_planes, out, info, &plan))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_video_yuv_to_rgb: %s", why);
	GR_CHECK_ARG(ctx, out->ptr);
	for (uint32_t i = 0; i < num_planes; i++)
		GR_CHECK_ARG(ctx, planes[i].ptr);

	YuvArgs a = {};
	for (uint32_t i = 0; i < num_planes; i++)
	{
		a.plane[i] = static_cast<const uint8_t *>(planes[i].ptr);
		a.pitch[i] = planes[i].pitch_bytes;
	}
	a.w = int(planes[0].width);
	a.h = int(planes[0].height);
	a.cw = num_planes > 1 ? int(planes[1].width) : 0;
	a.ch = num_planes > 1 ? int(planes[1].height) : 0;
	a.out = static_cast<uint8_t *>(out->ptr);
	a.out_pitch = out->pitch_bytes;
	a.aligned = (is_aligned(&planes[0], 16u) ? 1u : 0u) | (is_aligned(out, 16u) ? 8u : 0u);
	a.nv21 = plan.spec_nv21;
	const gr_push_yuv_to_rgb &push = plan.push;
	for (int row = 0; row < 3; row++)
		for (int col = 0; col < 4; col++)
			a.m[4 * row + col] = push.yuv_to_rgb[4 * col + row];
	for (int col = 0; col < 3; col++)
		for (int row = 0; row < 3; row++)
			a.prim[3 * col + row] = push.primary_conversion[4 * col + row];
	memcpy(a.inv_resolution, push.inv_resolution, sizeof(a.inv_resolution));
	memcpy(a.chroma_siting, push.chroma_siting, sizeof(a.chroma_siting));
	memcpy(a.chroma_clamp, push.chroma_clamp, sizeof(a.chroma_clamp));
	a.unorm_rescale = push.unorm_rescale;

	const bool wide = planes[0].format == GR_FORMAT_R16_UNORM;
	const int kind = out->format == GR_FORMAT_R16G16B16A16_SFLOAT ? YUV_OUT_RGBA16F : out->format == GR_FORMAT_A2B10G10R10_UNORM_PACK32 ? YUV_OUT_A2B10G10R10 : YUV_OUT_RGBA8;
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "video_yuv_to_rgb"};
	const dim3 grid(gr_div_up(planes[0].width, 64 * DIRECT_PX), gr_div_up(planes[0].height, 2 * DIRECT_ROWS)), block(256);
	bool launched = false; // <PLANES 1..3, WIDE, OUT 0..2>: all 18 combinations exist
	with_index<3>(int(num_planes) - 1, [&](auto n) {
		launched = with_index<3>(kind, [&](auto o) {
			with_flags([&](auto wd) { hipLaunchKernelGGL((k_yuv_to_rgb<n.value + 1, wd.value, o.value>), grid, block, 0, s, a); }, wide);
		});
	});
	if (!launched)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_video_yuv_to_rgb: unsupported plane layout");
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
