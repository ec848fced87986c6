// Follows MIT-licensed work (Granite, (c) 2015-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// FFT (renderer/fft/fft.{hpp,cpp} semantics): the plan, the butterflies, the index maps and the twiddle indexing.  Shared by the gfx950
// kernels (fft.hip) and by a host build that runs the same passes one lane at a time (tests/cpp/fft_core_host.cpp): the kernels add
// the barriers between the phases below and the launch, nothing else.  Written from the algorithm (Stockham autosort), DESIGN.md 7.9.
//
// One C2C pass of radix R along dimension d, cumulative radix p, T = N / R:   for every j in [0, T), k = j mod p,
//     u[t] = in[j + t T] * W_N^(t k N / (p R)),   v = DFT_R(u),   out[(j - k) R + k + t p] = v[t],   t in [0, R).
// A workgroup takes `columns` adjacent (j, x, y, z) columns, holds their R points in LDS and computes DFT_R there by the same
// recurrence with radices 4 and 8 in registers.  W_N^m = exp(dir 2 pi i m / N) is one table over the full circle, computed in double
// and rounded once; every twiddle any pass needs is an entry of it.  Arithmetic and LDS are fp32 for both data types; FP16 is the
// type of memory (user buffers, images and the scratch between passes).
#pragma once
#include "core_base.hpp"

namespace gr_fft
{
using gr_core::float_to_half;
using gr_core::half_to_float;

constexpr uint32_t GROUP = 512u;          // lanes of a workgroup
constexpr uint32_t TILE_ELEMENTS = 8192u; // complex numbers a workgroup holds at most (64 KiB of fp32 pairs)
constexpr uint32_t REGS = TILE_ELEMENTS / GROUP;
constexpr uint32_t MAX_COLUMNS = 512u;
constexpr uint32_t LDS_LIMIT = 80u * 1024u; // two workgroups share a CU's 160 KiB
constexpr uint32_t ROW_SINGLE_LOG2 = 12u;   // a row of up to 4096 points is one pass
constexpr uint32_t MAX_PASSES = 16u, MAX_SUBS = 6u;
constexpr uint32_t RESOLVE_GROUP = 256u;
constexpr uint32_t MAX_IMAGE_EXTENT = 65536u;

enum Mode : uint32_t { FORWARD_C2C = 0, INVERSE_C2C = 1, R2C = 2, C2R = 3 };
enum DataType : uint32_t { FP32 = 0, FP16 = 1 };
enum ResourceType : uint32_t { TEXTURE = 0, BUFFER = 1 };
enum PassKind : uint32_t { PASS_C2C = 0, PASS_R2C_RESOLVE = 1, PASS_C2R_RESOLVE = 2 };
enum BufferId : uint32_t { BUF_SRC = 0, BUF_DST = 1, BUF_SCRATCH_A = 2, BUF_SCRATCH_B = 3 };
// complex pairs / real scalars, fp32 / fp16, linear buffer / image
enum ViewKind : uint32_t { VIEW_C32 = 0, VIEW_C16 = 1, VIEW_R32 = 2, VIEW_R16 = 3, VIEW_IMG_C32 = 4, VIEW_IMG_C16 = 5, VIEW_IMG_R32 = 6, VIEW_IMG_R16 = 7 };

struct alignas(8) c32
{
	float x, y;
};
GR_HD c32 operator+(c32 a, c32 b) { return {a.x + b.x, a.y + b.y}; }
GR_HD c32 operator-(c32 a, c32 b) { return {a.x - b.x, a.y - b.y}; }
GR_HD c32 cmul(c32 a, c32 b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
GR_HD c32 conj(c32 a) { return {a.x, -a.y}; }
// a * (dir i)
GR_HD c32 rot(c32 a, float dir) { return {-dir * a.y, dir * a.x}; }

GR_HD c32 unpack_half2(uint32_t v) { return {half_to_float(v & 0xffffu), half_to_float(v >> 16)}; }
GR_HD uint32_t pack_half2(c32 v) { return float_to_half(v.x) | (float_to_half(v.y) << 16); }

// ---- plan -------------------------------------------------------------------------------------------------------------------
struct Options
{
	uint32_t nx, ny, nz, dimensions, mode, data_type, input_resource, output_resource;
};

// One side of a pass.  Offsets count "units": complex numbers for the complex kinds, scalars for the real kinds (where a complex
// column x is the scalar pair 2 x, 2 x + 1).  For an image the unit is a packed coordinate x | y << 16.
struct View
{
	uint8_t *ptr;
	uint32_t kind;
	uint32_t x_stride, row_stride, layer_stride;
	uint32_t width, height, pitch_bytes;
	int32_t offset_x, offset_y;
};

struct Pass
{
	uint32_t kind, dim;
	uint32_t n, radix, p, t;         // length along dim, R, cumulative radix before this pass, T = n / R
	uint32_t log2_radix, log2_t;
	uint32_t columns, log2_columns;  // columns a workgroup holds
	uint32_t total_columns;
	uint32_t cols, ny, nz;           // extents of the array this pass walks (cols: complex columns of a row)
	uint32_t in_t_fastest, out_t_fastest;
	uint32_t sub_count, sub_radix[MAX_SUBS];
	uint32_t table_n;
	uint32_t lds_stride, lds_bytes, group, grid;
	uint32_t reads, writes;
	float dir;
	View in, out;
	const c32 *twiddle;
};

struct Plan
{
	Options options;
	uint32_t count;
	Pass passes[MAX_PASSES];
	uint32_t table_n;
	float dir;
	uint32_t real, half_cols;                                  // R2C / C2R; Nx / 2
	uint32_t scratch_row_stride, scratch_count;
	uint64_t scratch_elements;
};

inline bool is_pow2(uint32_t v) { return v && !(v & (v - 1u)); }
inline uint32_t log2_of(uint32_t v)
{
	uint32_t l = 0;
	while ((1u << l) < v)
		l++;
	return l;
}
GR_HD uint32_t lds_at(const Pass &P, uint32_t c, uint32_t t) { return c * P.lds_stride + t + (t >> 5); }

inline View linear_view(uint32_t kind, uint32_t row_stride, uint32_t layer_stride)
{
	View v = {};
	v.kind = kind;
	v.x_stride = (kind == VIEW_R32 || kind == VIEW_R16) ? 2u : 1u;
	v.row_stride = row_stride;
	v.layer_stride = layer_stride;
	return v;
}

// 0, or -1 for options that are refused (everything the reference's plan() returns false for, texture input, and sizes the index
// arithmetic does not cover).
inline int build_plan(const Options &o, Plan &plan)
{
	plan = {};
	plan.options = o;
	if (o.dimensions < 1 || o.dimensions > 3 || o.mode > C2R || o.data_type > FP16 || o.input_resource > BUFFER || o.output_resource > BUFFER)
		return -1;
	if (o.nx == 0 || o.ny == 0 || o.nz == 0)
		return -1;
	const bool real = o.mode == R2C || o.mode == C2R, fp16 = o.data_type == FP16, image = o.output_resource == TEXTURE;
	if (o.input_resource == TEXTURE)
		return -1;
	if (image && (o.nz > 1 || (real && o.dimensions < 2)))
		return -1;
	if (!is_pow2(o.nx))
		return -1;
	const uint32_t n0 = real ? o.nx >> 1 : o.nx;
	if (n0 < 4)
		return -1;
	if (o.dimensions >= 2 && (!is_pow2(o.ny) || o.ny < 4))
		return -1;
	if (o.dimensions >= 3 && (!is_pow2(o.nz) || o.nz < 4))
		return -1;
	// 2^31 elements or more; factor by factor, so that no product of three 32-bit extents wraps
	if (o.nx >= (1u << 31) || uint64_t(o.nx) * o.ny >= (1ull << 31) || uint64_t(o.nx) * o.ny * o.nz >= (1ull << 31))
		return -1;
	const uint32_t half_cols = o.nx >> 1;
	if (image && ((real ? half_cols + 1u : o.nx) > MAX_IMAGE_EXTENT || o.ny > MAX_IMAGE_EXTENT))
		return -1;

	plan.real = real;
	plan.half_cols = half_cols;
	plan.dir = (o.mode == FORWARD_C2C || o.mode == R2C) ? -1.0f : 1.0f;
	plan.table_n = o.nx;
	if (o.dimensions >= 2 && o.ny > plan.table_n)
		plan.table_n = o.ny;
	if (o.dimensions >= 3 && o.nz > plan.table_n)
		plan.table_n = o.nz;
	plan.scratch_row_stride = real ? ((half_cols + 1u + 15u) & ~15u) : o.nx;
	plan.scratch_elements = uint64_t(plan.scratch_row_stride) * o.ny * o.nz;
	if (plan.scratch_elements >= (1ull << 31))
		return -1;

	const uint32_t extent[3] = {n0, o.ny, o.nz};
	const uint32_t min_columns = fp16 ? 16u : 8u; // a 64-byte run of the memory type
	const uint32_t wide_log2 = log2_of(TILE_ELEMENTS / min_columns);

	auto add_resolve = [&](uint32_t kind) {
		Pass &P = plan.passes[plan.count++];
		P.kind = kind;
		P.dim = 0;
		P.n = o.nx;
		P.cols = kind == PASS_R2C_RESOLVE ? half_cols + 1u : half_cols; // columns written
		P.ny = o.ny;
		P.nz = o.nz;
		P.group = RESOLVE_GROUP;
		P.grid = uint32_t((uint64_t(P.cols) * o.ny * o.nz + RESOLVE_GROUP - 1u) / RESOLVE_GROUP);
	};
	auto add_dim = [&](uint32_t dim, uint32_t cols) {
		const uint32_t n = extent[dim], bits = log2_of(n);
		uint32_t count = 1;
		if (!(dim == 0 && bits <= ROW_SINGLE_LOG2))
			count = (bits + wide_log2 - 1u) / wide_log2;
		uint32_t p = 1;
		for (uint32_t i = 0; i < count; i++)
		{
			Pass &P = plan.passes[plan.count++];
			P.kind = PASS_C2C;
			P.dim = dim;
			P.n = n;
			P.log2_radix = bits / count + (i < bits % count ? 1u : 0u);
			P.radix = 1u << P.log2_radix;
			P.p = p;
			P.t = n / P.radix;
			P.log2_t = log2_of(P.t);
			P.cols = cols;
			P.ny = o.ny;
			P.nz = o.nz;
			const uint64_t total = dim == 0 ? uint64_t(P.t) * o.ny * o.nz : dim == 1 ? uint64_t(cols) * P.t * o.nz : uint64_t(cols) * o.ny * P.t;
			P.total_columns = uint32_t(total);
			P.in_t_fastest = dim == 0 && P.t == 1;
			P.out_t_fastest = dim == 0 && p == 1;
			const uint32_t floor_columns = (P.in_t_fastest && P.out_t_fastest) ? 1u : min_columns;
			uint32_t columns = TILE_ELEMENTS / P.radix;
			if (columns > MAX_COLUMNS)
				columns = MAX_COLUMNS;
			// small problems: narrower tiles until there are workgroups for every CU several times over, but never so narrow that a
			// radix-8 step leaves lanes without a butterfly (GROUP * 8 points)
			while (columns > floor_columns && columns * P.radix > GROUP * 8u && (total + columns - 1u) / columns < 1024u)
				columns >>= 1;
			P.columns = columns;
			P.log2_columns = log2_of(columns);
			uint32_t left = P.log2_radix;
			while (left % 3u)
			{
				P.sub_radix[P.sub_count++] = 4;
				left -= 2;
			}
			for (; left; left -= 3)
				P.sub_radix[P.sub_count++] = 8;
			P.lds_stride = (P.radix + (P.radix >> 5)) | 1u;
			P.lds_bytes = columns * P.lds_stride * 8u + 3u * columns * 4u;
			P.group = GROUP;
			P.grid = uint32_t((total + columns - 1u) / columns);
			p *= P.radix;
		}
	};

	if (o.mode == C2R)
	{
		for (uint32_t dim = o.dimensions; dim-- > 1;)
			add_dim(dim, half_cols + 1u);
		add_resolve(PASS_C2R_RESOLVE);
		add_dim(0, half_cols);
	}
	else
	{
		add_dim(0, n0);
		if (o.mode == R2C)
			add_resolve(PASS_R2C_RESOLVE);
		for (uint32_t dim = 1; dim < o.dimensions; dim++)
			add_dim(dim, real ? half_cols + 1u : o.nx);
	}

	const uint32_t scratch_kind = fp16 ? VIEW_C16 : VIEW_C32;
	plan.scratch_count = plan.count >= 3 ? 2u : plan.count - 1u;
	for (uint32_t i = 0; i < plan.count; i++)
	{
		Pass &P = plan.passes[i];
		P.table_n = plan.table_n;
		P.dir = plan.dir;
		P.reads = i == 0 ? uint32_t(BUF_SRC) : BUF_SCRATCH_A + ((i - 1u) & 1u);
		P.writes = i + 1u == plan.count ? uint32_t(BUF_DST) : BUF_SCRATCH_A + (i & 1u);
		P.in = linear_view(scratch_kind, plan.scratch_row_stride, plan.scratch_row_stride * o.ny);
		P.out = P.in;
		if (P.lds_bytes > LDS_LIMIT)
			return -1;
	}
	return 0;
}

// The user's side of the first and the last pass.  `real_side`: scalars (R2C input, C2R output).
inline uint32_t user_view_kind(const Options &o, bool output)
{
	const bool fp16 = o.data_type == FP16;
	const bool real_side = output ? o.mode == C2R : o.mode == R2C;
	const bool image = output && o.output_resource == TEXTURE;
	return (image ? 4u : 0u) + (real_side ? 2u : 0u) + (fp16 ? 1u : 0u);
}
// Units of a row the pass chain touches on a user buffer: Nx scalars on a real side; Nx / 2 + 1 complex numbers on the complex side
// of a real transform; Nx complex numbers otherwise.
inline uint32_t user_row_units(const Options &o, bool output)
{
	const bool real = o.mode == R2C || o.mode == C2R;
	const bool real_side = output ? o.mode == C2R : o.mode == R2C;
	return real_side ? o.nx : (real ? (o.nx >> 1) + 1u : o.nx);
}
inline uint32_t view_unit_bytes(uint32_t kind)
{
	switch (kind & 3u)
	{
	case VIEW_C32: return 8;
	case VIEW_C16: return 4;
	case VIEW_R32: return 4;
	default: return 2;
	}
}

// table[m] = exp(dir 2 pi i m / n), m in [0, n): computed in double, rounded once.
inline void build_twiddles(c32 *table, uint32_t n, float dir)
{
	for (uint32_t m = 0; m < n; m++)
	{
		const double theta = 2.0 * 3.14159265358979323846 * double(dir) * (double(m) / double(n));
		table[m] = {float(cos(theta)), float(sin(theta))};
	}
}

// ---- memory -----------------------------------------------------------------------------------------------------------------
GR_HD c32 view_load(const View &v, uint32_t at)
{
	switch (v.kind)
	{
	case VIEW_C32:
		return reinterpret_cast<const c32 *>(v.ptr)[at];
	case VIEW_C16:
		return unpack_half2(reinterpret_cast<const uint32_t *>(v.ptr)[at]);
	case VIEW_R32:
	{
		const float *f = reinterpret_cast<const float *>(v.ptr) + at;
		return {f[0], f[1]};
	}
	default: // VIEW_R16: even strides, so `at` is even
		return unpack_half2(reinterpret_cast<const uint32_t *>(v.ptr)[at >> 1]);
	}
}

GR_HD void view_store(const View &v, uint32_t at, c32 value)
{
	switch (v.kind)
	{
	case VIEW_C32:
		reinterpret_cast<c32 *>(v.ptr)[at] = value;
		break;
	case VIEW_C16:
		reinterpret_cast<uint32_t *>(v.ptr)[at] = pack_half2(value);
		break;
	case VIEW_R32:
	{
		float *f = reinterpret_cast<float *>(v.ptr) + at;
		f[0] = value.x;
		f[1] = value.y;
		break;
	}
	case VIEW_R16:
		reinterpret_cast<uint32_t *>(v.ptr)[at >> 1] = pack_half2(value);
		break;
	default:
	{
		// image: `at` is x | y << 16 in complex columns; a store outside the image is dropped
		const bool real = v.kind >= VIEW_IMG_R32, half = v.kind & 1u;
		const int32_t px = int32_t((at & 0xffffu) * (real ? 2u : 1u)) + v.offset_x, py = int32_t(at >> 16) + v.offset_y;
		if (py < 0 || py >= int32_t(v.height))
			break;
		uint8_t *row = v.ptr + size_t(py) * v.pitch_bytes;
		if (!real)
		{
			if (px < 0 || px >= int32_t(v.width))
				break;
			if (half)
				reinterpret_cast<uint32_t *>(row)[px] = pack_half2(value);
			else
				reinterpret_cast<c32 *>(row)[px] = value;
			break;
		}
		for (int32_t i = 0; i < 2; i++)
		{
			const int32_t tx = px + i;
			const float s = i ? value.y : value.x;
			if (tx < 0 || tx >= int32_t(v.width))
				continue;
			if (half)
				reinterpret_cast<uint16_t *>(row)[tx] = uint16_t(float_to_half(s));
			else
				reinterpret_cast<float *>(row)[tx] = s;
		}
		break;
	}
	}
}

GR_HD bool view_is_image(const View &v) { return v.kind >= VIEW_IMG_C32; }
GR_HD uint32_t view_at(const View &v, uint32_t x, uint32_t y, uint32_t z)
{
	if (view_is_image(v))
		return x | (y << 16);
	return x * v.x_stride + y * v.row_stride + z * v.layer_stride;
}
GR_HD uint32_t view_dim_stride(const View &v, uint32_t dim)
{
	if (view_is_image(v))
		return dim == 0 ? 1u : 65536u;
	return dim == 0 ? v.x_stride : (dim == 1 ? v.row_stride : v.layer_stride);
}

// ---- butterflies ------------------------------------------------------------------------------------------------------------
GR_HD void butterfly4(c32 &a0, c32 &a1, c32 &a2, c32 &a3, float dir)
{
	const c32 t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = rot(a1 - a3, dir);
	a0 = t0 + t2;
	a1 = t1 + t3;
	a2 = t0 - t2;
	a3 = t1 - t3;
}
GR_HD void butterfly8(c32 *a, float dir)
{
	c32 e0 = a[0], e1 = a[2], e2 = a[4], e3 = a[6], o0 = a[1], o1 = a[3], o2 = a[5], o3 = a[7];
	butterfly4(e0, e1, e2, e3, dir);
	butterfly4(o0, o1, o2, o3, dir);
	constexpr float H = 0.70710678118654752440f;
	o1 = cmul(o1, c32{H, dir * H});
	o2 = rot(o2, dir);
	o3 = cmul(o3, c32{-H, dir * H});
	a[0] = e0 + o0;
	a[4] = e0 - o0;
	a[1] = e1 + o1;
	a[5] = e1 - o1;
	a[2] = e2 + o2;
	a[6] = e2 - o2;
	a[3] = e3 + o3;
	a[7] = e3 - o3;
}

// ---- the phases of a C2C pass; a barrier stands between each two ------------------------------------------------------------
// LDS: columns x lds_stride complex numbers, then per column: input offset, output offset, k = j mod p.
GR_HD uint32_t *column_table(const Pass &P, c32 *lds) { return reinterpret_cast<uint32_t *>(lds + P.columns * P.lds_stride); }
GR_HD uint32_t valid_columns(const Pass &P, uint32_t group)
{
	const uint32_t first = group * P.columns, left = P.total_columns - first;
	return left < P.columns ? left : P.columns;
}

GR_HD void phase_columns(const Pass &P, c32 *lds, uint32_t group, uint32_t lane)
{
	uint32_t *table = column_table(P, lds);
	const uint32_t valid = valid_columns(P, group);
	for (uint32_t c = lane; c < valid; c += GROUP)
	{
		const uint32_t q = group * P.columns + c;
		uint32_t xyz[3] = {0, 0, 0}, j;
		if (P.dim == 0)
		{
			j = q & (P.t - 1u);
			const uint32_t rest = q >> P.log2_t;
			xyz[1] = rest % P.ny;
			xyz[2] = rest / P.ny;
		}
		else if (P.dim == 1)
		{
			xyz[0] = q % P.cols;
			const uint32_t rest = q / P.cols;
			j = rest & (P.t - 1u);
			xyz[2] = rest >> P.log2_t;
		}
		else
		{
			xyz[0] = q % P.cols;
			const uint32_t rest = q / P.cols;
			xyz[1] = rest % P.ny;
			j = rest / P.ny;
		}
		const uint32_t k = j & (P.p - 1u);
		uint32_t in[3] = {xyz[0], xyz[1], xyz[2]}, out[3] = {xyz[0], xyz[1], xyz[2]};
		in[P.dim] = j;
		out[P.dim] = ((j - k) << P.log2_radix) + k;
		table[c] = view_at(P.in, in[0], in[1], in[2]);
		table[P.columns + c] = view_at(P.out, out[0], out[1], out[2]);
		table[2u * P.columns + c] = k;
	}
}

GR_HD void tile_element(const Pass &P, bool t_fastest, uint32_t e, uint32_t &c, uint32_t &t)
{
	if (t_fastest)
	{
		t = e & (P.radix - 1u);
		c = e >> P.log2_radix;
	}
	else
	{
		c = e & (P.columns - 1u);
		t = e >> P.log2_columns;
	}
}

GR_HD void phase_load(const Pass &P, c32 *lds, uint32_t group, uint32_t lane)
{
	const uint32_t *table = column_table(P, lds);
	const uint32_t valid = valid_columns(P, group);
	const uint32_t step = P.t * view_dim_stride(P.in, P.dim), scale = P.table_n / (P.p * P.radix);
	for (uint32_t e = lane; e < P.columns * P.radix; e += GROUP)
	{
		uint32_t c, t;
		tile_element(P, P.in_t_fastest, e, c, t);
		if (c >= valid)
			continue;
		c32 v = view_load(P.in, table[c] + t * step);
		if (P.p > 1u)
			v = cmul(v, P.twiddle[t * table[2u * P.columns + c] * scale]);
		lds[lds_at(P, c, t)] = v;
	}
}

// One radix-RADIX step of the R-point transforms in LDS, cumulative local radix `local_p`: read and compute ...
template <uint32_t RADIX> GR_HD void phase_butterflies(const Pass &P, uint32_t local_p, const c32 *lds, c32 *regs, uint32_t lane)
{
	constexpr uint32_t LOG2 = RADIX == 8u ? 3u : 2u, PER_LANE = REGS / RADIX;
	const uint32_t per_column_log2 = P.log2_radix - LOG2, per_column = 1u << per_column_log2;
	const uint32_t total = P.columns << per_column_log2, scale = P.table_n / (local_p * RADIX);
GR_UNROLL
	for (uint32_t i = 0; i < PER_LANE; i++)
	{
		const uint32_t g = lane + i * GROUP;
		if (g < total)
		{
			const uint32_t c = g >> per_column_log2, b = g & (per_column - 1u), k = b & (local_p - 1u);
			c32 a[RADIX];
GR_UNROLL
			for (uint32_t m = 0; m < RADIX; m++)
			{
				a[m] = lds[lds_at(P, c, b + m * per_column)];
				if (m > 0u && local_p > 1u)
					a[m] = cmul(a[m], P.twiddle[m * k * scale]);
			}
			if (RADIX == 8u)
				butterfly8(a, P.dir);
			else
				butterfly4(a[0], a[1], a[2], a[3], P.dir);
GR_UNROLL
			for (uint32_t m = 0; m < RADIX; m++)
				regs[i * RADIX + m] = a[m];
		}
	}
}
// ... and, after every lane has read, write.
template <uint32_t RADIX> GR_HD void phase_scatter(const Pass &P, uint32_t local_p, c32 *lds, const c32 *regs, uint32_t lane)
{
	constexpr uint32_t LOG2 = RADIX == 8u ? 3u : 2u, PER_LANE = REGS / RADIX;
	const uint32_t per_column_log2 = P.log2_radix - LOG2, per_column = 1u << per_column_log2;
	const uint32_t total = P.columns << per_column_log2;
GR_UNROLL
	for (uint32_t i = 0; i < PER_LANE; i++)
	{
		const uint32_t g = lane + i * GROUP;
		if (g < total)
		{
			const uint32_t c = g >> per_column_log2, b = g & (per_column - 1u), k = b & (local_p - 1u);
			const uint32_t first = ((b - k) << LOG2) + k;
GR_UNROLL
			for (uint32_t m = 0; m < RADIX; m++)
				lds[lds_at(P, c, first + m * local_p)] = regs[i * RADIX + m];
		}
	}
}

GR_HD void phase_store(const Pass &P, const c32 *lds, uint32_t group, uint32_t lane)
{
	const uint32_t *table = column_table(P, const_cast<c32 *>(lds));
	const uint32_t valid = valid_columns(P, group);
	const uint32_t step = P.p * view_dim_stride(P.out, P.dim);
	for (uint32_t e = lane; e < P.columns * P.radix; e += GROUP)
	{
		uint32_t c, t;
		tile_element(P, P.out_t_fastest, e, c, t);
		if (c >= valid)
			continue;
		view_store(P.out, table[P.columns + c] + t * step, lds[lds_at(P, c, t)]);
	}
}

// ---- resolve passes: one output column per lane -----------------------------------------------------------------------------
// R2C: Z = the Nx / 2-point transform of the row read as pairs; X[k] = E[k] + W^k O[k], k in [0, Nx / 2].
// C2R: Z'[k] = (X[k] + conj X[Nx / 2 - k]) + i W^k (X[k] - conj X[Nx / 2 - k]), k in [0, Nx / 2): twice the packed spectrum, so that the
//      unnormalised inverse gives Nx x.
GR_HD void resolve_element(const Pass &P, uint32_t index)
{
	const uint32_t total = P.cols * P.ny * P.nz;
	if (index >= total)
		return;
	const uint32_t k = index % P.cols, rest = index / P.cols, y = rest % P.ny, z = rest / P.ny;
	const uint32_t half = P.n >> 1;
	const c32 w = P.twiddle[k * (P.table_n / P.n)];
	if (P.kind == PASS_R2C_RESOLVE)
	{
		const c32 a = view_load(P.in, view_at(P.in, k & (half - 1u), y, z));
		const c32 b = conj(view_load(P.in, view_at(P.in, (half - k) & (half - 1u), y, z)));
		const c32 even = a + b, d = a - b, odd = cmul(w, c32{d.y, -d.x}); // -i d
		view_store(P.out, view_at(P.out, k, y, z), c32{0.5f * (even.x + odd.x), 0.5f * (even.y + odd.y)});
	}
	else
	{
		c32 a = view_load(P.in, view_at(P.in, k, y, z));
		c32 b = conj(view_load(P.in, view_at(P.in, half - k, y, z)));
		if (k == 0u) // the DC and Nyquist columns of a real signal's spectrum are real: their imaginary parts are not read
			a.y = b.y = 0.0f;
		const c32 d = a - b, odd = cmul(w, c32{-d.y, d.x}); // i d
		view_store(P.out, view_at(P.out, k, y, z), a + b + odd);
	}
}
} // namespace gr_fft
