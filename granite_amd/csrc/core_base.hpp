// The scalar helpers every *_core.hpp header starts from, stated once for the gfx950 kernels (hipcc), for the stand-alone host programs the
// CPU tests build from the same headers (g++) and for the host emulation of tests/cpp/hip_emu.hpp: the host + device function macro, fp16
// conversion, the sampler's linear_axis rule, integer clamp and wrap, the UNORM8 decode and a three-float vector.  A per-feature header
// keeps its own namespace and names what it takes with `using gr_core::...;`.  Nothing else belongs here: arithmetic that only one feature
// has stays in that feature's header.  tests/test_core_base_cpu.py holds the two fp16 conversions to numpy's over every half code.
//
// Left where they are on purpose -- equal results from different code, or different results that the reference prescribes:
//   - device_common.hpp's clampi, min(max(v, lo), hi): the device-only form.  The ternary form below gives the same value but other
//     device code in every kernel that samples through it (post.hip, hiz.hip);
//   - sample_linear_with and every bilinear or trilinear combine (env_core, cacao_core, ocean_core, decal_core, aa.hip, lighting.hip,
//     ssr.hip): their operation orders differ on purpose;
//   - Granite::floatToHalf (host/math.cpp, muglm's ties-upward rounding) and float_to_half_away (video.hip);
//   - the UNORM8 and sRGB encodes (encode_unorm8, aa::unorm8_encode, gr_cacao::to_unorm8, fsr.hip, aa.hip);
//   - lighting.hip's fma-chained dot, ssr.hip's float3_, device_vec.hpp;
//   - gr_fft::cmul and gr_ocean::cmul: fft.hip is built with contraction on, and operand order matters there.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GR_HD __host__ __device__ __forceinline__
#define GR_UNROLL _Pragma("unroll")
#else
#define GR_HD inline
#define GR_UNROLL
#endif

namespace gr_core
{
constexpr float SAMPLER_SNAP = 1.0f / 256.0f;

struct f3
{
	float x, y, z;
};
GR_HD f3 make3(float x, float y, float z) { return {x, y, z}; }
GR_HD f3 operator+(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
GR_HD f3 operator*(f3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
GR_HD float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
GR_HD f3 cross3(f3 a, f3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
GR_HD float length3(f3 a) { return sqrtf(dot3(a, a)); }
GR_HD f3 normalize3(f3 a)
{
	const float inv = 1.0f / sqrtf(dot3(a, a));
	return a * inv;
}

GR_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// Euclidean modulo: -1 is n - 1
GR_HD int wrapi(int v, int n)
{
	v %= n;
	return v < 0 ? v + n : v;
}

// f = unnormalised coordinate - 0.5: index of the first texel and weight of the second (oracle_common.h: linear_axis).  A coordinate
// within 2^-8 of a texel centre reads that texel alone.
GR_HD void linear_axis(float f, int &i0, float &weight)
{
	const float fl = floorf(f + SAMPLER_SNAP);
	float a = f - fl;
	if (a < SAMPLER_SNAP)
		a = 0.0f;
	i0 = int(fl);
	weight = a;
}

// UNORM8 -> float: v / 255 for an integer v in [0, 255], bit-identical to the IEEE quotient for all 256 inputs
// (tests/test_oracle_kat.py) at two VALU operations instead of a full division: 1 / 255 split into its fp32 rounding and
// the remainder, v * hi + fl(v * lo) with one rounding at the end.
GR_HD float unorm8_to_float(uint32_t v)
{
	const float f = float(v);
	const float hi = 0x1.010102p-8f, lo = -0x1.fdfdfep-33f;
	return fmaf(f, hi, f * lo);
}

// ---- fp16: the hardware conversion on the device, the same function in software on the host ------------------------------------
GR_HD float half_to_float(uint32_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return float(__builtin_bit_cast(_Float16, uint16_t(h)));
#else
	const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
	uint32_t bits;
	if (e == 0)
	{
		const float v = float(m) * 5.9604644775390625e-08f; // m * 2^-24
		memcpy(&bits, &v, 4);
		bits |= s;
	}
	else if (e == 31)
		bits = s | 0x7f800000u | (m << 13);
	else
		bits = s | ((e + 112u) << 23) | (m << 13);
	float f;
	memcpy(&f, &bits, 4);
	return f;
#endif
}

// round to nearest even, as v_cvt_f16_f32 and the oracle's float_to_half_rne
GR_HD uint32_t float_to_half(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return uint32_t(__builtin_bit_cast(uint16_t, _Float16(f)));
#else
	uint32_t u;
	memcpy(&u, &f, 4);
	const uint32_t s = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
	if (a >= 0x7f800000u)
		return s | 0x7c00u | (a > 0x7f800000u ? (0x200u | ((a >> 13) & 0x3ffu)) : 0u);
	if (a >= 0x477ff000u)
		return s | 0x7c00u;
	if (a < 0x38800000u)
	{
		if (a < 0x33000000u)
			return s;
		const uint32_t e = a >> 23, m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e; // 14 .. 24
		const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
		return s | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
	}
	const uint32_t r = a - 0x38000000u; // rebias 127 -> 15
	const uint32_t q = r >> 13, rem = r & 0x1fffu;
	return s | (q + ((rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ? 1u : 0u));
#endif
}

// The fp16 store conversion of a value that is an fp32 result first, as the shaders' are.  On the device the value is pinned in a
// register before it is converted: otherwise the compiler fuses a multiply and the conversion behind it into one mixed-precision
// instruction that rounds the exact product once, to fp16, and a store differs from the shader's in its last bit now and then.
GR_HD uint32_t float_to_half_pinned(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
	asm("" : "+v"(f));
#endif
	return float_to_half(f);
}
} // namespace gr_core
