// Follows MIT-licensed work (FidelityFX CACAO, (c) 2016 Intel Corporation, modifications (c) 2021 Advanced Micro Devices, Inc.; Granite
// integration (c) 2022-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// SSAO as the reference runs it (renderer/post/ssao.cpp -> ffx-cacao/src/ffx_cacao.hlsl): native resolution, normals from the G-buffer,
// shader quality level 3 (adaptive) or 2.  This header holds the host restatement of the constant block (ffx_cacao.cpp), the workspace
// layout, the per-texel arithmetic of every stage and the kernels themselves; cacao.hip adds the argument checks and the launches.  The
// same text is compiled for the host (tests/cpp/cacao_core_host.cpp under tests/cpp/hip_emu.hpp) and held to tests/cacao_ref.py before a
// device runs it.  Both builds use -ffp-contract=off and correctly rounded fp32 division and square root.
//
// Rules that the text of the shader does not settle, each stated once here and once in tests/cacao_ref.py:
//   - Samplers are what ffx_cacao_impl.cpp:513-562 creates.  g_PointClampSampler and g_PointMirrorSampler filter LINEARLY (nearest mip),
//     g_LinearClampSampler is linear, g_ViewspaceDepthTapSampler is nearest / nearest mip / clamp.
//   - Linear filtering is the project's model: per axis linear_axis(u * size - 0.5) -- exact fp32 weights, a coordinate within 2^-8 of a
//     texel centre reads that texel alone --, the four texels joined by two lerps along x, t * (1 - a) + t' * a, then one along y; a
//     weight of exactly 0 does not read its texel.
//   - A gather ignores the filter: it returns the texels (i0, j0 + 1), (i0 + 1, j0 + 1), (i0 + 1, j0), (i0, j0) as x, y, z, w, with
//     i0, j0 the first texel of linear_axis, plus the offset.
//   - Nearest: texel floor(u * size), clamped to the level; nearest mip: ceil(lod + 0.5) - 1, clamped to [0, 3].
//   - Clamp addressing clamps the texel index; mirrored repeat reflects it about the edge (-1 -> 0, n -> n - 1, period 2 n).
//   - A texel load (Load, operator[]) outside the image returns zero; an image store outside the image is dropped.  Mip k of an extent
//     n is max(1, n >> k): the prepare shader stores mip k at coord >> k, which overruns an odd extent, so those stores are guarded here.
//   - min16float is RelaxedPrecision in the reference's blobs (cs_6_2 without 16-bit types): evaluated in fp32, rounded to fp16 exactly
//     where the shader packs with f32tof16 -- every LDS store of the blur.
//   - normalize(v) is v / sqrt(dot(v, v)); dot and mul sum left to right; round() is to nearest even; max, min and saturate return the
//     operand that is not NaN.  Only pow and log2 are library functions.
//   - UNORM8 loads are v / 255, SNORM8 loads max(v / 127, -1), the 10-bit UNORM load v / 1023; UNORM8 stores are
//     uint(saturate(c) * 255 + 0.5) as everywhere in this project, SNORM8 stores floor(clamp(c, -1, 1) * 127 + 0.5).
#pragma once
#include "core_base.hpp"
#include "../../include/granite_hip.h"

namespace gr_cacao
{
using gr_core::clampi;
using gr_core::float_to_half_pinned; // f32tof16 of a value that is an fp32 result first
using gr_core::half_to_float;
using gr_core::linear_axis;

constexpr uint32_t PASSES = 4u, DEPTH_MIPS = 4u;
constexpr int MAX_TAPS = 32, ADAPTIVE_BASE_TAPS = 5, ADAPTIVE_FLEXIBLE_TAPS = MAX_TAPS - ADAPTIVE_BASE_TAPS, Q2_TAPS = 12;
constexpr float HALOING_REDUCTION_AMOUNT = 0.6f, NORMAL_EDGES_DOT_THRESHOLD = 0.5f, DEPTH_MIPS_GLOBAL_OFFSET = -4.3f;
constexpr uint32_t WORKSPACE_ALIGN = 256u;

// g_FFX_CACAO_samplePatternMain (ffx_cacao.hlsl:25-35): offset x, y, weight, log2 of the offset's length.  A constant array: the device
// build keeps it in constant memory.
static constexpr float SAMPLE_PATTERN[MAX_TAPS][4] = {
	{0.78488064f, 0.56661671f, 1.500000f, -0.126083f},   {0.26022232f, -0.29575172f, 1.500000f, -1.064030f},
	{0.10459357f, 0.08372527f, 1.110000f, -2.730563f},   {-0.68286800f, 0.04963045f, 1.090000f, -0.498827f},
	{-0.13570161f, -0.64190155f, 1.250000f, -0.532765f}, {-0.26193795f, -0.08205118f, 0.670000f, -1.783245f},
	{-0.61177456f, 0.66664219f, 0.710000f, -0.044234f},  {0.43675563f, 0.25119025f, 0.610000f, -1.167283f},
	{0.07884444f, 0.86618668f, 0.640000f, -0.459002f},   {-0.12790935f, -0.29869005f, 0.600000f, -1.729424f},
	{-0.04031125f, 0.02413622f, 0.600000f, -4.792042f},  {0.16201244f, -0.52851415f, 0.790000f, -1.067055f},
	{-0.70991218f, 0.47301072f, 0.640000f, -0.335236f},  {0.03277707f, -0.22349690f, 0.600000f, -1.982384f},
	{0.68921727f, 0.36800742f, 0.630000f, -0.266718f},   {0.29251814f, 0.37775412f, 0.610000f, -1.422520f},
	{-0.12224089f, 0.96582592f, 0.600000f, -0.426142f},  {0.11071457f, -0.16131058f, 0.600000f, -2.165947f},
	{0.46562141f, -0.59747696f, 0.600000f, -0.189760f},  {-0.51548797f, 0.11804193f, 0.600000f, -1.246800f},
	{0.89141309f, -0.42090443f, 0.600000f, 0.028192f},   {-0.32402530f, -0.01591529f, 0.600000f, -1.543018f},
	{0.60771245f, 0.41635221f, 0.600000f, -0.605411f},   {0.02379565f, -0.08239821f, 0.600000f, -3.809046f},
	{0.48951152f, -0.23657045f, 0.600000f, -1.189011f},  {-0.17611565f, -0.81696892f, 0.600000f, -0.513724f},
	{-0.33930185f, -0.20732205f, 0.600000f, -1.698047f}, {-0.91974425f, 0.05403209f, 0.600000f, 0.062246f},
	{-0.15064627f, -0.14949332f, 0.600000f, -1.896062f}, {0.53180975f, -0.35210401f, 0.600000f, -0.758838f},
	{0.41487166f, 0.81442589f, 0.600000f, -0.505648f},   {-0.24106961f, -0.32721516f, 0.600000f, -1.665244f},
};

// ---- the constant block, on the host -------------------------------------------------------------------------------------------
inline void reference_settings(gr_cacao_settings &s) // renderer/post/ssao.cpp:73-91
{
	s = {};
	s.radius = 0.6f;
	s.shadow_multiplier = 1.0f;
	s.shadow_power = 1.50f;
	s.shadow_clamp = 0.98f;
	s.horizon_angle_threshold = 0.06f;
	s.fade_out_from = 20.0f;
	s.fade_out_to = 40.0f;
	s.quality_level = GR_CACAO_QUALITY_HIGHEST;
	s.adaptive_quality_limit = 0.75f;
	s.blur_pass_count = 2;
	s.sharpness = 0.98f;
	s.detail_shadow_strength = 0.5f;
	s.generate_normals = 0;
	s.bilateral_sigma_squared = 5.0f;
	s.bilateral_similarity_distance_sigma = 0.1f;
}

inline void update_buffer_sizes(uint32_t width, uint32_t height, gr_cacao_buffer_sizes &b) // ffx_cacao.cpp:50-106, useDownsampledSsao = false
{
	const uint32_t half_w = (width + 1) / 2, half_h = (height + 1) / 2;
	b = {};
	b.inputOutputBufferWidth = width;
	b.inputOutputBufferHeight = height;
	b.depthBufferWidth = width;
	b.depthBufferHeight = height;
	b.ssaoBufferWidth = half_w;
	b.ssaoBufferHeight = half_h;
	b.deinterleavedDepthBufferWidth = half_w;
	b.deinterleavedDepthBufferHeight = half_h;
	b.importanceMapWidth = (half_w + 1) / 2;
	b.importanceMapHeight = (half_h + 1) / 2;
	b.downsampledSsaoBufferWidth = 1;
	b.downsampledSsaoBufferHeight = 1;
}

inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); } // FFX_CACAO_CLAMP

// proj and normals_to_view: 16 floats as a muglm mat4 lies in memory; elements[i][j] of FFX_CACAO_Matrix4x4 is m[4 * i + j].  The
// reference reads elements[3][2] and [2][2] "row major" from that column-major matrix, and flips Y (ffx_cacao.cpp:125-136).
inline void update_constants(gr_cacao_constants &c, const gr_cacao_settings &s, const gr_cacao_buffer_sizes &b, const float *proj, const float *normals_to_view)
{
	c.BilateralSigmaSquared = s.bilateral_sigma_squared;
	c.BilateralSimilarityDistanceSigma = s.bilateral_similarity_distance_sigma;
	memcpy(c.NormalsWorldToViewspaceMatrix, normals_to_view, 64);
	c.LoadCounterAvgDiv = 9.0f / float(double(b.importanceMapWidth * b.importanceMapHeight) * 255.0);
	const float mul = -proj[4 * 3 + 2];
	float add = proj[4 * 2 + 2];
	if (mul * add < 0)
		add = -add;
	c.DepthUnpackConsts[0] = mul;
	c.DepthUnpackConsts[1] = add;
	const float tan_half_fov_y = 1.0f / -proj[4 * 1 + 1], tan_half_fov_x = 1.0f / proj[0];
	c.CameraTanHalfFOV[0] = tan_half_fov_x;
	c.CameraTanHalfFOV[1] = tan_half_fov_y;
	c.NDCToViewMul[0] = c.CameraTanHalfFOV[0] * 2.0f;
	c.NDCToViewMul[1] = c.CameraTanHalfFOV[1] * -2.0f;
	c.NDCToViewAdd[0] = c.CameraTanHalfFOV[0] * -1.0f;
	c.NDCToViewAdd[1] = c.CameraTanHalfFOV[1] * 1.0f;
	const float ratio = float(b.inputOutputBufferWidth) / float(b.depthBufferWidth);
	const float border = (1.0f - ratio) / 2.0f;
	for (int i = 0; i < 2; i++)
	{
		c.DepthBufferUVToViewMul[i] = c.NDCToViewMul[i] / ratio;
		c.DepthBufferUVToViewAdd[i] = c.NDCToViewAdd[i] - c.NDCToViewMul[i] * border / ratio;
	}
	c.EffectRadius = clampf(s.radius, 0.0f, 100000.0f);
	c.EffectShadowStrength = clampf(s.shadow_multiplier * 4.3f, 0.0f, 10.0f);
	c.EffectShadowPow = clampf(s.shadow_power, 0.0f, 10.0f);
	c.EffectShadowClamp = clampf(s.shadow_clamp, 0.0f, 1.0f);
	c.EffectFadeOutMul = -1.0f / (s.fade_out_to - s.fade_out_from);
	c.EffectFadeOutAdd = s.fade_out_from / (s.fade_out_to - s.fade_out_from) + 1.0f;
	c.EffectHorizonAngleThreshold = clampf(s.horizon_angle_threshold, 0.0f, 1.0f);
	float near_limit = s.radius * 1.2f;
	c.DepthPrecisionOffsetMod = 0.9992f;
	near_limit /= tan_half_fov_y; // (the special cases of the two lowest quality levels are not reachable: they are refused)
	c.EffectSamplingRadiusNearLimitRec = 1.0f / near_limit;
	c.AdaptiveSampleCountLimit = s.adaptive_quality_limit;
	c.NegRecEffectRadius = -1.0f / c.EffectRadius;
	c.InvSharpness = clampf(1.0f - s.sharpness, 0.0f, 1.0f);
	c.DetailAOStrength = s.detail_shadow_strength;
	const auto dims = [](float *d, float *inv, uint32_t w, uint32_t h) {
		d[0] = float(w);
		d[1] = float(h);
		inv[0] = 1.0f / float(w);
		inv[1] = 1.0f / float(h);
	};
	dims(c.SSAOBufferDimensions, c.SSAOBufferInverseDimensions, b.ssaoBufferWidth, b.ssaoBufferHeight);
	dims(c.DepthBufferDimensions, c.DepthBufferInverseDimensions, b.depthBufferWidth, b.depthBufferHeight);
	c.DepthBufferOffset[0] = int32_t(b.depthBufferXOffset);
	c.DepthBufferOffset[1] = int32_t(b.depthBufferYOffset);
	dims(c.InputOutputBufferDimensions, c.InputOutputBufferInverseDimensions, b.inputOutputBufferWidth, b.inputOutputBufferHeight);
	dims(c.ImportanceMapDimensions, c.ImportanceMapInverseDimensions, b.importanceMapWidth, b.importanceMapHeight);
	dims(c.DeinterleavedDepthBufferDimensions, c.DeinterleavedDepthBufferInverseDimensions, b.deinterleavedDepthBufferWidth, b.deinterleavedDepthBufferHeight);
	c.DeinterleavedDepthBufferOffset[0] = float(b.deinterleavedDepthBufferXOffset);
	c.DeinterleavedDepthBufferOffset[1] = float(b.deinterleavedDepthBufferYOffset);
	c.DeinterleavedDepthBufferNormalisedOffset[0] = float(b.deinterleavedDepthBufferXOffset) / float(b.deinterleavedDepthBufferWidth);
	c.DeinterleavedDepthBufferNormalisedOffset[1] = float(b.deinterleavedDepthBufferYOffset) / float(b.deinterleavedDepthBufferHeight);
	c.NormalsUnpackMul = 2.0f;
	c.NormalsUnpackAdd = -1.0f;
}

inline void update_per_pass_constants(gr_cacao_constants &c, const gr_cacao_buffer_sizes &b, int pass) // ffx_cacao.cpp:236-269
{
	c.PerPassFullResUVOffset[0] = float(pass % 2) / float(b.ssaoBufferWidth);
	c.PerPassFullResUVOffset[1] = float(pass / 2) / float(b.ssaoBufferHeight);
	c.PassIndex = pass;
	const int sub_pass_count = 5;
	static const int spmap[5] = {0, 1, 4, 3, 2};
	for (int sub_pass = 0; sub_pass < sub_pass_count; sub_pass++)
	{
		const int a = pass, bb = spmap[sub_pass];
		const float angle0 = (float(a) + float(bb) / float(sub_pass_count)) * (3.1415926535897932384626433832795f) * 0.5f;
		const float ca = cosf(angle0), sa = sinf(angle0);
		const float scale = 1.0f + (float(a) - 1.5f + (float(bb) - (float(sub_pass_count) - 1.0f) * 0.5f) / float(sub_pass_count)) * 0.07f;
		c.PatternRotScaleMatrices[sub_pass][0] = scale * ca;
		c.PatternRotScaleMatrices[sub_pass][1] = scale * -sa;
		c.PatternRotScaleMatrices[sub_pass][2] = -scale * sa;
		c.PatternRotScaleMatrices[sub_pass][3] = -scale * ca;
	}
}

// ---- the workspace --------------------------------------------------------------------------------------------------------------
GR_HD uint32_t mip_extent(uint32_t size, uint32_t k)
{
	const uint32_t n = size >> k;
	return n ? n : 1u;
}

// Byte offsets from the workspace's start.  Layers and mips are tightly packed; every intermediate starts at a multiple of 256.
struct Workspace
{
	uint32_t width, height;   // input and output
	uint32_t half_w, half_h;  // SSAO and deinterleaved buffers
	uint32_t imp_w, imp_h;    // importance map
	uint64_t depth_mip[DEPTH_MIPS]; // R16F, 4 layers a mip
	uint64_t normals;         // RGBA8_SNORM, 4 layers
	uint64_t ssao[2];         // ping, pong: RG8, 4 layers
	uint64_t importance[2];   // map, pong: R8
	uint64_t load_counter;    // one uint32
	uint64_t bytes;
};

inline Workspace workspace_layout(uint32_t width, uint32_t height)
{
	Workspace w = {};
	w.width = width;
	w.height = height;
	w.half_w = (width + 1) / 2;
	w.half_h = (height + 1) / 2;
	w.imp_w = (w.half_w + 1) / 2;
	w.imp_h = (w.half_h + 1) / 2;
	uint64_t at = 0;
	const auto take = [&at](uint64_t bytes) {
		const uint64_t here = at;
		at = (at + bytes + WORKSPACE_ALIGN - 1) / WORKSPACE_ALIGN * WORKSPACE_ALIGN;
		return here;
	};
	uint64_t chain = 0, first = 0;
	for (uint32_t k = 0; k < DEPTH_MIPS; k++) // one intermediate: the mips follow one another without padding
	{
		w.depth_mip[k] = chain;
		chain += uint64_t(mip_extent(w.half_w, k)) * mip_extent(w.half_h, k) * 2u * PASSES;
	}
	first = take(chain);
	for (uint32_t k = 0; k < DEPTH_MIPS; k++)
		w.depth_mip[k] += first;
	const uint64_t half_texels = uint64_t(w.half_w) * w.half_h;
	w.normals = take(half_texels * 4u * PASSES);
	w.ssao[0] = take(half_texels * 2u * PASSES);
	w.ssao[1] = take(half_texels * 2u * PASSES);
	w.importance[0] = take(uint64_t(w.imp_w) * w.imp_h);
	w.importance[1] = take(uint64_t(w.imp_w) * w.imp_h);
	w.load_counter = take(4);
	w.bytes = at;
	return w;
}

// ---- small arithmetic -------------------------------------------------------------------------------------------------------------
GR_HD float saturate(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
// v / 255 for an integer v in [0, 255], bit for bit (checked again for all 256 inputs by tests/test_cacao_core_cpu.py)
GR_HD float unorm8(uint32_t v) { return gr_core::unorm8_to_float(v); }
// k / 3 for k in 0 .. 3, bit for bit, without the division
static_assert(2.0f * (1.0f / 3.0f) == 2.0f / 3.0f && 3.0f * (1.0f / 3.0f) == 1.0f, "k * (1 / 3) is k / 3 for the four edge levels");
GR_HD float third(uint32_t k) { return float(k) * (1.0f / 3.0f); }
GR_HD float snorm8(uint32_t v) { return fmaxf(float(int8_t(v)) / 127.0f, -1.0f); }
GR_HD uint32_t to_unorm8(float c) { return uint32_t(saturate(c) * 255.0f + 0.5f); }
GR_HD uint32_t to_snorm8(float c) { return uint32_t(int32_t(floorf(fminf(fmaxf(c, -1.0f), 1.0f) * 127.0f + 0.5f))) & 0xffu; }
GR_HD int mirrori(int i, int n)
{
	const int period = 2 * n;
	int m = i % period;
	if (m < 0)
		m += period;
	return m < n ? m : period - 1 - m;
}
GR_HD float dot4(float ax, float ay, float az, float aw, float bx, float by, float bz, float bw) { return ax * bx + ay * by + az * bz + aw * bw; }

// Linear filtering of one channel; fetch(x, y) takes texel indices already wrapped.
template <bool MIRROR, typename Fetch> GR_HD float sample_linear(Fetch fetch, int w, int h, float u, float v)
{
	int ix, iy;
	float a, b;
	linear_axis(u * float(w) - 0.5f, ix, a);
	linear_axis(v * float(h) - 0.5f, iy, b);
	const int x0 = MIRROR ? mirrori(ix, w) : clampi(ix, 0, w - 1), x1 = MIRROR ? mirrori(ix + 1, w) : clampi(ix + 1, 0, w - 1);
	const int y0 = MIRROR ? mirrori(iy, h) : clampi(iy, 0, h - 1), y1 = MIRROR ? mirrori(iy + 1, h) : clampi(iy + 1, 0, h - 1);
	float t = fetch(x0, y0);
	if (a != 0.0f)
		t = t * (1.0f - a) + fetch(x1, y0) * a;
	if (b != 0.0f)
	{
		float t1 = fetch(x0, y1);
		if (a != 0.0f)
			t1 = t1 * (1.0f - a) + fetch(x1, y1) * a;
		t = t * (1.0f - b) + t1 * b;
	}
	return t;
}

GR_HD float view_depth(const gr_cacao_constants &c, float screen_depth) { return c.DepthUnpackConsts[0] / (c.DepthUnpackConsts[1] - screen_depth); }

// FFX_CACAO_MipSmartAverage.  (-1 / EffectRadius * EffectRadius is what the shader says.)
GR_HD float mip_smart_average(const gr_cacao_constants &c, float d0, float d1, float d2, float d3)
{
	const float closest = fminf(fminf(d0, d1), fminf(d2, d3));
	const float falloff = -1.0f / c.EffectRadius * c.EffectRadius;
	const float t0 = d0 - closest, t1 = d1 - closest, t2 = d2 - closest, t3 = d3 - closest;
	const float w0 = saturate(t0 * t0 * falloff + 1.0f), w1 = saturate(t1 * t1 * falloff + 1.0f);
	const float w2 = saturate(t2 * t2 * falloff + 1.0f), w3 = saturate(t3 * t3 * falloff + 1.0f);
	return dot4(w0, w1, w2, w3, d0, d1, d2, d3) / dot4(w0, w1, w2, w3, 1.0f, 1.0f, 1.0f, 1.0f);
}

// FFX_CACAO_Prepare_LoadNormal of one A2B10G10R10 word (0 past the image), as the RGBA8_SNORM texel it is stored as
GR_HD uint32_t prepare_normal(const gr_cacao_constants &c, uint32_t word)
{
	const float nx = float(word & 1023u) / 1023.0f * c.NormalsUnpackMul + c.NormalsUnpackAdd;
	const float ny = float((word >> 10) & 1023u) / 1023.0f * c.NormalsUnpackMul + c.NormalsUnpackAdd;
	const float nz = float((word >> 20) & 1023u) / 1023.0f * c.NormalsUnpackMul + c.NormalsUnpackAdd;
	const float(*m)[4] = c.NormalsWorldToViewspaceMatrix; // column c of the matrix is m[c]
	const float vx = m[0][0] * nx + m[1][0] * ny + m[2][0] * nz;
	const float vy = m[0][1] * nx + m[1][1] * ny + m[2][1] * nz;
	const float vz = -(m[0][2] * nx + m[1][2] * ny + m[2][2] * nz);
	const float len = sqrtf(vx * vx + vy * vy + vz * vz);
	return to_snorm8(vx / len) | (to_snorm8(vy / len) << 8) | (to_snorm8(vz / len) << 16) | (to_snorm8(1.0f) << 24);
}

GR_HD float pack_edges(float l, float r, float t, float b)
{
	l = rintf(saturate(l) * 3.05f);
	r = rintf(saturate(r) * 3.05f);
	t = rintf(saturate(t) * 3.05f);
	b = rintf(saturate(b) * 3.05f);
	return dot4(l, r, t, b, 64.0f / 255.0f, 16.0f / 255.0f, 4.0f / 255.0f, 1.0f / 255.0f);
}
// FFX_CACAO_UnpackEdges / FFX_CACAO_UnpackEdgesFloat16_4 of the sampled edge channel: left, right, top, bottom
GR_HD void unpack_edges(const gr_cacao_constants &c, float packed_value, float e[4])
{
	const uint32_t packed = uint32_t(packed_value * 255.5f);
	e[0] = saturate(third((packed >> 6) & 3u) + c.InvSharpness);
	e[1] = saturate(third((packed >> 4) & 3u) + c.InvSharpness);
	e[2] = saturate(third((packed >> 2) & 3u) + c.InvSharpness);
	e[3] = saturate(third(packed & 3u) + c.InvSharpness);
}

// ---- SSAO generation --------------------------------------------------------------------------------------------------------------
// Everything a generate, importance or apply lane reads, as pointers.  Per-pass members are indexed by the pass.
struct Images
{
	const uint8_t *depth[PASSES][DEPTH_MIPS]; // R16F
	int mip_w[DEPTH_MIPS], mip_h[DEPTH_MIPS];
	const uint8_t *normals[PASSES];           // RGBA8_SNORM
	const uint8_t *ssao[2][PASSES];           // RG8
	const uint8_t *importance[2];             // R8
	const uint32_t *load_counter;
	int half_w, half_h, imp_w, imp_h;
};
inline Images images_of(const void *workspace, const Workspace &w)
{
	const uint8_t *base = static_cast<const uint8_t *>(workspace);
	Images im = {};
	for (uint32_t k = 0; k < DEPTH_MIPS; k++)
	{
		im.mip_w[k] = int(mip_extent(w.half_w, k));
		im.mip_h[k] = int(mip_extent(w.half_h, k));
		for (uint32_t p = 0; p < PASSES; p++)
			im.depth[p][k] = base + w.depth_mip[k] + uint64_t(p) * im.mip_w[k] * im.mip_h[k] * 2u;
	}
	const uint64_t half_texels = uint64_t(w.half_w) * w.half_h;
	for (uint32_t p = 0; p < PASSES; p++)
	{
		im.normals[p] = base + w.normals + p * half_texels * 4u;
		im.ssao[0][p] = base + w.ssao[0] + p * half_texels * 2u;
		im.ssao[1][p] = base + w.ssao[1] + p * half_texels * 2u;
	}
	im.importance[0] = base + w.importance[0];
	im.importance[1] = base + w.importance[1];
	im.load_counter = reinterpret_cast<const uint32_t *>(base + w.load_counter);
	im.half_w = int(w.half_w);
	im.half_h = int(w.half_h);
	im.imp_w = int(w.imp_w);
	im.imp_h = int(w.imp_h);
	return im;
}

struct PerPass
{
	float rot_scale[PASSES][5][4];
	float full_res_uv_offset[PASSES][2];
};
inline PerPass per_pass_of(const gr_cacao_constants constants[4])
{
	PerPass p;
	for (uint32_t i = 0; i < PASSES; i++)
	{
		memcpy(p.rot_scale[i], constants[i].PatternRotScaleMatrices, sizeof(p.rot_scale[i]));
		memcpy(p.full_res_uv_offset[i], constants[i].PerPassFullResUVOffset, sizeof(p.full_res_uv_offset[i]));
	}
	return p;
}

GR_HD float depth_texel(const Images &im, uint32_t pass, int mip, int x, int y)
{
	return half_to_float(reinterpret_cast<const uint16_t *>(im.depth[pass][mip])[size_t(y) * im.mip_w[mip] + x]);
}
// g_ViewspaceDepthTapSampler: nearest texel of the nearest mip, clamped
GR_HD int nearest_mip(float lod)
{
	const float t = ceilf(lod + 0.5f) - 1.0f;
	return t > 0.0f ? (t < 3.0f ? int(t) : 3) : 0;
}
GR_HD float depth_tap(const Images &im, uint32_t pass, float u, float v, float lod)
{
	const int mip = nearest_mip(lod);
	const int w = im.mip_w[mip], h = im.mip_h[mip];
	const int x = int(fminf(fmaxf(floorf(u * float(w)), 0.0f), float(w - 1))), y = int(fminf(fmaxf(floorf(v * float(h)), 0.0f), float(h - 1)));
	return depth_texel(im, pass, mip, x, y);
}
// g_DeinterleavedNormals[int3(coord, pass)]: zero outside the image
GR_HD void normal_texel(const Images &im, uint32_t pass, int x, int y, float n[3])
{
	uint32_t word = 0;
	const bool inside = uint32_t(x) < uint32_t(im.half_w) && uint32_t(y) < uint32_t(im.half_h);
	if (inside)
		word = reinterpret_cast<const uint32_t *>(im.normals[pass])[size_t(y) * im.half_w + x];
	n[0] = inside ? snorm8(word & 0xffu) : 0.0f;
	n[1] = inside ? snorm8((word >> 8) & 0xffu) : 0.0f;
	n[2] = inside ? snorm8((word >> 16) & 0xffu) : 0.0f;
}

GR_HD float pixel_obscurance(const gr_cacao_constants &c, const float n[3], float dx, float dy, float dz, float falloff_mul_sq)
{
	const float length_sq = dx * dx + dy * dy + dz * dz;
	const float n_dot_d = (n[0] * dx + n[1] * dy + n[2] * dz) / sqrtf(length_sq);
	const float falloff = fmaxf(0.0f, length_sq * falloff_mul_sq + 1.0f);
	return fmaxf(0.0f, n_dot_d - c.EffectHorizonAngleThreshold) * falloff;
}

struct TapState
{
	float obscurance_sum, weight_sum;
};
// One depth sample of a tap pair: FFX_CACAO_SSAOTapInner (weight_mod >= 0) and one turn of FFX_CACAO_SSAOAddHits, which overwrites the
// pattern's weight with the haloing term alone (weight_mod < 0 says so).
GR_HD void tap_sample(const gr_cacao_constants &c, const Images &im, uint32_t pass, TapState &s, float u, float v, float lod, const float centre[3],
                         const float n[3], float falloff_mul_sq, float weight_mod)
{
	const float z = depth_tap(im, pass, u, v, lod);
	const float hx = (c.DepthBufferUVToViewMul[0] * u + c.DepthBufferUVToViewAdd[0]) * z;
	const float hy = (c.DepthBufferUVToViewMul[1] * v + c.DepthBufferUVToViewAdd[1]) * z;
	const float dx = hx - centre[0], dy = hy - centre[1], dz = z - centre[2];
	const float obscurance = pixel_obscurance(c, n, dx, dy, dz, falloff_mul_sq);
	float reduct = fmaxf(0.0f, -dz);
	reduct = saturate(reduct * c.NegRecEffectRadius + 2.0f);
	float weight = HALOING_REDUCTION_AMOUNT * reduct + (1.0f - HALOING_REDUCTION_AMOUNT);
	if (weight_mod >= 0.0f)
		weight *= weight_mod;
	s.obscurance_sum += obscurance * weight;
	s.weight_sum += weight;
}

// FFX_CACAO_GenerateSSAOShadowsInternal for texel (X, Y) of `pass`.  QUALITY is the shader's level (2 or 3).  out: the two channels
// before the RG8 store.  lod_flag (host builds of the tests only, may be null): set when a tap's lod + 0.5 lies within 2^-10 of 1, 2
// or 3, where the last bit of log2 selects the mip.
template <int QUALITY, bool BASE>
GR_HD void generate_texel(const gr_cacao_constants &c, const PerPass &pp, const Images &im, uint32_t pass, int X, int Y, float out[2], bool *lod_flag = nullptr)
{
	const float svx = float(X), svy = float(Y);
	const float inv_w = c.DeinterleavedDepthBufferInverseDimensions[0], inv_h = c.DeinterleavedDepthBufferInverseDimensions[1];
	const float uvx = (svx + 0.5f) * inv_w + c.DeinterleavedDepthBufferNormalisedOffset[0];
	const float uvy = (svy + 0.5f) * inv_h + c.DeinterleavedDepthBufferNormalisedOffset[1];
	// the two gathers through g_PointMirrorSampler, offsets (-1, -1) and (0, 0): centre, left, top, right, bottom
	int ix, iy;
	float unused;
	linear_axis(uvx * float(im.half_w) - 0.5f, ix, unused);
	linear_axis(uvy * float(im.half_h) - 0.5f, iy, unused);
	const int xl = mirrori(ix - 1, im.half_w), xc = mirrori(ix, im.half_w), xr = mirrori(ix + 1, im.half_w);
	const int yt = mirrori(iy - 1, im.half_h), yc = mirrori(iy, im.half_h), yb = mirrori(iy + 1, im.half_h);
	const float pix_z = depth_texel(im, pass, 0, xc, yc);
	const float pix_lz = depth_texel(im, pass, 0, xl, yc), pix_tz = depth_texel(im, pass, 0, xc, yt);
	const float pix_rz = depth_texel(im, pass, 0, xr, yc), pix_bz = depth_texel(im, pass, 0, xc, yb);

	const float nsx = (svx + 0.5f) * c.SSAOBufferInverseDimensions[0], nsy = (svy + 0.5f) * c.SSAOBufferInverseDimensions[1];
	float centre[3] = {(c.NDCToViewMul[0] * nsx + c.NDCToViewAdd[0]) * pix_z, (c.NDCToViewMul[1] * nsy + c.NDCToViewAdd[1]) * pix_z, pix_z};
	float n[3];
	normal_texel(im, pass, X, Y, n);
	const float size_x = centre[2] * c.NDCToViewMul[0] * c.SSAOBufferInverseDimensions[0];
	const float size_y = centre[2] * c.NDCToViewMul[1] * c.SSAOBufferInverseDimensions[1];

	// FFX_CACAO_CalculateRadiusParameters
	const float centre_length = sqrtf(centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2]);
	const float too_close = saturate(centre_length * c.EffectSamplingRadiusNearLimitRec) * 0.8f + 0.2f;
	const float effect_radius = c.EffectRadius * too_close;
	const float lookup_radius_mod = (0.85f * effect_radius) / size_x;
	const float falloff_mul_sq = -1.0f / (effect_radius * effect_radius);

	const uint32_t pseudo_random = uint32_t(svy * 2.0f + svx) % 5u;
	const float *rs = pp.rot_scale[pass][pseudo_random];
	const float m00 = rs[0] * lookup_radius_mod, m01 = rs[1] * lookup_radius_mod, m10 = rs[2] * lookup_radius_mod, m11 = rs[3] * lookup_radius_mod;

	TapState s = {0.0f, 0.0f};
	float el = 1.0f, er = 1.0f, et = 1.0f, eb = 1.0f;
	centre[0] *= c.DepthPrecisionOffsetMod;
	centre[1] *= c.DepthPrecisionOffsetMod;
	centre[2] *= c.DepthPrecisionOffsetMod;

	if (!BASE)
	{
		// FFX_CACAO_CalculateEdges(pixZ, pixLZ, pixRZ, pixTZ, pixBZ)
		const float dl = pix_lz - pix_z, dr = pix_rz - pix_z, dt = pix_tz - pix_z, db = pix_bz - pix_z;
		const float al = dl + dr, ar = dr + dl, at = dt + db, ab = db + dt;
		const float denom = pix_z * 0.040f;
		el = saturate(1.3f - fminf(fabsf(dl), fabsf(al)) / denom);
		er = saturate(1.3f - fminf(fabsf(dr), fabsf(ar)) / denom);
		et = saturate(1.3f - fminf(fabsf(dt), fabsf(at)) / denom);
		eb = saturate(1.3f - fminf(fabsf(db), fabsf(ab)) / denom);

		// detail AO from the four neighbours
		const float vx = centre[0] / centre[2], vy = centre[1] / centre[2];
		const float zl = pix_lz - centre[2], zr = pix_rz - centre[2], zt = pix_tz - centre[2], zb = pix_bz - centre[2];
		const float modified = 4.0f * falloff_mul_sq;
		const float ol = pixel_obscurance(c, n, -size_x + vx * zl, 0.0f + vy * zl, 0.0f + 1.0f * zl, modified);
		const float orr = pixel_obscurance(c, n, size_x + vx * zr, 0.0f + vy * zr, 0.0f + 1.0f * zr, modified);
		const float ot = pixel_obscurance(c, n, 0.0f + vx * zt, -size_y + vy * zt, 0.0f + 1.0f * zt, modified);
		const float ob = pixel_obscurance(c, n, 0.0f + vx * zb, size_y + vy * zb, 0.0f + 1.0f * zb, modified);
		s.obscurance_sum += c.DetailAOStrength * dot4(ol, orr, ot, ob, el, er, et, eb);

		// edges from the normals of the four neighbours in this pass's layer
		float nl[3], nr[3], nt[3], nb[3];
		normal_texel(im, pass, X - 1, Y, nl);
		normal_texel(im, pass, X + 1, Y, nr);
		normal_texel(im, pass, X, Y - 1, nt);
		normal_texel(im, pass, X, Y + 1, nb);
		el *= saturate(n[0] * nl[0] + n[1] * nl[1] + n[2] * nl[2] + NORMAL_EDGES_DOT_THRESHOLD);
		er *= saturate(n[0] * nr[0] + n[1] * nr[1] + n[2] * nr[2] + NORMAL_EDGES_DOT_THRESHOLD);
		et *= saturate(n[0] * nt[0] + n[1] * nt[1] + n[2] * nt[2] + NORMAL_EDGES_DOT_THRESHOLD);
		eb *= saturate(n[0] * nb[0] + n[1] * nb[1] + n[2] * nb[2] + NORMAL_EDGES_DOT_THRESHOLD);
	}

	const float mip_offset = log2f(lookup_radius_mod) + DEPTH_MIPS_GLOBAL_OFFSET;
	const auto flag = [lod_flag](float lod) {
		if (lod_flag)
			for (int k = 1; k <= 3; k++)
				if (fabsf(lod + 0.5f - float(k)) <= 0x1p-10f)
					*lod_flag = true;
	};
	(void)flag;

	int first = 0, last = BASE ? ADAPTIVE_BASE_TAPS : Q2_TAPS;
	if (QUALITY == 3 && !BASE)
	{
		const float full_u = nsx + pp.full_res_uv_offset[pass][0], full_v = nsy + pp.full_res_uv_offset[pass][1];
		const uint8_t *map = im.importance[0];
		const int imp_w = im.imp_w;
		float importance = sample_linear<false>([map, imp_w](int x, int y) { return unorm8(map[size_t(y) * imp_w + x]); }, im.imp_w, im.imp_h, full_u, full_v);
		s.obscurance_sum *= (float(ADAPTIVE_BASE_TAPS) / float(MAX_TAPS)) + (importance * float(ADAPTIVE_FLEXIBLE_TAPS) / float(MAX_TAPS));
		const uint8_t *base_texel = im.ssao[1][pass] + (size_t(Y) * im.half_w + X) * 2u;
		s.weight_sum += unorm8(base_texel[1]) * float(ADAPTIVE_BASE_TAPS * 4.0);
		s.obscurance_sum += unorm8(base_texel[0]) * s.weight_sum;
		const float average_importance = float(*im.load_counter) * c.LoadCounterAvgDiv;
		importance *= saturate(c.AdaptiveSampleCountLimit / average_importance);
		const uint32_t additional = uint32_t(float(ADAPTIVE_FLEXIBLE_TAPS) * importance + 1.5f);
		first = ADAPTIVE_BASE_TAPS;
		last = int(additional + uint32_t(ADAPTIVE_BASE_TAPS) < uint32_t(MAX_TAPS) ? additional + uint32_t(ADAPTIVE_BASE_TAPS) : uint32_t(MAX_TAPS));
	}
	for (int i = first; i < last; i++)
	{
		const float *sample = SAMPLE_PATTERN[i];
		const float ox = rintf(m00 * sample[0] + m01 * sample[1]), oy = rintf(m10 * sample[0] + m11 * sample[1]);
		const float lod = sample[3] + mip_offset;
#if !defined(__HIP_DEVICE_COMPILE__)
		flag(lod);
#endif
		if (QUALITY == 3 && !BASE)
		{
			const float du = ox * inv_w, dv = oy * inv_h;
			tap_sample(c, im, pass, s, uvx + du, uvy + dv, lod, centre, n, falloff_mul_sq, -1.0f);
			tap_sample(c, im, pass, s, uvx - du, uvy - dv, lod, centre, n, falloff_mul_sq, -1.0f);
		}
		else
		{
			const float weight_mod = 1.0f * sample[2];
			tap_sample(c, im, pass, s, ox * inv_w + uvx, oy * inv_h + uvy, lod, centre, n, falloff_mul_sq, weight_mod);
			tap_sample(c, im, pass, s, -ox * inv_w + uvx, -oy * inv_h + uvy, lod, centre, n, falloff_mul_sq, weight_mod);
		}
	}

	float obscurance = s.obscurance_sum / s.weight_sum;
	if (BASE)
	{
		out[0] = obscurance;
		out[1] = s.weight_sum / (float(ADAPTIVE_BASE_TAPS) * 4.0f);
		return;
	}
	float fade_out = saturate(centre[2] * c.EffectFadeOutMul + c.EffectFadeOutAdd);
	const float edge_fade_out = saturate((1.0f - el - er) * 0.35f) + saturate((1.0f - et - eb) * 0.35f);
	fade_out *= saturate(1.0f - edge_fade_out);
	obscurance = c.EffectShadowStrength * obscurance;
	obscurance = fminf(obscurance, c.EffectShadowClamp);
	obscurance *= fade_out;
	const float occlusion = 1.0f - obscurance;
	out[0] = powf(saturate(occlusion), c.EffectShadowPow);
	out[1] = pack_edges(el, er, et, eb);
}

// ---- importance map -----------------------------------------------------------------------------------------------------------------
GR_HD float importance_texel(const gr_cacao_constants &c, const Images &im, int X, int Y)
{
	const float u = (float(2 * X) + 0.5f) * c.SSAOBufferInverseDimensions[0], v = (float(2 * Y) + 0.5f) * c.SSAOBufferInverseDimensions[1];
	int ix, iy;
	float unused;
	linear_axis(u * float(im.half_w) - 0.5f, ix, unused);
	linear_axis(v * float(im.half_h) - 0.5f, iy, unused);
	const int x0 = clampi(ix, 0, im.half_w - 1), x1 = clampi(ix + 1, 0, im.half_w - 1);
	const int y0 = clampi(iy, 0, im.half_h - 1), y1 = clampi(iy + 1, 0, im.half_h - 1);
	float min_v = 1.0f, max_v = 0.0f;
	for (uint32_t p = 0; p < PASSES; p++)
	{
		const uint8_t *layer = im.ssao[1][p];
		const int xs[4] = {x0, x1, x1, x0}, ys[4] = {y1, y1, y0, y0}; // gather order x, y, z, w
		float vals[4];
		for (int k = 0; k < 4; k++)
		{
			float t = unorm8(layer[(size_t(ys[k]) * im.half_w + xs[k]) * 2u]);
			t = c.EffectShadowStrength * t;
			t = 1.0f - t;
			vals[k] = powf(saturate(t), c.EffectShadowPow);
		}
		max_v = fmaxf(max_v, fmaxf(fmaxf(vals[0], vals[1]), fmaxf(vals[2], vals[3])));
		min_v = fminf(min_v, fminf(fminf(vals[0], vals[1]), fminf(vals[2], vals[3])));
	}
	return powf(saturate((max_v - min_v) * 2.0f), 0.8f);
}

// PostprocessImportanceMapA (B = false) and B: the four taps half a texel and one and a half texels off the centre
template <bool B> GR_HD float importance_postprocess_texel(const gr_cacao_constants &c, const Images &im, int X, int Y)
{
	const uint8_t *map = im.importance[B ? 1 : 0];
	const int w = im.imp_w, h = im.imp_h;
	const auto tap = [map, w, h](float u, float v) { return sample_linear<false>([map, w](int x, int y) { return unorm8(map[size_t(y) * w + x]); }, w, h, u, v); };
	const float u = (float(X) + 0.5f) * c.ImportanceMapInverseDimensions[0], v = (float(Y) + 0.5f) * c.ImportanceMapInverseDimensions[1];
	const float centre = tap(u, v);
	const float hx = 0.5f * c.ImportanceMapInverseDimensions[0], hy = 0.5f * c.ImportanceMapInverseDimensions[1];
	float vx, vy, vz, vw;
	if (!B)
	{
		vx = tap(u + -hx * 3.0f, v + -hy);
		vy = tap(u + hx, v + -hy * 3.0f);
		vz = tap(u + hx * 3.0f, v + hy);
		vw = tap(u + -hx, v + hy * 3.0f);
	}
	else
	{
		vx = tap(u + -hx, v + -hy * 3.0f);
		vy = tap(u + hx * 3.0f, v + -hy);
		vz = tap(u + hx, v + hy * 3.0f);
		vw = tap(u + -hx * 3.0f, v + hy);
	}
	const float avg = dot4(vx, vy, vz, vw, 0.25f, 0.25f, 0.25f, 0.25f);
	const float max_val = fmaxf(centre, fmaxf(fmaxf(vx, vz), fmaxf(vy, vw)));
	return max_val + 1.0f * (avg - max_val); // lerp(maxVal, avgVal, c_FFX_CACAO_SmoothenImportance = 1)
}

// ---- blur -----------------------------------------------------------------------------------------------------------------------------
// FFX_CACAO_CalcBlurredSampleF16_4 for one of its four lanes
GR_HD float blurred_sample(const float e[4], float centre, float left, float right, float top, float bottom)
{
	float sum = centre * 0.5f, weight = 0.5f;
	sum += left * e[0];
	weight += e[0];
	sum += right * e[1];
	weight += e[1];
	sum += top * e[2];
	weight += e[2];
	sum += bottom * e[3];
	weight += e[3];
	return sum / weight;
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------------
GR_HD uint32_t apply_texel(const gr_cacao_constants &c, const Images &im, uint32_t from_pong, int X, int Y)
{
	const int hx = X / 2, hy = Y / 2, mx = X % 2, my = Y % 2;
	const int ic = mx + my * 2, ih = (1 - mx) + my * 2, iv = mx + (1 - my) * 2, id = (1 - mx) + (1 - my) * 2;
	const uint8_t *const *layers = im.ssao[from_pong ? 1 : 0];
	const uint8_t *centre = layers[ic] + (size_t(hy) * im.half_w + hx) * 2u;
	float ao = unorm8(centre[0]);
	float e[4];
	unpack_edges(c, unorm8(centre[1]), e);
	const float fmx = float(mx), fmy = float(my), fmxe = e[1] - e[0], fmye = e[3] - e[2];
	const float inx = float(X), iny = float(Y);
	const float isx = c.SSAOBufferInverseDimensions[0], isy = c.SSAOBufferInverseDimensions[1];
	const int w = im.half_w, h = im.half_h;
	const auto tap = [layers, w, h](int layer, float u, float v) {
		const uint8_t *p = layers[layer];
		return sample_linear<false>([p, w](int x, int y) { return unorm8(p[(size_t(y) * w + x) * 2u]); }, w, h, u, v);
	};
	const float ao_h = tap(ih, (inx + (fmx + fmxe - 0.5f)) * 0.5f * isx, (iny + (0.5f - fmy)) * 0.5f * isy);
	const float ao_v = tap(iv, (inx + (0.5f - fmx)) * 0.5f * isx, (iny + (fmy - 0.5f + fmye)) * 0.5f * isy);
	const float ao_d = tap(id, (inx + (fmx - 0.5f + fmxe)) * 0.5f * isx, (iny + (fmy - 0.5f + fmye)) * 0.5f * isy);
	const float wy = (e[0] + e[1]) * 0.5f, wz = (e[2] + e[3]) * 0.5f, ww = (wy + wz) * 0.5f;
	const float weights_sum = dot4(1.0f, wy, wz, ww, 1.0f, 1.0f, 1.0f, 1.0f);
	ao = dot4(ao, ao_h, ao_v, ao_d, 1.0f, wy, wz, ww) / weights_sum;
	return to_unorm8(ao);
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__) || defined(CACAO_EMU)
constexpr uint32_t GROUP = 8u;       // every shader but the blur: numthreads(8, 8, 1)
constexpr uint32_t BLUR_GROUP = 16u; // FFX_CACAO_BLUR_WIDTH / HEIGHT
constexpr int BLUR_TILE_W = 4, BLUR_TILE_H = 3;
constexpr int BLUR_ARRAY_W = 2 * int(BLUR_GROUP) + 2, BLUR_ARRAY_H = BLUR_TILE_H * int(BLUR_GROUP) + 2;

struct PrepareDepthsLaunch
{
	gr_cacao_constants c;
	const uint8_t *depth; // D32F
	uint32_t depth_pitch;
	int width, height;
	uint8_t *workspace;
	Workspace ws;
};

// ClearLoadCounter + PrepareNativeDepthsAndMips.  One lane per half-resolution texel; the mips go through the LDS "smart average".
__global__ __launch_bounds__(GROUP *GROUP) void k_cacao_prepare_depths(PrepareDepthsLaunch a)
{
	__shared__ float s_depths[4][GROUP][GROUP];
	const uint32_t gx = threadIdx.x, gy = threadIdx.y;
	const uint32_t tx = blockIdx.x * GROUP + gx, ty = blockIdx.y * GROUP + gy;
	if (tx == 0 && ty == 0)
		*reinterpret_cast<uint32_t *>(a.workspace + a.ws.load_counter) = 0u;

	// GatherRed at the corner shared by texels (2 tx, 2 ty) .. (2 tx + 1, 2 ty + 1)
	const float u = (float(2u * tx) + 0.5f) * a.c.DepthBufferInverseDimensions[0], v = (float(2u * ty) + 0.5f) * a.c.DepthBufferInverseDimensions[1];
	int ix, iy;
	float unused;
	linear_axis(u * float(a.width) - 0.5f, ix, unused);
	linear_axis(v * float(a.height) - 0.5f, iy, unused);
	const int x0 = clampi(ix, 0, a.width - 1), x1 = clampi(ix + 1, 0, a.width - 1);
	const int y0 = clampi(iy, 0, a.height - 1), y1 = clampi(iy + 1, 0, a.height - 1);
	const float *row0 = reinterpret_cast<const float *>(a.depth + size_t(y0) * a.depth_pitch), *row1 = reinterpret_cast<const float *>(a.depth + size_t(y1) * a.depth_pitch);
	// layer 0 = samples.w (x0, y0), 1 = .z (x1, y0), 2 = .x (x0, y1), 3 = .y (x1, y1)
	const float d[4] = {view_depth(a.c, row0[x0]), view_depth(a.c, row0[x1]), view_depth(a.c, row1[x0]), view_depth(a.c, row1[x1])};
	for (uint32_t l = 0; l < 4; l++)
		s_depths[l][gx][gy] = d[l];
	const auto store = [&a](uint32_t mip, uint32_t layer, uint32_t x, uint32_t y, float value) {
		const uint32_t w = mip_extent(a.ws.half_w, mip), h = mip_extent(a.ws.half_h, mip);
		if (x < w && y < h)
			reinterpret_cast<uint16_t *>(a.workspace + a.ws.depth_mip[mip] + uint64_t(layer) * w * h * 2u)[size_t(y) * w + x] = uint16_t(float_to_half_pinned(value));
	};
	for (uint32_t l = 0; l < 4; l++)
		store(0, l, tx, ty, d[l]);

	const uint32_t layer = 2u * (gy % 2u) + (gx % 2u);
	const uint32_t ox = gx % 2u, oy = gy % 2u;
	const uint32_t bx = gx - ox, by = gy - oy;
	__syncthreads();
	{
		const float avg = mip_smart_average(a.c, s_depths[layer][bx][by], s_depths[layer][bx][by + 1], s_depths[layer][bx + 1][by], s_depths[layer][bx + 1][by + 1]);
		store(1, layer, tx / 2u, ty / 2u, avg);
		s_depths[layer][bx][by] = avg;
	}
	bool alive = gx % 4u == ox && gy % 4u == oy;
	__syncthreads();
	if (alive)
	{
		const float avg = mip_smart_average(a.c, s_depths[layer][bx][by], s_depths[layer][bx][by + 2], s_depths[layer][bx + 2][by], s_depths[layer][bx + 2][by + 2]);
		store(2, layer, tx / 4u, ty / 4u, avg);
		s_depths[layer][bx][by] = avg;
	}
	alive = gx % 8u == ox && gy % 8u == oy;
	__syncthreads();
	if (alive)
	{
		const float avg = mip_smart_average(a.c, s_depths[layer][bx][by], s_depths[layer][bx][by + 4], s_depths[layer][bx + 4][by], s_depths[layer][bx + 4][by + 4]);
		store(3, layer, tx / 8u, ty / 8u, avg);
	}
}

struct PrepareNormalsLaunch
{
	gr_cacao_constants c;
	const uint8_t *normal; // A2B10G10R10
	uint32_t normal_pitch;
	int width, height;
	uint8_t *workspace;
	Workspace ws;
};

__global__ __launch_bounds__(GROUP *GROUP) void k_cacao_prepare_normals(PrepareNormalsLaunch a)
{
	const uint32_t tx = blockIdx.x * GROUP + threadIdx.x, ty = blockIdx.y * GROUP + threadIdx.y;
	if (tx >= a.ws.half_w || ty >= a.ws.half_h)
		return;
	const uint64_t layer_bytes = uint64_t(a.ws.half_w) * a.ws.half_h * 4u;
	for (uint32_t l = 0; l < 4; l++)
	{
		const int x = int(2u * tx + (l & 1u)), y = int(2u * ty + (l >> 1));
		const uint32_t word = x < a.width && y < a.height ? reinterpret_cast<const uint32_t *>(a.normal + size_t(y) * a.normal_pitch)[x] : 0u;
		reinterpret_cast<uint32_t *>(a.workspace + a.ws.normals + l * layer_bytes)[size_t(ty) * a.ws.half_w + tx] = prepare_normal(a.c, word);
	}
}

struct GenerateLaunch
{
	gr_cacao_constants c;
	PerPass pp;
	Images im;
	uint8_t *out[PASSES]; // RG8 layer of each pass
};

// GenerateQ3Base / GenerateQ2 / GenerateQ3, the pass in blockIdx.z
template <int QUALITY, bool BASE> __global__ __launch_bounds__(GROUP *GROUP) void k_cacao_generate(GenerateLaunch a)
{
	const uint32_t x = blockIdx.x * GROUP + threadIdx.x, y = blockIdx.y * GROUP + threadIdx.y, pass = blockIdx.z;
	if (x >= uint32_t(a.im.half_w) || y >= uint32_t(a.im.half_h))
		return;
	float out[2];
	generate_texel<QUALITY, BASE>(a.c, a.pp, a.im, pass, int(x), int(y), out);
	reinterpret_cast<uint16_t *>(a.out[pass])[size_t(y) * a.im.half_w + x] = uint16_t(to_unorm8(out[0]) | (to_unorm8(out[1]) << 8));
}

struct ImportanceLaunch
{
	gr_cacao_constants c;
	Images im;
	uint8_t *out;           // R8
	uint32_t *load_counter; // PostprocessImportanceMapB only
};

__global__ __launch_bounds__(GROUP *GROUP) void k_cacao_importance_generate(ImportanceLaunch a)
{
	const uint32_t x = blockIdx.x * GROUP + threadIdx.x, y = blockIdx.y * GROUP + threadIdx.y;
	if (x >= uint32_t(a.im.imp_w) || y >= uint32_t(a.im.imp_h))
		return;
	a.out[size_t(y) * a.im.imp_w + x] = uint8_t(to_unorm8(importance_texel(a.c, a.im, int(x), int(y))));
}

// Groups of 8 x 8 texels; a workgroup walks the groups blockIdx.x, blockIdx.x + gridDim.x, ...  PostprocessImportanceMapA is launched with
// one workgroup a group.  PostprocessImportanceMapB with at most IMPORTANCE_MAX_GROUPS, each ending in one add to the counter word: the
// adds serialise on the word (measured at 4K: 8100 adds cost 90 us, 2048 workgroups walking four groups each 27 us).
constexpr uint32_t IMPORTANCE_MAX_GROUPS = 2048u;
template <bool B> __global__ __launch_bounds__(GROUP *GROUP) void k_cacao_importance_postprocess(ImportanceLaunch a)
{
	__shared__ uint32_t s_sum;
	const bool first = threadIdx.x == 0 && threadIdx.y == 0;
	if (B)
	{
		if (first)
			s_sum = 0u;
		__syncthreads();
	}
	const uint32_t groups_x = (uint32_t(a.im.imp_w) + GROUP - 1u) / GROUP, groups_y = (uint32_t(a.im.imp_h) + GROUP - 1u) / GROUP;
	for (uint32_t group = blockIdx.x; group < groups_x * groups_y; group += gridDim.x)
	{
		const uint32_t x = (group % groups_x) * GROUP + threadIdx.x, y = (group / groups_x) * GROUP + threadIdx.y;
		if (x >= uint32_t(a.im.imp_w) || y >= uint32_t(a.im.imp_h))
			continue;
		const float value = importance_postprocess_texel<B>(a.c, a.im, int(x), int(y));
		a.out[size_t(y) * a.im.imp_w + x] = uint8_t(to_unorm8(value));
		// every ninth texel; integer adds, so the total does not depend on their order
		if (B && (x % 3u) + (y % 3u) == 0u)
			atomicAdd(&s_sum, uint32_t(saturate(value) * 255.0f + 0.5f));
	}
	if (B)
	{
		__syncthreads();
		if (first && s_sum)
			atomicAdd(a.load_counter, s_sum);
	}
}

struct BlurLaunch
{
	gr_cacao_constants c;
	const uint8_t *in[PASSES]; // RG8
	uint8_t *out[PASSES];
	int half_w, half_h;
	uint32_t blur_passes;
};

// EdgeSensitiveBlurN: 16 x 16 lanes of 4 x 3 texels; occlusion as fp16 pairs in two LDS arrays, the tile shrinks by 2 N.  The pass is
// in blockIdx.z.  Rows of the arrays run along x (the shader's run along y): the values are the same, the banks are not.
__global__ __launch_bounds__(BLUR_GROUP *BLUR_GROUP) void k_cacao_blur(BlurLaunch a)
{
	__shared__ uint32_t s_front[BLUR_ARRAY_H][BLUR_ARRAY_W + 1], s_back[BLUR_ARRAY_H][BLUR_ARRAY_W + 1];
	const int n = int(a.blur_passes);
	const int tid_x = int(threadIdx.x), tid_y = int(threadIdx.y);
	const uint32_t pass = blockIdx.z;
	const int image_x = int(blockIdx.x) * (BLUR_TILE_W * int(BLUR_GROUP) - 2 * n) + BLUR_TILE_W * tid_x - n;
	const int image_y = int(blockIdx.y) * (BLUR_TILE_H * int(BLUR_GROUP) - 2 * n) + BLUR_TILE_H * tid_y - n;
	const int buffer_x = 2 * tid_x + 1, buffer_y = BLUR_TILE_H * tid_y + 1;
	const uint8_t *in = a.in[pass];
	const int w = a.half_w, h = a.half_h;

	// the apron no lane stores: read by the outermost lanes, whose results the shrinking tile discards
	if (tid_x == 0)
		GR_UNROLL
		for (int y = 0; y < BLUR_TILE_H; y++)
			s_front[buffer_y + y][0] = s_back[buffer_y + y][0] = s_front[buffer_y + y][BLUR_ARRAY_W - 1] = s_back[buffer_y + y][BLUR_ARRAY_W - 1] = 0u;
	if (tid_y == 0)
		GR_UNROLL
		for (int x = 0; x < 2; x++)
			s_front[0][buffer_x + x] = s_back[0][buffer_x + x] = s_front[BLUR_ARRAY_H - 1][buffer_x + x] = s_back[BLUR_ARRAY_H - 1][buffer_x + x] = 0u;

	float edges[BLUR_TILE_H][BLUR_TILE_W][4];
	uint32_t edge_bytes[BLUR_TILE_H][BLUR_TILE_W];
	GR_UNROLL
	for (int y = 0; y < BLUR_TILE_H; y++)
	{
		float ssao[BLUR_TILE_W];
		GR_UNROLL
		for (int x = 0; x < BLUR_TILE_W; x++)
		{
			// g_PointMirrorSampler at a texel centre: linear, mirrored
			const float u = (float(image_x + x) + 0.5f) * a.c.SSAOBufferInverseDimensions[0], v = (float(image_y + y) + 0.5f) * a.c.SSAOBufferInverseDimensions[1];
			ssao[x] = sample_linear<true>([in, w](int tx, int ty) { return unorm8(in[(size_t(ty) * w + tx) * 2u]); }, w, h, u, v);
			const float packed = sample_linear<true>([in, w](int tx, int ty) { return unorm8(in[(size_t(ty) * w + tx) * 2u + 1u]); }, w, h, u, v);
			unpack_edges(a.c, packed, edges[y][x]);
			edge_bytes[y][x] = to_unorm8(packed);
		}
		s_front[buffer_y + y][buffer_x] = float_to_half_pinned(ssao[0]) | (float_to_half_pinned(ssao[1]) << 16);
		s_front[buffer_y + y][buffer_x + 1] = float_to_half_pinned(ssao[2]) | (float_to_half_pinned(ssao[3]) << 16);
	}
	__syncthreads();

	for (int i = 0; i < n; i++)
	{
		uint32_t(*src)[BLUR_ARRAY_W + 1] = (i & 1) ? s_back : s_front;
		uint32_t(*dst)[BLUR_ARRAY_W + 1] = (i & 1) ? s_front : s_back;
		GR_UNROLL
		for (int y = 0; y < BLUR_TILE_H; y++)
		{
			const int cx = buffer_x, cy = buffer_y + y;
			const uint32_t c0 = src[cy][cx], c1 = src[cy][cx + 1], t0 = src[cy - 1][cx], t1 = src[cy - 1][cx + 1], b0 = src[cy + 1][cx], b1 = src[cy + 1][cx + 1];
			const float centre[4] = {half_to_float(c0 & 0xffffu), half_to_float(c0 >> 16), half_to_float(c1 & 0xffffu), half_to_float(c1 >> 16)};
			const float top[4] = {half_to_float(t0 & 0xffffu), half_to_float(t0 >> 16), half_to_float(t1 & 0xffffu), half_to_float(t1 >> 16)};
			const float bottom[4] = {half_to_float(b0 & 0xffffu), half_to_float(b0 >> 16), half_to_float(b1 & 0xffffu), half_to_float(b1 >> 16)};
			const float left[4] = {half_to_float(src[cy][cx - 1] >> 16), centre[0], centre[1], centre[2]};
			const float right[4] = {centre[1], centre[2], centre[3], half_to_float(src[cy][cx + 2] & 0xffffu)};
			float r[4];
			GR_UNROLL
			for (int k = 0; k < 4; k++)
				r[k] = blurred_sample(edges[y][k], centre[k], left[k], right[k], top[k], bottom[k]);
			dst[cy][cx] = float_to_half_pinned(r[0]) | (float_to_half_pinned(r[1]) << 16);
			dst[cy][cx + 1] = float_to_half_pinned(r[2]) | (float_to_half_pinned(r[3]) << 16);
		}
		__syncthreads();
	}

	uint32_t(*result)[BLUR_ARRAY_W + 1] = (n & 1) ? s_back : s_front;
	uint8_t *out = a.out[pass];
	GR_UNROLL
	for (int y = 0; y < BLUR_TILE_H; y++)
	{
		const int output_y = BLUR_TILE_H * tid_y + y;
		if (output_y < n || output_y >= BLUR_TILE_H * int(BLUR_GROUP) - n)
			continue;
		const uint32_t r0 = result[buffer_y + y][buffer_x], r1 = result[buffer_y + y][buffer_x + 1];
		const float value[4] = {half_to_float(r0 & 0xffffu), half_to_float(r0 >> 16), half_to_float(r1 & 0xffffu), half_to_float(r1 >> 16)};
		GR_UNROLL
		for (int x = 0; x < BLUR_TILE_W; x++)
		{
			const int output_x = BLUR_TILE_W * tid_x + x, px = image_x + x, py = image_y + y;
			if (output_x < n || output_x >= BLUR_TILE_W * int(BLUR_GROUP) - n || px < 0 || py < 0 || px >= w || py >= h)
				continue;
			reinterpret_cast<uint16_t *>(out)[size_t(py) * w + px] = uint16_t(to_unorm8(value[x]) | (edge_bytes[y][x] << 8));
		}
	}
}

struct ApplyLaunch
{
	gr_cacao_constants c;
	Images im;
	uint8_t *out; // R8
	uint32_t out_pitch;
	int width, height;
	uint32_t from_pong;
};

__global__ __launch_bounds__(GROUP *GROUP) void k_cacao_apply(ApplyLaunch a)
{
	const uint32_t x = blockIdx.x * GROUP + threadIdx.x, y = blockIdx.y * GROUP + threadIdx.y;
	if (x >= uint32_t(a.width) || y >= uint32_t(a.height))
		return;
	a.out[size_t(y) * a.out_pitch + x] = uint8_t(apply_texel(a.c, a.im, a.from_pong, int(x), int(y)));
}
#endif
} // namespace gr_cacao
