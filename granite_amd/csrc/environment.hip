// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Environment baking: what renderer/utils/image_utils.cpp's convert_equirect_to_cube, convert_cube_to_ibl_specular and
// convert_cube_to_ibl_diffuse draw with skybox.vert + {skybox_latlon, util/ibl_specular, util/ibl_diffuse}.frag, one render pass per
// face and level there, one launch per entry point here (plus one per mip level of the equirect cube, each reading the one above).
// The arithmetic is env_core.hpp's; this file adds the mapping of texels and taps to lanes.
//
//   k_env_latlon    one lane per level-0 texel: direction, atan / asin, one LinearWrap tap.
//   k_env_blit      one lane per texel of a mip level: the linear blit of generate_mipmap, per face.
//   k_env_specular  all faces and levels in one launch.  A workgroup of four waves belongs to one level: it first computes that
//                   level's 1024 (L, NdotL) entries -- they depend on (i, roughness) alone, V = N -- into 16 KiB of LDS.  Levels of
//                   at least SPECULAR_WAVE_BELOW texels then run one texel per lane, every lane walking the table (the NdotL > 0
//                   test is the same for the whole wave there); smaller levels give a texel to a wave, lane k taking samples
//                   k, k + 64, ..., and reduce across the wave, so the 1 x 1 x 6 tail is 6 waves of 16 samples each.
//   k_env_diffuse   a wave per texel, lane k taking taps k, k + 64, ... of the 252 x 63 grid; sin / cos of the 315 angles in LDS.
#include "ctx.hpp"
#include "env_core.hpp"

namespace
{
using namespace gr_env;

constexpr uint32_t GROUP = 256u, WAVES = GROUP / 64u;
// A level with fewer texels than this gives each texel a wave: 16384 lanes do not fill 256 CUs x 4 SIMDs with one wave each.
constexpr uint32_t SPECULAR_WAVE_BELOW = 16384u;

struct FaceMatrices
{
	float inv[6][16]; // inverse(proj * look) per face, column major
};

struct LatlonArgs
{
	Equirect equirect;
	uint2 *out;
	uint32_t size;
	FaceMatrices faces;
};

struct BlitArgs
{
	const uint2 *src;
	uint2 *dst;
	uint32_t src_size, dst_size;
};

struct SpecularArgs
{
	Cube src;
	uint8_t *out;
	uint32_t out_size, out_levels;
	float base_lod;
	uint32_t first_group[MAX_LEVELS + 1]; // level l owns workgroups [first_group[l], first_group[l + 1])
	FaceMatrices faces;
};

struct DiffuseArgs
{
	Cube src;
	uint2 *out;
	uint32_t out_size, level;
	FaceMatrices faces;
};

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
	for (int offset = 32; offset > 0; offset >>= 1)
		v += __shfl_xor(v, offset, 64);
	return v;
}

__global__ __launch_bounds__(GROUP) void k_env_latlon(LatlonArgs a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x, face_texels = a.size * a.size;
	if (index >= 6u * face_texels)
		return;
	const uint32_t face = index / face_texels, at = index - face * face_texels;
	const int y = int(at / a.size), x = int(at - uint32_t(y) * a.size);
	const f3 rgb = latlon(a.equirect, texel_direction(a.faces.inv[face], int(a.size), x, y));
	a.out[index] = pack_rgba(rgb, 1.0f);
}

__global__ __launch_bounds__(GROUP) void k_env_blit(BlitArgs a)
{
	const uint32_t index = blockIdx.x * GROUP + threadIdx.x, face_texels = a.dst_size * a.dst_size;
	if (index >= 6u * face_texels)
		return;
	const uint32_t face = index / face_texels, at = index - face * face_texels;
	const int y = int(at / a.dst_size), x = int(at - uint32_t(y) * a.dst_size);
	f3 rgb;
	float alpha;
	blit_texel(a.src + size_t(face) * a.src_size * a.src_size, int(a.src_size), int(a.dst_size), x, y, rgb, alpha);
	a.dst[index] = pack_rgba(rgb, alpha);
}

__global__ __launch_bounds__(GROUP) void k_env_specular(SpecularArgs a)
{
	__shared__ SpecularSample table[SPECULAR_SAMPLES];
	uint32_t level = 0;
	while (level + 1u < a.out_levels && blockIdx.x >= a.first_group[level + 1u])
		level++;
	const float roughness = specular_roughness(level, a.out_levels);
	for (uint32_t i = threadIdx.x; i < SPECULAR_SAMPLES; i += GROUP)
		table[i] = specular_sample(i, roughness);
	__syncthreads();

	const uint32_t n = level_size(a.out_size, level), face_texels = n * n, texels = 6u * face_texels;
	const LodPair lods = trilinear_levels(a.base_lod + float(level), a.src.levels);
	const CubeLevel l0 = cube_level(a.src, lods.level0), l1 = cube_level(a.src, lods.level1);
	const uint32_t group = blockIdx.x - a.first_group[level];
	const bool per_wave = texels < SPECULAR_WAVE_BELOW;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t index = per_wave ? group * WAVES + threadIdx.x / 64u : group * GROUP + threadIdx.x;
	if (index >= texels)
		return;
	const uint32_t face = index / face_texels, at = index - face * face_texels;
	const int y = int(at / n), x = int(at - uint32_t(y) * n);
	const Frame frame = specular_frame(texel_direction(a.faces.inv[face], int(n), x, y));
	f3 sum = {0.0f, 0.0f, 0.0f};
	float weight = 0.0f;
	uint2 *out = reinterpret_cast<uint2 *>(a.out + chain_offset(a.out_size, level, 0));
	if (per_wave)
	{
		specular_accumulate(l0, l1, lods.weight, frame, table, lane, 64u, sum, weight);
		sum = {wave_sum(sum.x), wave_sum(sum.y), wave_sum(sum.z)};
		weight = wave_sum(weight);
		if (lane != 0u)
			return;
	}
	else
		specular_accumulate(l0, l1, lods.weight, frame, table, 0u, 1u, sum, weight);
	out[index] = pack_rgba({sum.x / weight, sum.y / weight, sum.z / weight}, 1.0f);
}

__global__ __launch_bounds__(GROUP) void k_env_diffuse(DiffuseArgs a)
{
	__shared__ SinCos phi[DIFFUSE_PHI_STEPS], theta[DIFFUSE_THETA_STEPS];
	for (uint32_t k = threadIdx.x; k < DIFFUSE_PHI_STEPS + DIFFUSE_THETA_STEPS; k += GROUP)
	{
		const bool is_phi = k < DIFFUSE_PHI_STEPS;
		const float angle = diffuse_angle(is_phi ? k : k - DIFFUSE_PHI_STEPS);
		const SinCos sc = {sinf(angle), cosf(angle)};
		if (is_phi)
			phi[k] = sc;
		else
			theta[k - DIFFUSE_PHI_STEPS] = sc;
	}
	__syncthreads();

	const uint32_t n = a.out_size, face_texels = n * n;
	const uint32_t index = blockIdx.x * WAVES + threadIdx.x / 64u, lane = threadIdx.x & 63u;
	if (index >= 6u * face_texels)
		return;
	const uint32_t face = index / face_texels, at = index - face * face_texels;
	const int y = int(at / n), x = int(at - uint32_t(y) * n);
	const Frame frame = diffuse_frame(texel_direction(a.faces.inv[face], int(n), x, y));
	const CubeLevel l = cube_level(a.src, a.level);
	f3 sum = {0.0f, 0.0f, 0.0f};
	diffuse_accumulate(l, frame, phi, theta, lane, 64u, sum);
	sum = {wave_sum(sum.x), wave_sum(sum.y), wave_sum(sum.z)};
	if (lane == 0u)
		a.out[index] = pack_rgba(diffuse_resolve(sum), 1.0f);
}

void face_matrices(FaceMatrices &m) { face_inverse_matrices(m.inv); }

constexpr uint32_t MAX_CUBE_SIZE = 16384u; // 6 n^2 texel indices stay below 2^32

// What every entry point asks of a cube it reads or writes.
int check_chain(gr_ctx *ctx, const char *who, const char *what, const void *ptr, uint32_t size, uint32_t levels)
{
	if (!ptr)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: invalid argument: %s is a null pointer", who, what);
	if (size == 0 || size > MAX_CUBE_SIZE)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: %s size %u is outside 1 .. %u", who, what, size, MAX_CUBE_SIZE);
	if (levels == 0 || levels > full_chain_levels(size))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: %s levels %u are beyond the chain of size %u (1 .. %u)", who, what, levels, size, full_chain_levels(size));
	if (reinterpret_cast<uintptr_t>(ptr) & 15u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "%s: %s is not 16-byte aligned", who, what);
	return GR_OK;
}
} // namespace

extern "C" uint64_t gr_cube_chain_offset(uint32_t size, uint32_t level, uint32_t face)
{
	return gr_env::chain_offset(size, level, face);
}

extern "C" uint64_t gr_cube_chain_bytes(uint32_t size, uint32_t levels)
{
	return gr_env::chain_offset(size, levels, 0);
}

extern "C" int gr_env_equirect_to_cube(gr_ctx *ctx, gr_stream stream, const gr_image *equirect, void *cube, uint32_t size, uint32_t levels)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, equirect);
	if (equirect->format != GR_FORMAT_R16G16B16A16_SFLOAT)
		return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_env_equirect_to_cube: equirect format %u is not R16G16B16A16_SFLOAT", equirect->format);
	if (int code = check_chain(ctx, "gr_env_equirect_to_cube", "cube", cube, size, levels))
		return code;
	GR_CHECK_IMAGE(ctx, equirect, GR_FORMAT_R16G16B16A16_SFLOAT);
	if (equirect->width > 65536u || equirect->height > 65536u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_env_equirect_to_cube: equirect extent %u x %u is outside 1 .. 65536", equirect->width, equirect->height);

	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "env_equirect_to_cube"};
	LatlonArgs a = {};
	a.equirect = {static_cast<const uint8_t *>(equirect->ptr), int(equirect->width), int(equirect->height), equirect->pitch_bytes};
	a.out = static_cast<uint2 *>(cube);
	a.size = size;
	face_matrices(a.faces);
	hipLaunchKernelGGL(k_env_latlon, dim3(gr_div_up(6u * size * size, GROUP)), dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	for (uint32_t level = 1; level < levels; level++)
	{
		BlitArgs b = {};
		b.src = reinterpret_cast<const uint2 *>(static_cast<const uint8_t *>(cube) + chain_offset(size, level - 1u, 0));
		b.dst = reinterpret_cast<uint2 *>(static_cast<uint8_t *>(cube) + chain_offset(size, level, 0));
		b.src_size = level_size(size, level - 1u);
		b.dst_size = level_size(size, level);
		hipLaunchKernelGGL(k_env_blit, dim3(gr_div_up(6u * b.dst_size * b.dst_size, GROUP)), dim3(GROUP), 0, s, b);
		GR_CHECK_LAUNCH(ctx);
	}
	return GR_OK;
}

extern "C" int gr_env_specular(gr_ctx *ctx, gr_stream stream, const gr_cube *src, void *out, uint32_t out_size, uint32_t out_levels)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, src);
	if (int code = check_chain(ctx, "gr_env_specular", "src", src->ptr, src->size, src->levels))
		return code;
	if (int code = check_chain(ctx, "gr_env_specular", "out", out, out_size, out_levels))
		return code;

	SpecularArgs a = {};
	a.src = {static_cast<const uint8_t *>(src->ptr), src->size, src->levels};
	a.out = static_cast<uint8_t *>(out);
	a.out_size = out_size;
	a.out_levels = out_levels;
	a.base_lod = log2f(float(src->size)) - log2f(float(out_size));
	for (uint32_t level = 0; level < out_levels; level++)
	{
		const uint32_t n = level_size(out_size, level), texels = 6u * n * n;
		a.first_group[level + 1u] = a.first_group[level] + gr_div_up(texels, texels < SPECULAR_WAVE_BELOW ? WAVES : GROUP);
	}
	face_matrices(a.faces);
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "env_specular"};
	hipLaunchKernelGGL(k_env_specular, dim3(a.first_group[out_levels]), dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

extern "C" int gr_env_diffuse(gr_ctx *ctx, gr_stream stream, const gr_cube *src, void *out, uint32_t out_size)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, src);
	if (int code = check_chain(ctx, "gr_env_diffuse", "src", src->ptr, src->size, src->levels))
		return code;
	if (int code = check_chain(ctx, "gr_env_diffuse", "out", out, out_size, 1))
		return code;
	// the shader's two float loops, run here as written: the kernel's tables are sized by what they come to
	const uint32_t phi_steps = diffuse_steps(2.0f * SHADER_PI), theta_steps = diffuse_steps(0.5f * SHADER_PI);
	if (phi_steps != DIFFUSE_PHI_STEPS || theta_steps != DIFFUSE_THETA_STEPS || phi_steps * theta_steps != 15876u)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_env_diffuse: the hemisphere loops run %u x %u times here, not 252 x 63", phi_steps, theta_steps);

	DiffuseArgs a = {};
	a.src = {static_cast<const uint8_t *>(src->ptr), src->size, src->levels};
	a.out = static_cast<uint2 *>(out);
	a.out_size = out_size;
	const float lod = log2f(float(out_size)) - 5.0f;
	a.level = nearest_level(lod > 0.0f ? lod : 0.0f, src->levels);
	face_matrices(a.faces);
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "env_diffuse"};
	hipLaunchKernelGGL(k_env_diffuse, dim3(gr_div_up(6u * out_size * out_size, WAVES)), dim3(GROUP), 0, s, a);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}
