// TEST INFRASTRUCTURE.  granite_amd/csrc/env_core.hpp -- the per-texel arithmetic the kernels of environment.hip call -- built for the
// host as a shared library.  Every texel is computed as the kernels compute it, including the split of a texel's taps over `lanes`
// lanes (1: one texel per lane; 64: a wave per texel, partial sums added in the order of the wave's butterfly reduction).
// tests/test_env_core_cpu.py holds it to the golden of the executed shaders (tests/golden/env_bake_shader_v1.npz) before a device
// sees the code.
#include <vector>
#include "../../granite_amd/csrc/env_core.hpp"
#include "../../granite_amd/csrc/host/math.cpp"

using namespace gr_env;

namespace
{
// what wave_sum of environment.hip leaves in lane 0: log2(lanes) rounds of v[i] += v[i ^ offset]
float butterfly(std::vector<float> v)
{
	for (size_t offset = v.size() / 2; offset > 0; offset /= 2)
	{
		std::vector<float> next(v.size());
		for (size_t i = 0; i < v.size(); i++)
			next[i] = v[i] + v[i ^ offset];
		v = next;
	}
	return v[0];
}
f3 butterfly3(const std::vector<f3> &v)
{
	std::vector<float> x, y, z;
	for (const f3 &e : v)
	{
		x.push_back(e.x);
		y.push_back(e.y);
		z.push_back(e.z);
	}
	return {butterfly(x), butterfly(y), butterfly(z)};
}
} // namespace

extern "C" void env_host_matrices(float *out) { face_inverse_matrices(reinterpret_cast<float(*)[16]>(out)); }

extern "C" uint64_t env_host_chain_offset(uint32_t size, uint32_t level, uint32_t face) { return chain_offset(size, level, face); }

extern "C" void env_host_equirect_to_cube(const float *matrices, const uint8_t *equirect, int w, int h, uint8_t *cube, uint32_t size, uint32_t levels)
{
	const Equirect e = {equirect, w, h, uint32_t(w) * 8u};
	uint2 *out = reinterpret_cast<uint2 *>(cube);
	for (uint32_t face = 0; face < 6; face++)
		for (uint32_t y = 0; y < size; y++)
			for (uint32_t x = 0; x < size; x++)
				out[(face * size + y) * size + x] = pack_rgba(latlon(e, texel_direction(matrices + 16 * face, int(size), int(x), int(y))), 1.0f);
	for (uint32_t level = 1; level < levels; level++)
	{
		const uint32_t m = level_size(size, level - 1), n = level_size(size, level);
		const uint2 *src = reinterpret_cast<const uint2 *>(cube + chain_offset(size, level - 1, 0));
		uint2 *dst = reinterpret_cast<uint2 *>(cube + chain_offset(size, level, 0));
		for (uint32_t face = 0; face < 6; face++)
			for (uint32_t y = 0; y < n; y++)
				for (uint32_t x = 0; x < n; x++)
				{
					f3 rgb;
					float alpha;
					blit_texel(src + size_t(face) * m * m, int(m), int(n), int(x), int(y), rgb, alpha);
					dst[(face * n + y) * n + x] = pack_rgba(rgb, alpha);
				}
	}
}

extern "C" void env_host_specular(const float *matrices, const uint8_t *src, uint32_t src_size, uint32_t src_levels, uint8_t *out, uint32_t out_size,
                                  uint32_t out_levels, uint32_t lanes)
{
	const Cube cube = {src, src_size, src_levels};
	const float base_lod = log2f(float(src_size)) - log2f(float(out_size));
	std::vector<SpecularSample> table(SPECULAR_SAMPLES);
	for (uint32_t level = 0; level < out_levels; level++)
	{
		for (uint32_t i = 0; i < SPECULAR_SAMPLES; i++)
			table[i] = specular_sample(i, specular_roughness(level, out_levels));
		const LodPair lods = trilinear_levels(base_lod + float(level), src_levels);
		const CubeLevel l0 = cube_level(cube, lods.level0), l1 = cube_level(cube, lods.level1);
		const uint32_t n = level_size(out_size, level);
		uint2 *dst = reinterpret_cast<uint2 *>(out + chain_offset(out_size, level, 0));
		for (uint32_t face = 0; face < 6; face++)
			for (uint32_t y = 0; y < n; y++)
				for (uint32_t x = 0; x < n; x++)
				{
					const Frame frame = specular_frame(texel_direction(matrices + 16 * face, int(n), int(x), int(y)));
					std::vector<f3> sums(lanes, f3{0.0f, 0.0f, 0.0f});
					std::vector<float> weights(lanes, 0.0f);
					for (uint32_t lane = 0; lane < lanes; lane++)
						specular_accumulate(l0, l1, lods.weight, frame, table.data(), lane, lanes, sums[lane], weights[lane]);
					const f3 sum = butterfly3(sums);
					const float weight = butterfly(weights);
					dst[(face * n + y) * n + x] = pack_rgba({sum.x / weight, sum.y / weight, sum.z / weight}, 1.0f);
				}
	}
}

extern "C" int env_host_diffuse(const float *matrices, const uint8_t *src, uint32_t src_size, uint32_t src_levels, uint8_t *out, uint32_t out_size,
                                uint32_t lanes)
{
	if (diffuse_steps(2.0f * SHADER_PI) != DIFFUSE_PHI_STEPS || diffuse_steps(0.5f * SHADER_PI) != DIFFUSE_THETA_STEPS)
		return -1;
	const Cube cube = {src, src_size, src_levels};
	const float lod = log2f(float(out_size)) - 5.0f;
	const CubeLevel l = cube_level(cube, nearest_level(lod > 0.0f ? lod : 0.0f, src_levels));
	std::vector<SinCos> phi(DIFFUSE_PHI_STEPS), theta(DIFFUSE_THETA_STEPS);
	for (uint32_t k = 0; k < DIFFUSE_PHI_STEPS; k++)
		phi[k] = {sinf(diffuse_angle(k)), cosf(diffuse_angle(k))};
	for (uint32_t k = 0; k < DIFFUSE_THETA_STEPS; k++)
		theta[k] = {sinf(diffuse_angle(k)), cosf(diffuse_angle(k))};
	uint2 *dst = reinterpret_cast<uint2 *>(out);
	for (uint32_t face = 0; face < 6; face++)
		for (uint32_t y = 0; y < out_size; y++)
			for (uint32_t x = 0; x < out_size; x++)
			{
				const Frame frame = diffuse_frame(texel_direction(matrices + 16 * face, int(out_size), int(x), int(y)));
				std::vector<f3> sums(lanes, f3{0.0f, 0.0f, 0.0f});
				for (uint32_t lane = 0; lane < lanes; lane++)
					diffuse_accumulate(l, frame, phi.data(), theta.data(), lane, lanes, sums[lane]);
				dst[(face * out_size + y) * out_size + x] = pack_rgba(diffuse_resolve(butterfly3(sums)), 1.0f);
			}
	return 0;
}

// One bilinear tap of one level along `dir`; which face it lands on and its (s, t).
extern "C" int env_host_sample(const uint8_t *src, uint32_t src_size, uint32_t src_levels, uint32_t level, const float *dir, float *rgb, float *st)
{
	const Cube cube = {src, src_size, src_levels};
	const CubeLevel l = cube_level(cube, level);
	const f3 d = {dir[0], dir[1], dir[2]};
	const f3 r = sample_cube(l, l, 0.0f, d);
	rgb[0] = r.x;
	rgb[1] = r.y;
	rgb[2] = r.z;
	float sc, tc, ma;
	const int face = select_face(d, sc, tc, ma);
	st[0] = sc * (0.5f / ma) + 0.5f;
	st[1] = tc * (0.5f / ma) + 0.5f;
	return face;
}
