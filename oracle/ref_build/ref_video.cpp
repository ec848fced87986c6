// ORACLE — TEST INFRASTRUCTURE ONLY.
//
// Runs the REFERENCE's own video scaler on the CPU: util/scaler.comp, re-spelled into gen/ at build time, under the specialisation
// constants VideoScaler::rescale sets (video/scaler.cpp:283-287: CONTROL, EOTF, OETF, OUTPUT_PLANES).  CONTROL sizes the shader's
// shared arrays, so the constants stay compile-time ones: each object built from this file holds one combination (the Makefile's
// VIDEO_VARIANTS, -DSPEC_*) and registers it; the object built with -DVIDEO_ENTRY holds the registry and the entry point.
//
// A workgroup is a team of 64 real threads, one 64-lane subgroup (local_index = invocation index); barrier() is a team barrier;
// quad swaps exchange through a per-quad rendezvous (the shader swaps with every lane active).  Workgroups cover the output grid of
// 8 x 8 tiles, edge tiles included, one after the other; stores outside an image are dropped.
//
// texelFetch outside the input reads zero.  That is an ASSUMPTION: robust image access, which the kernel and tests/video_ref.py take
// on the same-size path, where the shader fetches without clamping (the rescale path clamps with CLAMP_COORD first).
#include <barrier>
#include <memory>
#include <thread>
#include <vector>
#include "glsl_cpu.hpp"

namespace video
{
// What one specialisation needs from the caller; the weight table is the fp16 one of gr_video_scaler_weights, widened.
struct Call
{
	glsl::Texture input;
	glsl::Image planes[3];
	int num_planes;
	float gamma_space_transform[12]; // row major 3 x 4
	float primary_transform[9];      // column major
	int resolution[2];
	float scaling_to_input[2], inv_input_resolution[2], dither_strength;
	const glsl::f16vec2 *weights;
};
struct Variant
{
	int control, eotf, oetf, planes;
	void (*run)(const Call &call, int groups_x, int groups_y);
};
std::vector<Variant> &registry();

#ifndef VIDEO_ENTRY
namespace
{
constexpr int spec[4] = {SPEC_CONTROL, SPEC_EOTF, SPEC_OETF, SPEC_OUTPUT_PLANES}; // gen/scaler.inc forgets the macros at its end
std::barrier<> *team_barrier = nullptr;
std::unique_ptr<std::barrier<>> quad_barriers[16];
glsl::vec2 quad_slots[64];

glsl::vec2 quad_exchange(const glsl::vec2 &v, unsigned partner_xor)
{
	const unsigned lane = glsl::gl_SubgroupInvocationID;
	quad_slots[lane] = v;
	quad_barriers[lane >> 2]->arrive_and_wait();
	const glsl::vec2 other = quad_slots[lane ^ partner_xor];
	quad_barriers[lane >> 2]->arrive_and_wait();
	return other;
}
} // namespace
} // namespace video

namespace glsl
{
namespace // every object holds its own specialisation of the shader
{
static inline void barrier() { video::team_barrier->arrive_and_wait(); }
static inline vec2 subgroupQuadSwapHorizontal(const vec2 &v) { return video::quad_exchange(v, 1); }
static inline vec2 subgroupQuadSwapVertical(const vec2 &v) { return video::quad_exchange(v, 2); }
#define sampler2D(t, s) combined_sampler(t, s)
namespace scaler
{
static constexpr struct
{
	unsigned x = 64, y = 1, z = 1;
} gl_WorkGroupSize; // layout(local_size_x = 64) in;
#include "gen/scaler.inc"
}
#undef sampler2D
} // namespace
} // namespace glsl

namespace video
{
namespace
{
void run(const Call &call, int groups_x, int groups_y)
{
	using namespace glsl;
	namespace s = glsl::scaler;
	s::uTexture = call.input;
	s::uLinearSampler = sampler();
	s::uOutput = call.planes[0];
	if (call.num_planes > 1)
		s::uChromaPlane2 = call.planes[1];
	if (call.num_planes > 2)
		s::uChromaPlane3 = call.planes[2];
	s::weights = const_cast<f16vec2 *>(call.weights);
	// the row_major mat4x3 by meaning: gamma_space_transform * v = (row0 . v, row1 . v, row2 . v), so column j = (row0[j], row1[j], row2[j])
	for (int j = 0; j < 4; j++)
		s::ubo.gamma_space_transform[j] = vec3(call.gamma_space_transform[j], call.gamma_space_transform[4 + j], call.gamma_space_transform[8 + j]);
	for (int j = 0; j < 3; j++)
		s::ubo.primary_transform[j] = vec3(call.primary_transform[3 * j], call.primary_transform[3 * j + 1], call.primary_transform[3 * j + 2]);
	s::registers.resolution = ivec2(call.resolution[0], call.resolution[1]);
	s::registers.scaling_to_input = vec2(call.scaling_to_input[0], call.scaling_to_input[1]);
	s::registers.inv_input_resolution = vec2(call.inv_input_resolution[0], call.inv_input_resolution[1]);
	s::registers.dither_strength = call.dither_strength;

	std::barrier<> sync(64);
	team_barrier = &sync;
	for (auto &q : quad_barriers)
		q = std::make_unique<std::barrier<>>(4);
	std::vector<std::thread> threads;
	for (unsigned i = 0; i < 64; i++)
		threads.emplace_back([=, &sync]() {
			gl_LocalInvocationIndex = i;
			gl_LocalInvocationID = uvec3(i, 0u, 0u);
			gl_SubgroupSize = 64;
			gl_NumSubgroups = 1;
			gl_SubgroupID = 0;
			gl_SubgroupInvocationID = i;
			for (int gy = 0; gy < groups_y; gy++)
				for (int gx = 0; gx < groups_x; gx++)
				{
					gl_WorkGroupID = uvec3(uint(gx), uint(gy), 0u);
					s::main();
					sync.arrive_and_wait(); // the next group reuses the shared arrays
				}
		});
	for (auto &t : threads)
		t.join();
	team_barrier = nullptr;
}

const bool registered = (registry().push_back({spec[0], spec[1], spec[2], spec[3], run}), true);
} // namespace
} // namespace video

#else // VIDEO_ENTRY
std::vector<Variant> &registry()
{
	static std::vector<Variant> variants;
	return variants;
}
} // namespace video

namespace
{
// VkFormat values of the formats gr_video_scale takes (include/granite_hip.h)
glsl::Format input_format(int vk)
{
	switch (vk)
	{
	case 37: return glsl::Format::RGBA8_UNORM;
	case 43: return glsl::Format::RGBA8_SRGB;
	case 64: return glsl::Format::A2B10G10R10_UNORM;
	default: return glsl::Format::RGBA16F; // 97
	}
}

// Storage views of the output planes: UNORM (the shader applies the OETF itself, so an *_SRGB plane is written through a UNORM view)
bool output_format(int vk, glsl::Format &f)
{
	switch (vk)
	{
	case 9: f = glsl::Format::R8_UNORM; return true;
	case 16: f = glsl::Format::RG8_UNORM; return true;
	case 70: f = glsl::Format::R16_UNORM; return true;
	case 77: f = glsl::Format::RG16_UNORM; return true;
	case 37: case 43: f = glsl::Format::RGBA8_UNORM; return true;
	case 44: case 50: f = glsl::Format::BGRA8_UNORM; return true;
	default: return false;
	}
}
} // namespace

// One scaler.comp dispatch over the output grid of planes[0].  input: tightly packed texels; planes: tightly packed outputs of
// plane_w x plane_h in VkFormat plane_fmt; control / eotf / oetf / the matrices / push constants: gr_video_scale_plan's;
// weights: gr_video_scaler_weights' fp16 table (2 x 256 x 8 bits).  Returns -1 when this combination of specialisation
// constants was not built (VIDEO_VARIANTS in the Makefile) or a format is unknown.
extern "C" int ref_video_scale(const void *input, int in_w, int in_h, int in_format, int num_planes, void *const *planes, const int *plane_w,
                               const int *plane_h, const int *plane_fmt, int control, int eotf, int oetf, const float *gamma_space_transform,
                               const float *primary_transform, const int *resolution, const float *scaling_to_input,
                               const float *inv_input_resolution, float dither_strength, const uint16_t *weights)
{
	const video::Variant *variant = nullptr;
	for (const auto &v : video::registry())
		if (v.control == control && v.eotf == eotf && v.oetf == oetf && v.planes == num_planes)
			variant = &v;
	if (!variant || num_planes < 1 || num_planes > 3)
		return -1;
	video::Call call = {};
	call.input.data = input;
	call.input.w = in_w;
	call.input.h = in_h;
	call.input.format = input_format(in_format);
	call.input.fetch_zero_outside = true;
	call.num_planes = num_planes;
	for (int i = 0; i < num_planes; i++)
	{
		call.planes[i].data = planes[i];
		call.planes[i].w = plane_w[i];
		call.planes[i].h = plane_h[i];
		if (!output_format(plane_fmt[i], call.planes[i].format))
			return -1;
	}
	memcpy(call.gamma_space_transform, gamma_space_transform, sizeof(call.gamma_space_transform));
	memcpy(call.primary_transform, primary_transform, sizeof(call.primary_transform));
	memcpy(call.resolution, resolution, sizeof(call.resolution));
	memcpy(call.scaling_to_input, scaling_to_input, sizeof(call.scaling_to_input));
	memcpy(call.inv_input_resolution, inv_input_resolution, sizeof(call.inv_input_resolution));
	call.dither_strength = dither_strength;
	std::vector<glsl::f16vec2> table(2 * 256 * 4);
	for (size_t i = 0; i < table.size(); i++)
		table[i] = glsl::f16vec2(glsl::uint16BitsToHalf(weights[2 * i]), glsl::uint16BitsToHalf(weights[2 * i + 1]));
	call.weights = table.data();
	variant->run(call, (plane_w[0] + 7) / 8, (plane_h[0] + 7) / 8);
	return 0;
}
#endif
