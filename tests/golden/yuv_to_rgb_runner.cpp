// TEST INFRASTRUCTURE ONLY -- used by make_yuv_to_rgb_golden.py to record tests/golden/yuv_to_rgb_shader_v1.npz.
//
// Runs the reference's util/yuv_to_rgb.comp on the CPU: the shader is re-spelled into gen/ by oracle/ref_build/glsl2cpp.py at
// generation time (a temporary directory, removed afterwards) and compiled as C++ against oracle/ref_build/glsl_cpu.hpp.  The three
// specialisation constants stay compile-time ones: each object built from this file holds one set (-DSPEC_PQ, -DSPEC_NUM_PLANES,
// -DSPEC_NV21) and registers it; the object built with -DYUV_ENTRY holds the registry and the entry point.
//
// One invocation per output pixel in 8 x 8 groups, edge groups included, with gl_GlobalInvocationID / gl_LocalInvocationID /
// gl_WorkGroupID set per invocation; the luma texture is sampled NearestClamp, the chroma textures LinearClamp (dispatch_conversion),
// and planes the shader does not use are bound to the luma plane as the reference binds them.
#include <vector>
#include "glsl_cpu.hpp"

namespace yuv
{
struct Call
{
	glsl::Texture planes[3];
	glsl::Image output;
	float yuv_to_rgb[16], primary_conversion[16]; // column major
	unsigned resolution[2];
	float inv_resolution[2], chroma_siting[2], chroma_clamp[2], unorm_rescale;
};
struct Variant
{
	int pq, num_planes, nv21;
	void (*run)(const Call &call);
};
std::vector<Variant> &registry();
} // namespace yuv

#ifndef YUV_ENTRY
namespace
{
constexpr int spec[3] = {SPEC_PQ, SPEC_NUM_PLANES, SPEC_NV21}; // the generated text forgets the macros at its end
}

namespace glsl
{
namespace // every object holds its own specialisation of the shader
{
namespace yuv_to_rgb_shader
{
static constexpr struct
{
	unsigned x = 8, y = 8, z = 1;
} gl_WorkGroupSize; // layout(local_size_x = 8, local_size_y = 8) in;
#include "gen/yuv_to_rgb.inc"
} // namespace yuv_to_rgb_shader
} // namespace
} // namespace glsl

namespace yuv
{
namespace
{
void run(const Call &call)
{
	using namespace glsl;
	namespace s = glsl::yuv_to_rgb_shader;
	s::uOutput = call.output;
	s::uY = call.planes[0];
	s::uCb = call.planes[1];
	s::uCr = call.planes[2];
	for (int c = 0; c < 4; c++)
	{
		s::yuv_to_rgb[c] = vec4(call.yuv_to_rgb[4 * c], call.yuv_to_rgb[4 * c + 1], call.yuv_to_rgb[4 * c + 2], call.yuv_to_rgb[4 * c + 3]);
		s::primary_conversion[c] = vec4(call.primary_conversion[4 * c], call.primary_conversion[4 * c + 1], call.primary_conversion[4 * c + 2],
		                                call.primary_conversion[4 * c + 3]);
	}
	s::resolution = uvec2(call.resolution[0], call.resolution[1]);
	s::inv_resolution = vec2(call.inv_resolution[0], call.inv_resolution[1]);
	s::chroma_siting = vec2(call.chroma_siting[0], call.chroma_siting[1]);
	s::chroma_clamp = vec2(call.chroma_clamp[0], call.chroma_clamp[1]);
	s::unorm_rescale = call.unorm_rescale;
	const unsigned groups_x = (call.resolution[0] + 7) / 8, groups_y = (call.resolution[1] + 7) / 8;
	for (unsigned gy = 0; gy < groups_y; gy++)
		for (unsigned gx = 0; gx < groups_x; gx++)
			for (unsigned ly = 0; ly < 8; ly++)
				for (unsigned lx = 0; lx < 8; lx++)
				{
					gl_WorkGroupID = uvec3(gx, gy, 0u);
					gl_LocalInvocationID = uvec3(lx, ly, 0u);
					gl_LocalInvocationIndex = ly * 8 + lx;
					gl_GlobalInvocationID = uvec3(gx * 8 + lx, gy * 8 + ly, 0u);
					s::main();
				}
}

const bool registered = (registry().push_back({spec[0], spec[1], spec[2], run}), true);
} // namespace
} // namespace yuv

#else // YUV_ENTRY
namespace yuv
{
std::vector<Variant> &registry()
{
	static std::vector<Variant> variants;
	return variants;
}
} // namespace yuv

// One dispatch.  planes: tightly packed R8 (luma, planar chroma) or R8G8 (interleaved chroma) texels of plane_w x plane_h;
// ubo: the 41 floats yuv_to_rgb[16], primary_conversion[16], inv_resolution[2], chroma_siting[2], chroma_clamp[2], unorm_rescale,
// bit for bit; out: width x height texels, R8G8B8A8_UNORM without PQ and R16G16B16A16_SFLOAT with it.  Returns -1 when this set
// of specialisation constants was not built.
extern "C" int ref_yuv_to_rgb(int pq, int num_planes, int nv21, const void *const *planes, const int *plane_w, const int *plane_h, int width,
                              int height, const float *ubo, void *out)
{
	const yuv::Variant *variant = nullptr;
	for (const auto &v : yuv::registry())
		if (v.pq == pq && v.num_planes == num_planes && v.nv21 == nv21)
			variant = &v;
	if (!variant)
		return -1;
	yuv::Call call = {};
	for (int i = 0; i < 3; i++)
	{
		const int src = i < num_planes ? i : 0; // unused bindings see the luma plane, NearestClamp
		call.planes[i].data = planes[src];
		call.planes[i].w = plane_w[src];
		call.planes[i].h = plane_h[src];
		call.planes[i].format = num_planes == 2 && src == 1 ? glsl::Format::RG8_UNORM : glsl::Format::R8_UNORM;
		call.planes[i].filter = src == 0 ? glsl::Filter::Nearest : glsl::Filter::Linear;
	}
	call.output.data = out;
	call.output.w = width;
	call.output.h = height;
	call.output.format = pq ? glsl::Format::RGBA16F : glsl::Format::RGBA8_UNORM;
	memcpy(call.yuv_to_rgb, ubo, sizeof(call.yuv_to_rgb));
	memcpy(call.primary_conversion, ubo + 16, sizeof(call.primary_conversion));
	call.resolution[0] = unsigned(width);
	call.resolution[1] = unsigned(height);
	memcpy(call.inv_resolution, ubo + 32, 8);
	memcpy(call.chroma_siting, ubo + 34, 8);
	memcpy(call.chroma_clamp, ubo + 36, 8);
	call.unorm_rescale = ubo[38];
	variant->run(call);
	return 0;
}
#endif
