// TEST INFRASTRUCTURE ONLY -- used by make_shadow_golden.py to record tests/golden/shadow_shader_v1.npz.
//
// Runs the reference's lights/directional.frag with SHADOWS (one compile of this file per define set: -DSHADOW_VARIANT=<name> and the
// shader's own defines on the command line), and lights/resolve_vsm.frag, post/vsm_down_blur.frag and post/vsm_up_blur.frag (LAYERED 0 and 1;
// -DSHADOW_VSM_CHAIN) on the CPU: re-spelled into gen/ by oracle/ref_build/glsl2cpp.py at generation time (a temporary directory, removed
// afterwards) and compiled as C++ against oracle/ref_build/glsl_cpu.hpp with -ffp-contract=off.  What glsl_cpu.hpp lacks is supplied here:
//   sampler2DShadow, sampler2DArrayShadow       a D16_UNORM (v / 65535) or D32_SFLOAT map of one or four layers behind the LinearShadow
//                                               sampler (vulkan/device.cpp: compare GREATER_OR_EQUAL, linear, clamp to edge)
//   texture(vec4), textureProjLod               the footprint and weights of glsl_cpu.hpp's LinearClamp fetch (orc::linear_axis, with its
//                                               snap; orc::linear_combine); every texel, clamped to the edge, is compared first -- 1 where
//                                               ref >= texel, else 0 -- and the weights blend the four results
//   textureGather[Offset] with a reference      the four compare results of the footprint at floor(uv * size - 0.5) + offset, in the
//                                               component order of glsl_cpu.hpp's textureGatherOffset
//   sampler2DArray, textureLod, textureSize     R32G32_SFLOAT moments through LinearClamp; for the variants without layers the shader's
//                                               `sampler2D` is spelled as the same type
//   subpassLoad of a depth attachment, gl_ViewIndex
// What the rasteriser provides is stated as oracle/ref_build/ref_lighting.cpp states it: gl_FragCoord = pixel centre, vClip =
// inv_view_projection * (ndc, 0, 1) at the pixel centre, depth test NOT_EQUAL against the quad's z = 0, blending ONE / ONE into the
// RGBA16F target; the blur's vUV is the output pixel's centre over the output's size.
#include <cmath>
#include <cstdint>
#include <cstring>
#include "glsl_cpu.hpp"

using namespace glsl;

enum MapFormat : int32_t { MAP_D16 = 0, MAP_D32 = 1, MAP_RG32F = 2 };
struct MapData
{
	const void *data = nullptr;
	int w = 0, h = 0, layers = 1;
	int32_t format = MAP_D16;
	size_t at(int x, int y, int layer) const
	{
		x = orc::clampi(x, 0, w - 1);
		y = orc::clampi(y, 0, h - 1);
		layer = orc::clampi(layer, 0, layers - 1);
		return (size_t(layer) * h + y) * w + x;
	}
	float depth(int x, int y, int layer) const
	{
		const size_t i = at(x, y, layer);
		if (format == MAP_D16)
			return float(static_cast<const uint16_t *>(data)[i]) / 65535.0f;
		return static_cast<const float *>(data)[i];
	}
	vec2 moments(int x, int y, int layer) const
	{
		const float *p = static_cast<const float *>(data) + 2 * at(x, y, layer);
		return vec2(p[0], p[1]);
	}
};
struct sampler2DShadow : MapData {};
struct sampler2DArrayShadow : MapData {};
struct sampler2DArray : MapData {};
struct MomentSampler2D : MapData {};
struct DepthAttachment : MapData {};

static inline float compare_ge(float ref, float texel) { return ref >= texel ? 1.0f : 0.0f; }
static inline float shadow_fetch(const MapData &t, const vec2 &uv, int layer, float ref)
{
	float a, b;
	int x0, y0;
	orc::linear_axis(uv.x * float(t.w) - 0.5f, x0, a);
	orc::linear_axis(uv.y * float(t.h) - 0.5f, y0, b);
	return orc::linear_combine(compare_ge(ref, t.depth(x0, y0, layer)), compare_ge(ref, t.depth(x0 + 1, y0, layer)), compare_ge(ref, t.depth(x0, y0 + 1, layer)),
	                           compare_ge(ref, t.depth(x0 + 1, y0 + 1, layer)), a, b);
}
static inline vec4 shadow_gather(const MapData &t, const vec2 &uv, int layer, float ref, const ivec2 &o)
{
	const int i0 = int(floorf(uv.x * float(t.w) - 0.5f)) + o.x, j0 = int(floorf(uv.y * float(t.h) - 0.5f)) + o.y;
	return vec4(compare_ge(ref, t.depth(i0, j0 + 1, layer)), compare_ge(ref, t.depth(i0 + 1, j0 + 1, layer)), compare_ge(ref, t.depth(i0 + 1, j0, layer)),
	            compare_ge(ref, t.depth(i0, j0, layer)));
}
static inline vec4 moment_fetch(const MapData &t, const vec2 &uv, int layer)
{
	float a, b;
	int x0, y0;
	orc::linear_axis(uv.x * float(t.w) - 0.5f, x0, a);
	orc::linear_axis(uv.y * float(t.h) - 0.5f, y0, b);
	const vec2 m = orc::linear_combine(t.moments(x0, y0, layer), t.moments(x0 + 1, y0, layer), t.moments(x0, y0 + 1, layer), t.moments(x0 + 1, y0 + 1, layer), a, b);
	return vec4(m.x, m.y, 0.0f, 1.0f);
}

static inline float texture(const sampler2DArrayShadow &t, const vec4 &p) { return shadow_fetch(t, vec2(p.x, p.y), int(p.z), p.w); }
static inline float textureProjLod(const sampler2DShadow &t, const vec4 &p, float) { return shadow_fetch(t, vec2(p.x / p.w, p.y / p.w), 0, p.z / p.w); }
static inline vec4 textureGatherOffset(const sampler2DShadow &t, const vec2 &uv, float ref, const ivec2 &o) { return shadow_gather(t, uv, 0, ref, o); }
static inline vec4 textureGather(const sampler2DShadow &t, const vec2 &uv, float ref) { return shadow_gather(t, uv, 0, ref, ivec2(0, 0)); }
static inline vec4 textureGatherOffset(const sampler2DArrayShadow &t, const vec3 &uv, float ref, const ivec2 &o) { return shadow_gather(t, vec2(uv.x, uv.y), int(uv.z), ref, o); }
static inline vec4 textureGather(const sampler2DArrayShadow &t, const vec3 &uv, float ref) { return shadow_gather(t, vec2(uv.x, uv.y), int(uv.z), ref, ivec2(0, 0)); }
static inline ivec2 textureSize(const sampler2DShadow &t, int) { return ivec2(t.w, t.h); }
static inline ivec3 textureSize(const sampler2DArrayShadow &t, int) { return ivec3(t.w, t.h, t.layers); }
static inline vec4 textureLod(const sampler2DArray &t, const vec3 &uv, float) { return moment_fetch(t, vec2(uv.x, uv.y), int(uv.z)); }
static inline vec4 textureLod(const MomentSampler2D &t, const vec2 &uv, float) { return moment_fetch(t, uv, 0); }
static inline vec4 subpassLoad(const DepthAttachment &t) { return vec4(t.depth(int(gl_FragCoord.x), int(gl_FragCoord.y), 0), 0.0f, 0.0f, 1.0f); }
static thread_local int gl_ViewIndex = 0;

static inline MapData map_of(const void *data, int w, int h, int layers, int32_t format)
{
	MapData m;
	m.data = data, m.w = w, m.h = h, m.layers = layers, m.format = format;
	return m;
}

#if defined(SHADOW_VSM_CHAIN)
// ---- resolve_vsm.frag and the two blurs ---------------------------------------------------------------------------------------------
namespace resolve
{
#define subpassInput DepthAttachment
#include "gen/resolve_vsm.inc"
#undef subpassInput
}
#define LAYERED 0
#define sampler2D MomentSampler2D
namespace down_plain
{
#include "gen/vsm_down_blur.inc"
}
#undef SAMPLE_OFFSET
namespace up_plain
{
#include "gen/vsm_up_blur.inc"
}
#undef SAMPLE_OFFSET
#undef sampler2D
#undef LAYERED
#define LAYERED 1
namespace down_layered
{
#include "gen/vsm_down_blur.inc"
}
#undef SAMPLE_OFFSET
namespace up_layered
{
#include "gen/vsm_up_blur.inc"
}
#undef SAMPLE_OFFSET
#undef LAYERED

extern "C" {
// depth: w x h texels of `format` (MAP_D16 / MAP_D32) -> moments: w x h x 2 floats
void ref_vsm_moments(const void *depth, int32_t format, int32_t w, int32_t h, float *moments)
{
	static_cast<MapData &>(resolve::uDepth) = map_of(depth, w, h, 1, format);
	for (int y = 0; y < h; y++)
		for (int x = 0; x < w; x++)
		{
			gl_FragCoord = vec4(float(x) + 0.5f, float(y) + 0.5f, 0.0f, 1.0f);
			resolve::main();
			moments[2 * (size_t(y) * w + x)] = resolve::FragColor.x;
			moments[2 * (size_t(y) * w + x) + 1] = resolve::FragColor.y;
		}
}

// in: layers x in_h x in_w x 2 floats -> out: layers x out_h x out_w x 2 floats; layered 0 runs the sampler2D form once per layer (on that
// layer's image alone), layered 1 the multiview form with gl_ViewIndex = layer
void ref_vsm_blur(const float *in, int32_t in_w, int32_t in_h, int32_t layers, float *out, int32_t out_w, int32_t out_h, int32_t up, int32_t layered)
{
	for (int layer = 0; layer < layers; layer++)
	{
		const float *plane = in + size_t(layer) * in_w * in_h * 2;
		const vec2 inv_texel_size(1.0f / float(in_w), 1.0f / float(in_h));
		if (layered)
		{
			static_cast<MapData &>(down_layered::uSampler) = map_of(in, in_w, in_h, layers, MAP_RG32F);
			static_cast<MapData &>(up_layered::uSampler) = map_of(in, in_w, in_h, layers, MAP_RG32F);
			down_layered::registers.inv_texel_size = up_layered::registers.inv_texel_size = inv_texel_size;
			gl_ViewIndex = layer;
		}
		else
		{
			static_cast<MapData &>(down_plain::uSampler) = map_of(plane, in_w, in_h, 1, MAP_RG32F);
			static_cast<MapData &>(up_plain::uSampler) = map_of(plane, in_w, in_h, 1, MAP_RG32F);
			down_plain::registers.inv_texel_size = up_plain::registers.inv_texel_size = inv_texel_size;
		}
		for (int y = 0; y < out_h; y++)
			for (int x = 0; x < out_w; x++)
			{
				const vec2 uv((float(x) + 0.5f) / float(out_w), (float(y) + 0.5f) / float(out_h));
				vec2 value;
				if (layered && up)
					up_layered::vUV = uv, up_layered::main(), value = up_layered::FragColor;
				else if (layered)
					down_layered::vUV = uv, down_layered::main(), value = down_layered::FragColor;
				else if (up)
					up_plain::vUV = uv, up_plain::main(), value = up_plain::FragColor;
				else
					down_plain::vUV = uv, down_plain::main(), value = down_plain::FragColor;
				float *o = out + ((size_t(layer) * out_h + y) * out_w + x) * 2;
				o[0] = value.x, o[1] = value.y;
			}
	}
	gl_ViewIndex = 0;
}

void ref_srgb_table(float *table)
{
	for (int i = 0; i < 256; i++)
		table[i] = orc::srgb8_to_float(uint8_t(i));
}
}

#else
// ---- directional.frag, one define set --------------------------------------------------------------------------------------------------
#define STAGE_FRAGMENT 1
#if defined(DIRECTIONAL_SHADOW_VSM) && !defined(SHADOW_CASCADES)
#define sampler2D MomentSampler2D // uShadowmap; the variant has no ambient-occlusion texture and does not read uBRDFLut
#endif
#define SHADOW_PASTE2(a, b) a##b
#define SHADOW_PASTE(a, b) SHADOW_PASTE2(a, b)
#define SHADER_NAMESPACE SHADOW_PASTE(shader_, SHADOW_VARIANT) // the objects of all define sets are linked into one library
namespace SHADER_NAMESPACE
{
#include "gen/directional.inc"
}
#undef sampler2D

struct ShadowRun
{
	const uint32_t *albedo, *normal;
	const uint16_t *pbr;
	const float *depth;
	const uint16_t *emissive;
	const uint8_t *ambient_occlusion;
	const void *maps;
	uint16_t *hdr;     // width x height x 4 halves, out
	float *colour;     // width x height x 3, out: FragColor before the blend (0 on the far plane)
	float *term;       // width x height, out: get_directional_shadow_term (1 on the far plane)
	int32_t *layers;   // width x height x 2, out: layer_near, layer_far (cascaded variants)
	float *lerps;      // width x height x 2, out: shadow_lerp, white_lerp (cascaded variants)
	int32_t width, height, ao_width, ao_height, map_width, map_height, map_layers, map_format;
	float inv_view_projection[16], transforms[64];
	float color[3], camera_pos[3], direction[3], camera_front[3];
	float cascade_log_bias;
};

extern "C" void SHADOW_PASTE(ref_shadow_directional_, SHADOW_VARIANT)(const ShadowRun *r)
{
	namespace s = SHADER_NAMESPACE;
	const int W = r->width, H = r->height;
	auto make = [](const void *data, int w, int h, Format f, Filter filter = Filter::Nearest) {
		Texture t;
		t.data = data, t.w = w, t.h = h, t.format = f, t.filter = filter;
		return t;
	};
	mat4 inv_vp;
	for (int c = 0; c < 4; c++)
		inv_vp.c[c] = vec4(r->inv_view_projection[4 * c], r->inv_view_projection[4 * c + 1], r->inv_view_projection[4 * c + 2], r->inv_view_projection[4 * c + 3]);
	for (int i = 0; i < 4; i++)
		for (int c = 0; c < 4; c++)
			s::shadows.transforms[i].c[c] = vec4(r->transforms[16 * i + 4 * c], r->transforms[16 * i + 4 * c + 1], r->transforms[16 * i + 4 * c + 2], r->transforms[16 * i + 4 * c + 3]);
	s::shadows.inverse_view_projection = inv_vp;
	const vec2 inv_resolution(1.0f / float(W), 1.0f / float(H));
	s::BaseColor = make(r->albedo, W, H, Format::RGBA8_SRGB);
	s::Normal = make(r->normal, W, H, Format::A2B10G10R10_UNORM);
	s::PBR = make(r->pbr, W, H, Format::RG8_UNORM);
	s::Depth = make(r->depth, W, H, Format::R32F);
#if defined(AMBIENT_OCCLUSION)
	s::uAmbientOcclusion = make(r->ambient_occlusion, r->ao_width, r->ao_height, Format::R8_UNORM, Filter::Linear);
#endif
	static_cast<MapData &>(s::uShadowmap) = map_of(r->maps, r->map_width, r->map_height, r->map_layers, r->map_format);
	s::registers.inverse_view_projection_col2 = inv_vp.c[2];
	s::registers.color = vec3(r->color[0], r->color[1], r->color[2]);
	s::registers.camera_pos = vec3(r->camera_pos[0], r->camera_pos[1], r->camera_pos[2]);
	s::registers.direction = vec3(r->direction[0], r->direction[1], r->direction[2]);
	s::registers.camera_front = vec3(r->camera_front[0], r->camera_front[1], r->camera_front[2]);
	s::registers.cascade_log_bias = r->cascade_log_bias;
	s::registers.inv_resolution = inv_resolution;

	for (int y = 0; y < H; y++)
		for (int x = 0; x < W; x++)
		{
			const size_t pixel = size_t(y) * W + x;
			uint16_t *out = r->hdr + pixel * 4;
			memcpy(out, r->emissive + pixel * 4, 8);
			r->term[pixel] = 1.0f;
			r->colour[3 * pixel] = r->colour[3 * pixel + 1] = r->colour[3 * pixel + 2] = 0.0f;
			if (r->depth[pixel] == 0.0f)
				continue;
			gl_FragCoord = vec4(float(x) + 0.5f, float(y) + 0.5f, 0.0f, 1.0f);
			const vec2 ndc(2.0f * ((float(x) + 0.5f) * inv_resolution.x) - 1.0f, 2.0f * ((float(y) + 0.5f) * inv_resolution.y) - 1.0f);
			s::vClip = inv_vp * vec4(ndc.x, ndc.y, 0.0f, 1.0f);
			s::main();
			for (int c = 0; c < 3; c++)
			{
				r->colour[3 * pixel + c] = s::FragColor.d[c];
				out[c] = orc::float_to_half_rne(orc::half_to_float(out[c]) + s::FragColor.d[c]);
			}
			// the shader's own intermediate results at this fragment, by its own functions
			const vec4 clip = s::vClip + r->depth[pixel] * s::registers.inverse_view_projection_col2;
			const vec3 pos = clip.xyz / clip.w;
			r->term[pixel] = s::get_directional_shadow_term(pos, s::registers.camera_pos, s::registers.camera_front, s::registers.direction);
#if defined(SHADOW_CASCADES)
			vec3 clip_near, clip_far;
			float shadow_lerp, white_lerp;
			int layer_near, layer_far;
			s::compute_shadow_cascade(clip_near, clip_far, shadow_lerp, white_lerp, layer_near, layer_far, pos, s::registers.camera_pos, s::registers.camera_front,
			                          s::registers.direction);
			r->layers[2 * pixel] = layer_near, r->layers[2 * pixel + 1] = layer_far;
			r->lerps[2 * pixel] = shadow_lerp, r->lerps[2 * pixel + 1] = white_lerp;
#endif
		}
}
#endif
