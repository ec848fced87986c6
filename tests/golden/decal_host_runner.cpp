// TEST INFRASTRUCTURE ONLY -- used by make_decal_golden.py to record the host-side part of tests/golden/decal_shader_v1.npz.
//
// Calls the reference's own math library on a decal's world transform, the way oracle/ref_build/ref_shim.cpp calls it: this file only
// includes the reference's headers at generation time (math/simd.hpp, math/aabb.hpp, math/muglm) and is compiled with muglm.cpp from where
// it lies, with the flags of oracle/ref_build/Makefile's libref_muglm.so (-ffp-contract=off -msse4.1, the SSE4.1 paths of simd.hpp).
// What the reference does with a decal on the host, statement by statement:
//   sort key          dot(front, transform->get_aabb().get_center())           clusterer.cpp:1124-1131; the AABB is
//                     SIMD::transform_aabb(static AABB, world transform)       scene.cpp:773, VolumetricDecal::get_static_aabb() = +-0.5
//   world_to_texture  mat_affine(inverse(texture_to_world.to_mat4()))          scene.cpp:733-736
//   z range           SIMD::mul(world, transform, vec4(corner, 1)); dot(world.xyz() - pos, front); min / max   clusterer.cpp:1348-1369
//   mvp               SIMD::mul(mvp, view_projection, world.to_mat4())         clusterer.cpp:1406-1410
#include <cstring>
#include <limits>
#include "simd.hpp"
#include "aabb.hpp"
#include "muglm/muglm_impl.hpp"
#include "muglm/matrix_helper.hpp"

using namespace muglm;
using namespace Granite;

extern "C" void ref_decal_host(const float *world_rows12, const float *view_projection16, const float *camera_position3, const float *camera_front3,
                               float *sort_key, float *world_to_texture12, float *z_range2, float *mvp16)
{
	const mat_affine transform(vec4(world_rows12[0], world_rows12[1], world_rows12[2], world_rows12[3]), vec4(world_rows12[4], world_rows12[5], world_rows12[6], world_rows12[7]),
	                           vec4(world_rows12[8], world_rows12[9], world_rows12[10], world_rows12[11]));
	const vec3 pos(camera_position3[0], camera_position3[1], camera_position3[2]), front(camera_front3[0], camera_front3[1], camera_front3[2]);
	const AABB static_aabb(vec3(-0.5f), vec3(0.5f));

	AABB world_aabb(vec3(0.0f), vec3(0.0f));
	SIMD::transform_aabb(world_aabb, static_aabb, transform);
	*sort_key = dot(front, world_aabb.get_center());

	const mat_affine world_to_texture(inverse(transform.to_mat4()));
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 4; c++)
			world_to_texture12[4 * r + c] = world_to_texture[r][c];

	float lo = std::numeric_limits<float>::infinity();
	float hi = -lo;
	for (unsigned i = 0; i < 8; i++)
	{
		vec4 world_space;
		vec4 texel_space = vec4(static_aabb.get_corner(i), 1.0f);
		SIMD::mul(world_space, transform, texel_space);
		float z = dot(world_space.xyz() - pos, front);
		lo = std::min(lo, z);
		hi = std::max(hi, z);
	}
	z_range2[0] = lo;
	z_range2[1] = hi;

	mat4 vp, mvp;
	memcpy(&vp, view_projection16, sizeof(float) * 16);
	SIMD::mul(mvp, vp, transform.to_mat4());
	memcpy(mvp16, &mvp, sizeof(float) * 16);
}
