// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen; FidelityFX parts (c) 2021 Advanced Micro Devices, Inc.): see
// THIRD_PARTY_NOTICES.md at the repository root.
#include "math.hpp"

namespace Granite
{
mat4 inverse(const mat4 &m)
{
	// Cofactor expansion in double precision, rounded once to fp32.
	double a[16], inv[16];
	const float *src = m.data();
	for (int i = 0; i < 16; i++)
		a[i] = src[i];

	inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
	inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
	inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
	inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
	inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
	inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
	inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
	inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
	inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
	inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
	inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
	inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
	inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
	inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
	inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
	inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];

	double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
	double inv_det = 1.0 / det;
	mat4 r(0.0f);
	float *dst = r.data();
	for (int i = 0; i < 16; i++)
		dst[i] = float(inv[i] * inv_det);
	return r;
}

// muglm::inverse(mat4) (math/muglm/muglm.cpp:146-201) in fp32, operation for operation: for results that have to be the
// reference's bit for bit (a decal's world_to_texture, scene.cpp:733-736; inv_local_view_projection, render_context.cpp:67).  inverse()
// above works in double and differs from it in the last bits.
mat4 inverse_fp32(const mat4 &m)
{
	const float c00 = m[2][2] * m[3][3] - m[3][2] * m[2][3], c02 = m[1][2] * m[3][3] - m[3][2] * m[1][3], c03 = m[1][2] * m[2][3] - m[2][2] * m[1][3];
	const float c04 = m[2][1] * m[3][3] - m[3][1] * m[2][3], c06 = m[1][1] * m[3][3] - m[3][1] * m[1][3], c07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
	const float c08 = m[2][1] * m[3][2] - m[3][1] * m[2][2], c10 = m[1][1] * m[3][2] - m[3][1] * m[1][2], c11 = m[1][1] * m[2][2] - m[2][1] * m[1][2];
	const float c12 = m[2][0] * m[3][3] - m[3][0] * m[2][3], c14 = m[1][0] * m[3][3] - m[3][0] * m[1][3], c15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
	const float c16 = m[2][0] * m[3][2] - m[3][0] * m[2][2], c18 = m[1][0] * m[3][2] - m[3][0] * m[1][2], c19 = m[1][0] * m[2][2] - m[2][0] * m[1][2];
	const float c20 = m[2][0] * m[3][1] - m[3][0] * m[2][1], c22 = m[1][0] * m[3][1] - m[3][0] * m[1][1], c23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
	const float fac[6][4] = {{c00, c00, c02, c03}, {c04, c04, c06, c07}, {c08, c08, c10, c11}, {c12, c12, c14, c15}, {c16, c16, c18, c19}, {c20, c20, c22, c23}};
	float vec[4][4];
	for (int r = 0; r < 4; r++)
	{
		vec[r][0] = m[1][r];
		vec[r][1] = vec[r][2] = vec[r][3] = m[0][r];
	}
	mat4 inv(0.0f);
	for (int i = 0; i < 4; i++)
	{
		const float sign_a = (i & 1) ? -1.0f : 1.0f, sign_b = -sign_a;
		inv[0][i] = (vec[1][i] * fac[0][i] - vec[2][i] * fac[1][i] + vec[3][i] * fac[2][i]) * sign_a;
		inv[1][i] = (vec[0][i] * fac[0][i] - vec[2][i] * fac[3][i] + vec[3][i] * fac[4][i]) * sign_b;
		inv[2][i] = (vec[0][i] * fac[1][i] - vec[1][i] * fac[3][i] + vec[3][i] * fac[5][i]) * sign_a;
		inv[3][i] = (vec[0][i] * fac[2][i] - vec[1][i] * fac[4][i] + vec[2][i] * fac[5][i]) * sign_b;
	}
	const float d0 = m[0][0] * inv[0][0], d1 = m[0][1] * inv[1][0], d2 = m[0][2] * inv[2][0], d3 = m[0][3] * inv[3][0];
	const float one_over_determinant = 1.0f / ((d0 + d1) + (d2 + d3));
	for (int c = 0; c < 4; c++)
		inv[c] = inv[c] * one_over_determinant;
	return inv;
}

mat4 translate(const vec3 &v)
{
	mat4 m(1.0f);
	m[3] = vec4(v, 1.0f);
	return m;
}

mat4 scale(const vec3 &v)
{
	mat4 m(1.0f);
	m[0].x = v.x;
	m[1].y = v.y;
	m[2].z = v.z;
	return m;
}

mat4 perspective(float fovy, float aspect, float z_near, float z_far)
{
	float t = std::tan(fovy / 2.0f);
	mat4 r(0.0f);
	r[0][0] = 1.0f / (aspect * t);
	r[1][1] = 1.0f / t;
	r[2][2] = -1.0f - z_far / (z_near - z_far);
	r[3][2] = -(z_far * z_near) / (z_near - z_far);
	r[2][3] = -1.0f;
	for (int i = 0; i < 4; i++)
		r[i].y *= -1.0f;
	return r;
}

mat4 look_at(const vec3 &eye, const vec3 &center, const vec3 &up)
{
	vec3 f = normalize(center - eye);
	vec3 s = normalize(cross(f, up));
	vec3 u = cross(s, f);
	mat4 m(1.0f);
	m[0] = {s.x, u.x, -f.x, 0.0f};
	m[1] = {s.y, u.y, -f.y, 0.0f};
	m[2] = {s.z, u.z, -f.z, 0.0f};
	m[3] = {-dot(s, eye), -dot(u, eye), dot(f, eye), 1.0f};
	return m;
}

namespace
{
// muglm's forms: normalize multiplies by 1 / sqrt(dot), dot sums left to right
vec3 mu_normalize(const vec3 &v) { return v * (1.0f / std::sqrt(dot(v, v))); }
float mu_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

vec3 rotate(const quat &q, const vec3 &v)
{
	const vec3 quat_vector(q.x, q.y, q.z);
	const vec3 uv = cross(quat_vector, v);
	const vec3 uuv = cross(quat_vector, uv);
	return v + ((uv * q.w) + uuv) * 2.0f;
}

quat mul(const quat &p, const quat &q)
{
	return {p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z, p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y,
	        p.w * q.y + p.y * q.w + p.z * q.x - p.x * q.z, p.w * q.z + p.z * q.w + p.x * q.y - p.y * q.x};
}

quat rotate_vector(vec3 from, vec3 to)
{
	from = mu_normalize(from);
	to = mu_normalize(to);
	const float cos_angle = dot(from, to);
	if (std::fabs(cos_angle) > 0.9999f)
	{
		if (cos_angle > 0.9999f)
			return {1.0f, 0.0f, 0.0f, 0.0f};
		vec3 rotation = cross(vec3(1.0f, 0.0f, 0.0f), from);
		if (dot(rotation, rotation) > 0.001f)
			rotation = mu_normalize(rotation);
		else
			rotation = mu_normalize(cross(vec3(0.0f, 1.0f, 0.0f), from));
		return {0.0f, rotation};
	}
	const vec3 rotation = mu_normalize(cross(from, to));
	const vec3 half_vector = mu_normalize(from + to);
	const float cos_half_range = mu_clamp01(dot(half_vector, from));
	const float sin_half_angle = std::sqrt(1.0f - cos_half_range * cos_half_range);
	return {cos_half_range, rotation * sin_half_angle};
}

quat rotate_vector_axis(vec3 from, vec3 to, vec3 axis)
{
	axis = mu_normalize(axis);
	from = mu_normalize(cross(axis, from));
	to = mu_normalize(cross(axis, to));
	if (dot(to, from) < -0.9999f)
		return {0.0f, axis};
	const float d = dot(axis, cross(from, to));
	const float quat_sign = d < 0.0f ? -1.0f : (d > 0.0f ? 1.0f : 0.0f);
	const vec3 half_vector = mu_normalize(from + to);
	const float cos_half_range = mu_clamp01(dot(half_vector, from));
	const float sin_half_angle = quat_sign * std::sqrt(1.0f - cos_half_range * cos_half_range);
	return {cos_half_range, axis * sin_half_angle};
}
} // namespace

quat look_at(const vec3 &direction_, const vec3 &up)
{
	const vec3 z(0.0f, 0.0f, -1.0f), y(0.0f, 1.0f, 0.0f);
	const vec3 direction = mu_normalize(direction_);
	const vec3 right = cross(direction, up);
	const vec3 actual_up = cross(right, direction);
	const quat look_transform = rotate_vector(direction, z);
	const quat up_transform = rotate_vector_axis(rotate(look_transform, actual_up), y, z);
	return mul(up_transform, look_transform);
}

mat4 mat4_cast(const quat &q)
{
	mat4 res(1.0f);
	const float qxx = q.x * q.x, qyy = q.y * q.y, qzz = q.z * q.z, qxz = q.x * q.z, qxy = q.x * q.y, qyz = q.y * q.z;
	const float qwx = q.w * q.x, qwy = q.w * q.y, qwz = q.w * q.z;
	res[0][0] = 1.0f - 2.0f * (qyy + qzz);
	res[0][1] = 2.0f * (qxy + qwz);
	res[0][2] = 2.0f * (qxz - qwy);
	res[1][0] = 2.0f * (qxy - qwz);
	res[1][1] = 1.0f - 2.0f * (qxx + qzz);
	res[1][2] = 2.0f * (qyz + qwx);
	res[2][0] = 2.0f * (qxz + qwy);
	res[2][1] = 2.0f * (qyz - qwx);
	res[2][2] = 1.0f - 2.0f * (qxx + qyy);
	return res;
}

uint16_t floatToHalf(float v)
{
	uint32_t bits;
	memcpy(&bits, &v, sizeof(bits));
	const uint32_t sign = (bits >> 16) & 0x8000u;
	int exponent = int((bits >> 23) & 0xffu) - 112; // rebias 127 -> 15
	uint32_t mantissa = bits & 0x7fffffu;

	if (exponent >= 143) // source was inf / nan
	{
		if (mantissa == 0)
			return uint16_t(sign | 0x7c00u);
		mantissa >>= 13;
		return uint16_t(sign | 0x7c00u | mantissa | (mantissa == 0 ? 1u : 0u));
	}
	if (exponent <= 0)
	{
		if (exponent < -10)
			return uint16_t(sign);
		mantissa = (mantissa | 0x800000u) >> (1 - exponent);
		if (mantissa & 0x1000u)
			mantissa += 0x2000u; // ties (and everything above half) go up
		return uint16_t(sign | (mantissa >> 13));
	}
	if (mantissa & 0x1000u)
	{
		mantissa += 0x2000u;
		if (mantissa & 0x800000u)
		{
			mantissa = 0;
			exponent++;
		}
	}
	if (exponent > 30)
		return uint16_t(sign | 0x7c00u);
	return uint16_t(sign | (uint32_t(exponent) << 10) | (mantissa >> 13));
}
} // namespace Granite
