// What every launcher of the C ABI asks of a gr_image argument, stated once.  Host-only and free of HIP: a plain C++ program compiles it
// (tests/cpp/image_args_host.cpp).  Limits that belong to one kernel -- 16-byte alignment for a wide path, a largest extent, 32-bit
// offsets -- stay at that kernel's entry point.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/granite_hip.h"

// Bytes of one texel: the only format-to-size table of the kernel library.  0 for block-compressed and unknown formats.
static inline uint32_t gr_format_texel_bytes(uint32_t format)
{
	switch (format)
	{
	case GR_FORMAT_R8_UNORM: return 1;
	case GR_FORMAT_R8G8_UNORM:
	case GR_FORMAT_R16_UNORM:
	case GR_FORMAT_R16_SFLOAT:
	case GR_FORMAT_D16_UNORM: return 2;
	case GR_FORMAT_R8G8B8A8_UNORM:
	case GR_FORMAT_R8G8B8A8_SRGB:
	case GR_FORMAT_B8G8R8A8_UNORM:
	case GR_FORMAT_B8G8R8A8_SRGB:
	case GR_FORMAT_A2B10G10R10_UNORM_PACK32:
	case GR_FORMAT_R16G16_UNORM:
	case GR_FORMAT_R16G16_SFLOAT:
	case GR_FORMAT_R32_SFLOAT:
	case GR_FORMAT_B10G11R11_UFLOAT_PACK32:
	case GR_FORMAT_D32_SFLOAT: return 4;
	case GR_FORMAT_R16G16B16A16_SFLOAT:
	case GR_FORMAT_R32G32_SFLOAT: return 8;
	default: return 0;
	}
}

// The format an argument must have, or one of up to three.
struct gr_format_set
{
	uint32_t a, b, c;
	constexpr gr_format_set(uint32_t first, uint32_t second = GR_FORMAT_UNDEFINED, uint32_t third = GR_FORMAT_UNDEFINED) : a(first), b(second), c(third) {}
};
constexpr gr_format_set GR_RGBA8_FORMATS{GR_FORMAT_R8G8B8A8_UNORM, GR_FORMAT_R8G8B8A8_SRGB};
// an HDR colour target as the passes that only read it take it: RGBA16F, or the reference's default B10G11R11_UFLOAT_PACK32
constexpr gr_format_set GR_HDR_FORMATS{GR_FORMAT_R16G16B16A16_SFLOAT, GR_FORMAT_B10G11R11_UFLOAT_PACK32};

// The rule of the contract that `img` breaks, worded to follow the argument's name in a message ("out" + " pitch_bytes does not ..."), or
// nullptr.  Asked in this order: the image and its pointer are not null; the format is (one of) `formats`; the extent is non-zero and,
// where `width` and `height` are given, equals them; a row fits the pitch, the product taken in 64 bits; pitch_bytes and the pointer are
// multiples of the texel size.  gr_image_layout_rule is the part in the middle, format to row cover: what a plan query asks of a
// description whose ptr is not set yet, and all that the two launchers ask whose kernels address single bytes and take an image at any
// alignment (video.hip, texture_decode.hip).
static inline const char *gr_image_layout_rule(const gr_image *img, gr_format_set formats, uint32_t width = 0, uint32_t height = 0)
{
	const uint32_t texel = gr_format_texel_bytes(img->format);
	if ((img->format != formats.a && img->format != formats.b && img->format != formats.c) || texel == 0) // (GR_FORMAT_UNDEFINED has no texel size)
		return " has a format this argument does not take";
	if (img->width == 0 || img->height == 0)
		return " has no texels (width or height is 0)";
	if ((width && img->width != width) || (height && img->height != height))
		return " does not have the width and height this call works on";
	if (uint64_t(img->width) * texel > img->pitch_bytes)
		return " pitch_bytes does not cover a row of width texels";
	return nullptr;
}
static inline const char *gr_image_rule(const gr_image *img, gr_format_set formats, uint32_t width = 0, uint32_t height = 0)
{
	if (!img)
		return " is a null pointer";
	if (!img->ptr)
		return "->ptr is a null pointer";
	if (const char *rule = gr_image_layout_rule(img, formats, width, height))
		return rule;
	const uint32_t texel = gr_format_texel_bytes(img->format);
	if (img->pitch_bytes % texel || reinterpret_cast<uintptr_t>(img->ptr) % texel)
		return " pitch_bytes or ptr is not a multiple of the texel size";
	return nullptr;
}

// A limit of single launchers (lighting.hip, aa.hip), asked after gr_image_rule: their kernels form `y * pitch_bytes + x * texel` in 32 bits, so
// the image's last byte has to lie within 4 GiB of ptr.  An attachment viewed out of a larger allocation counts with the pitch it is viewed at.
static inline const char *gr_image_offset_rule(const gr_image *img)
{
	return uint64_t(img->pitch_bytes) * img->height > 0xffffffffull ? " pitch_bytes * height is above 4 GiB - 1: this launcher's kernels form byte offsets in 32 bits" : nullptr;
}

// Two byte ranges share at least one byte.  An empty range shares none.
static inline bool gr_images_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
	const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
	return a_bytes && b_bytes && pa < pb + b_bytes && pb < pa + a_bytes;
}
// [ptr, ptr + pitch_bytes * height) of both images: lanes read texels that other lanes of the same launch write when an output shares bytes
// with an input.
static inline bool gr_images_overlap(const gr_image *a, const gr_image *b)
{
	return gr_images_overlap(a->ptr, size_t(a->pitch_bytes) * a->height, b->ptr, size_t(b->pitch_bytes) * b->height);
}
