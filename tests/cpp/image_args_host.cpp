// granite_amd/csrc/image_args.hpp as a plain host program (tests/test_image_args_cpu.py builds it once plain and once with
// -fsanitize=address,undefined): the texel-size table against host/vk_subset.hpp, the 64-bit row cover, the alignment rule and the byte-range
// overlap.  Prints the table as one JSON line for the comparison with capi.FORMAT_BPP; exits 1 after naming every failed check.
#include <cstdio>
#include <cstring>
#include "../../granite_amd/csrc/image_args.hpp"
#include "../../granite_amd/csrc/host/vk_subset.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "image_args_host.cpp:%d: %s\n", __LINE__, #cond); failures++; } } while (0)

static bool broken(const char *rule, const char *word) { return rule && strstr(rule, word); }

int main()
{
	// every format number either header can name: uncompressed formats agree, block formats and unknown numbers have no texel size here
	printf("{");
	bool first = true;
	for (uint32_t f = 0; f < 256; f++)
	{
		const uint32_t texel = gr_format_texel_bytes(f);
		const bool block = f >= VK_FORMAT_BC1_RGB_UNORM_BLOCK && f <= VK_FORMAT_BC7_SRGB_BLOCK;
		EXPECT(texel == (block ? 0u : vk_format_block_size(VkFormat(f))));
		if (texel)
		{
			printf("%s\"%u\": %u", first ? "" : ", ", f, texel);
			first = false;
		}
	}
	printf("}\n");

	alignas(16) static unsigned char memory[4096];
	// a 16-texel pitch and a width that wraps in 32 bits: width * texel = pitch + 2^32 (or 2^33 for the 2-byte texel's 0x80000001)
	const struct { uint32_t format, width; } wraps[] = {{GR_FORMAT_R8G8B8A8_UNORM, 0x40000001u}, {GR_FORMAT_R16G16B16A16_SFLOAT, 0x20000001u},
	                                                    {GR_FORMAT_R8G8_UNORM, 0x80000001u}};
	for (const auto &w : wraps)
	{
		const uint32_t texel = gr_format_texel_bytes(w.format);
		gr_image img = {memory, 16, 8, 16 * texel, w.format};
		EXPECT(gr_image_rule(&img, w.format) == nullptr);
		img.width = w.width;
		EXPECT(uint32_t(img.width * texel) <= img.pitch_bytes); // the product the old checks formed
		EXPECT(broken(gr_image_rule(&img, w.format), "cover"));
		EXPECT(broken(gr_image_layout_rule(&img, w.format), "cover"));
		img.width = 16;
		img.pitch_bytes = 15 * texel;
		EXPECT(broken(gr_image_rule(&img, w.format), "cover"));
		// alignment: exactly the texel size passes, one byte off does not, for the pitch and for the pointer
		img.pitch_bytes = 17 * texel;
		img.ptr = memory + texel;
		EXPECT(gr_image_rule(&img, w.format) == nullptr);
		img.ptr = memory + texel + 1;
		EXPECT(broken(gr_image_rule(&img, w.format), "multiple"));
		img.ptr = memory;
		img.pitch_bytes = 16 * texel + 1;
		EXPECT(broken(gr_image_rule(&img, w.format), "multiple"));
		EXPECT(gr_image_layout_rule(&img, w.format) == nullptr); // the byte-addressed launchers take it
	}
	{
		// the order of the rules, and the optional extent and second format
		gr_image img = {memory, 16, 8, 64, GR_FORMAT_R8G8B8A8_SRGB};
		EXPECT(broken(gr_image_rule(nullptr, GR_RGBA8_FORMATS), "null"));
		EXPECT(gr_image_rule(&img, GR_RGBA8_FORMATS) == nullptr && gr_image_rule(&img, GR_RGBA8_FORMATS, 16, 8) == nullptr);
		EXPECT(broken(gr_image_rule(&img, GR_FORMAT_R8G8B8A8_UNORM), "format") && broken(gr_image_rule(&img, GR_HDR_FORMATS), "format"));
		EXPECT(broken(gr_image_rule(&img, GR_RGBA8_FORMATS, 16, 9), "width and height") && broken(gr_image_rule(&img, GR_RGBA8_FORMATS, 8, 8), "width and height"));
		img.format = GR_FORMAT_BC7_UNORM_BLOCK;
		EXPECT(broken(gr_image_rule(&img, GR_FORMAT_BC7_UNORM_BLOCK), "format")); // no texel size: never a valid image
		img.format = GR_FORMAT_R8G8B8A8_SRGB;
		img.width = 0;
		EXPECT(broken(gr_image_rule(&img, GR_RGBA8_FORMATS), "no texels"));
		img.ptr = nullptr;
		EXPECT(broken(gr_image_rule(&img, GR_FORMAT_R8_UNORM), "->ptr")); // the pointer is asked before the format
	}
	{
		const gr_image a = {memory, 16, 8, 64, GR_FORMAT_R8G8B8A8_UNORM}; // [0, 512)
		gr_image b = a;
		b.ptr = memory + 512; // adjacent
		EXPECT(!gr_images_overlap(&a, &b) && !gr_images_overlap(&b, &a));
		b.ptr = memory + 511; // one byte shared
		EXPECT(gr_images_overlap(&a, &b) && gr_images_overlap(&b, &a));
		b.ptr = memory + 64; // one row in
		EXPECT(gr_images_overlap(&a, &b));
		b.height = 2; // inside
		EXPECT(gr_images_overlap(&a, &b) && gr_images_overlap(&b, &a));
		b.height = 0; // no rows: no bytes
		EXPECT(!gr_images_overlap(&a, &b) && !gr_images_overlap(&b, &a));
		EXPECT(gr_images_overlap(&a, &a));
		EXPECT(gr_images_overlap(memory, 8, memory + 7, 1) && !gr_images_overlap(memory, 8, memory + 8, 8) && !gr_images_overlap(memory + 4, 0, memory, 8));
	}
	return failures ? 1 : 0;
}
