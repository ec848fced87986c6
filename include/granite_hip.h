/* granite_hip.h — C ABI of the MI355X (gfx950) executor for Granite's image-space chain.
 *
 * Granite has no C plugin ABI: its operator interface for this path is the C++ RenderGraph pass API
 * (renderer/render_graph.hpp:488-716,779-893) whose callbacks record GLSL dispatches / full-screen quads on a
 * Vulkan::CommandBuffer.  This header is what a HIP backend for those callbacks binds instead: one entry point per
 * shader dispatch on the hot path, taking plain pointers + sizes (no C++/torch types), with push-constant structs that
 * are byte-identical to the reference's.  Each entry point cites the reference call site it replaces.
 *
 * Conventions
 *   - All image/buffer pointers are DEVICE pointers into linear, row-major HBM buffers (origin top-left).
 *   - Every launcher is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *   - Return value: 0 on success, negative gr_status on failure; gr_last_error() holds the message.
 *     No exceptions cross this boundary.  Thread-safe per (ctx, stream).
 */
#ifndef GRANITE_HIP_H_
#define GRANITE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_ABI_VERSION 1

typedef struct gr_ctx gr_ctx;
typedef void *gr_stream; /* hipStream_t */

typedef enum gr_status
{
	GR_OK = 0,
	GR_ERR_INVALID_ARGUMENT = -1,
	GR_ERR_HIP = -2,
	GR_ERR_UNSUPPORTED_FORMAT = -3,
	GR_ERR_OUT_OF_MEMORY = -4
} gr_status;

/* Subset of VkFormat used on the path; numeric values are VkFormat's so reference call sites read the same. */
typedef enum gr_format
{
	GR_FORMAT_UNDEFINED = 0,
	GR_FORMAT_R8_UNORM = 9,
	GR_FORMAT_R8G8_UNORM = 16,
	GR_FORMAT_R8G8B8A8_UNORM = 37,
	GR_FORMAT_R8G8B8A8_SRGB = 43,
	GR_FORMAT_B8G8R8A8_UNORM = 44,     /* video output plane (gr_video_scale) */
	GR_FORMAT_B8G8R8A8_SRGB = 50,      /* video output plane (gr_video_scale) */
	GR_FORMAT_A2B10G10R10_UNORM_PACK32 = 64,
	GR_FORMAT_R16_UNORM = 70,          /* P010 / P016 / 16-bit YUV planes (gr_video_scale) */
	GR_FORMAT_R16_SFLOAT = 76,
	GR_FORMAT_R16G16_UNORM = 77,       /* P010 / P016 interleaved chroma (gr_video_scale) */
	GR_FORMAT_R16G16_SFLOAT = 83,
	GR_FORMAT_R16G16B16A16_SFLOAT = 97,
	GR_FORMAT_R32_SFLOAT = 100,
	GR_FORMAT_R32G32_SFLOAT = 103,     /* complex fp32 output of gr_fft_execute */
	GR_FORMAT_B10G11R11_UFLOAT_PACK32 = 122, /* HDR targets with renderTargetFp16 = false (scene_viewer_application.cpp:881-883), TAA colour (temporal.cpp:211-213) */
	GR_FORMAT_D16_UNORM = 124,
	GR_FORMAT_D32_SFLOAT = 126,
	/* Block-compressed inputs of gr_texture_decode (BC4 / BC5 UNORM are also what gr_texture_encode writes); no other entry point takes
	 * them.  140 and 142 (BC4 / BC5 SNORM) are absent. */
	GR_FORMAT_BC1_RGB_UNORM_BLOCK = 131,
	GR_FORMAT_BC1_RGB_SRGB_BLOCK = 132,
	GR_FORMAT_BC1_RGBA_UNORM_BLOCK = 133,
	GR_FORMAT_BC1_RGBA_SRGB_BLOCK = 134,
	GR_FORMAT_BC2_UNORM_BLOCK = 135,
	GR_FORMAT_BC2_SRGB_BLOCK = 136,
	GR_FORMAT_BC3_UNORM_BLOCK = 137,
	GR_FORMAT_BC3_SRGB_BLOCK = 138,
	GR_FORMAT_BC4_UNORM_BLOCK = 139,
	GR_FORMAT_BC5_UNORM_BLOCK = 141,
	GR_FORMAT_BC6H_UFLOAT_BLOCK = 143,
	GR_FORMAT_BC6H_SFLOAT_BLOCK = 144,
	GR_FORMAT_BC7_UNORM_BLOCK = 145,
	GR_FORMAT_BC7_SRGB_BLOCK = 146,
	/* ASTC LDR, 2-D footprints, 16 bytes a block: inputs of gr_texture_decode only.  The SFLOAT (HDR) forms are absent. */
	GR_FORMAT_ASTC_4x4_UNORM_BLOCK = 157,
	GR_FORMAT_ASTC_4x4_SRGB_BLOCK = 158,
	GR_FORMAT_ASTC_5x4_UNORM_BLOCK = 159,
	GR_FORMAT_ASTC_5x4_SRGB_BLOCK = 160,
	GR_FORMAT_ASTC_5x5_UNORM_BLOCK = 161,
	GR_FORMAT_ASTC_5x5_SRGB_BLOCK = 162,
	GR_FORMAT_ASTC_6x5_UNORM_BLOCK = 163,
	GR_FORMAT_ASTC_6x5_SRGB_BLOCK = 164,
	GR_FORMAT_ASTC_6x6_UNORM_BLOCK = 165,
	GR_FORMAT_ASTC_6x6_SRGB_BLOCK = 166,
	GR_FORMAT_ASTC_8x5_UNORM_BLOCK = 167,
	GR_FORMAT_ASTC_8x5_SRGB_BLOCK = 168,
	GR_FORMAT_ASTC_8x6_UNORM_BLOCK = 169,
	GR_FORMAT_ASTC_8x6_SRGB_BLOCK = 170,
	GR_FORMAT_ASTC_8x8_UNORM_BLOCK = 171,
	GR_FORMAT_ASTC_8x8_SRGB_BLOCK = 172,
	GR_FORMAT_ASTC_10x5_UNORM_BLOCK = 173,
	GR_FORMAT_ASTC_10x5_SRGB_BLOCK = 174,
	GR_FORMAT_ASTC_10x6_UNORM_BLOCK = 175,
	GR_FORMAT_ASTC_10x6_SRGB_BLOCK = 176,
	GR_FORMAT_ASTC_10x8_UNORM_BLOCK = 177,
	GR_FORMAT_ASTC_10x8_SRGB_BLOCK = 178,
	GR_FORMAT_ASTC_10x10_UNORM_BLOCK = 179,
	GR_FORMAT_ASTC_10x10_SRGB_BLOCK = 180,
	GR_FORMAT_ASTC_12x10_UNORM_BLOCK = 181,
	GR_FORMAT_ASTC_12x10_SRGB_BLOCK = 182,
	GR_FORMAT_ASTC_12x12_UNORM_BLOCK = 183,
	GR_FORMAT_ASTC_12x12_SRGB_BLOCK = 184
} gr_format;

/* A 2-D attachment as the executor sees it: what Vulkan::ImageView is to the reference's callbacks.
 * Every launcher asks the same of an image argument (granite_amd/csrc/image_args.hpp) before anything is launched: the image and its ptr
 * are not NULL; the format is one the argument takes; width and height are not 0 and match the call's other images where they must;
 * width * texel size <= pitch_bytes (in 64 bits); pitch_bytes and ptr are multiples of the texel size (gr_video_scale, gr_video_yuv_to_rgb
 * and gr_texture_decode address bytes and take any alignment).  A broken rule is GR_ERR_INVALID_ARGUMENT, with the argument and the rule in
 * gr_last_error(); a wrong format alone is GR_ERR_UNSUPPORTED_FORMAT from gr_tonemap, gr_fft_execute, gr_env_equirect_to_cube and
 * gr_texture_decode.  Where an entry point refuses an output that is its input, it refuses any shared byte of [ptr, ptr + pitch_bytes *
 * height).  Limits of a single kernel (a largest extent, 16-byte alignment for a faster path) are documented at its entry point.
 * A pitch wider than the row and a pointer into a larger allocation are taken by every launcher (rows padded to 256 bytes, views
 * into an atlas); where a kernel's form is chosen by alignment they may select the slower one (tests/test_gpu_image_layouts.py holds every
 * form to the same reference).  gr_lighting, gr_blit
 * and the anti-aliasing launchers (FXAA, SMAA, TAA) form byte offsets in 32 bits and refuse, in the same way, an image argument with
 * pitch_bytes * height above 2^32 - 1; the other launchers form them in 64 bits and have no such limit. */
typedef struct gr_image
{
	void *ptr;            /* device pointer */
	uint32_t width;
	uint32_t height;
	uint32_t pitch_bytes; /* row pitch; rows are tightly packed unless stated */
	uint32_t format;      /* gr_format */
} gr_image;

/* ---- context ----------------------------------------------------------------------------------------------------- */
gr_ctx *gr_create(int device);          /* replaces Vulkan::Context/Device creation for this path */
void gr_destroy(gr_ctx *ctx);
const char *gr_last_error(gr_ctx *ctx);
int gr_abi_version(void);
int gr_sync(gr_ctx *ctx, gr_stream stream); /* hipStreamSynchronize; Device::wait_idle analogue */

/* Physical-resource allocation used by RenderGraph::setup_physical_{image,buffer} (render_graph.cpp:2577-2684).
 * Memory is zero-initialised like the reference's (render_graph.cpp:2586-2587). */
int gr_alloc(gr_ctx *ctx, size_t bytes, void **dptr);
int gr_free(gr_ctx *ctx, void *dptr);
int gr_upload(gr_ctx *ctx, gr_stream stream, void *dst, const void *src_host, size_t bytes);   /* cmd.update_buffer */
int gr_download(gr_ctx *ctx, gr_stream stream, void *dst_host, const void *src, size_t bytes); /* readback */
/* Several cmd.update_buffer calls of one pass (clusterer.cpp:1178-1207,1302) as ONE kernel that reads pinned host memory
 * (hipHostMalloc'd, device-mapped) and writes HBM: no copy engine, no cross-engine signalling, ordered like any other
 * kernel on `stream`.  Sizes and offsets must be multiples of 4 bytes; at most GR_MAX_UPLOAD_RANGES ranges. */
#define GR_MAX_UPLOAD_RANGES 8
typedef struct gr_upload_range
{
	void *dst;             /* device */
	const void *src_pinned; /* pinned host */
	size_t bytes;
} gr_upload_range;
int gr_upload_batch(gr_ctx *ctx, gr_stream stream, const gr_upload_range *ranges, uint32_t count);
/* Pinned, device-mapped host memory for gr_upload_batch sources (hipHostMalloc / hipHostFree). */
int gr_alloc_host(gr_ctx *ctx, size_t bytes, void **hptr);
int gr_free_host(gr_ctx *ctx, void *hptr);
int gr_copy(gr_ctx *ctx, gr_stream stream, void *dst, const void *src, size_t bytes);
int gr_fill_zero(gr_ctx *ctx, gr_stream stream, void *dst, size_t bytes);
int gr_fill_byte(gr_ctx *ctx, gr_stream stream, void *dst, int value, size_t bytes); /* clear to a UNORM8 constant */

/* Host-only: the linear -> sRGB8 staircase table the *_SRGB stores use (count must be 1665 {threshold bits, byte} pairs;
 * csrc/device_common.hpp).  Exposed so that the table can be checked against the transfer function without a GPU. */
int gr_srgb_encode_table(uint32_t *entries_xy, uint32_t count);
/* Host-only: the exposed colour -> tonemapped sRGB8 staircase of gr_tonemap's *_SRGB path (1025 pairs). */
int gr_tonemap_srgb8_table(uint32_t *entries_xy, uint32_t count);

/* Measured HBM ceiling for the roofline ("a hipMemcpyDtoD / stream-triad probe on the box, in the same
 * run"): a float4 copy b = a and a triad a = b + s * c over `bytes`-sized arrays that do not fit the 256 MiB Infinity
 * Cache, best of `repeats` launches timed with hipEvents.  GB/s counts bytes read + written (copy 2 x, triad 3 x bytes). */
int gr_bandwidth_probe(gr_ctx *ctx, size_t bytes, int repeats, double *copy_GBps, double *triad_GBps);

/* Per-kernel GPU timing (RenderGraph::enable_timestamps analogue, render_graph.cpp:2196-2310): when enabled, every
 * launcher brackets its kernel with hipEvents on the launch stream; gr_timing_query drains {name, count, total_ms}. */
typedef struct gr_timing_entry
{
	const char *name;
	uint64_t count;
	double total_ms;
} gr_timing_entry;
int gr_timing_enable(gr_ctx *ctx, int enable);
/* Restrict bracketing to launchers whose name equals `name` (NULL = all): keeps event overhead out of a timed loop. */
int gr_timing_set_filter(gr_ctx *ctx, const char *name);
/* 1 when a launch of the kernel timed under `name` would currently get a hipEvent bracket (timing enabled and the filter, if any,
 * names it): a pre-recorded launch sequence containing it must be launched directly instead. */
int gr_timing_brackets(gr_ctx *ctx, const char *name);
/* Bracket only every n-th matching launch (1 = all).  An event pair around a kernel keeps the command processor from
 * overlapping that launch with its neighbours on the stream; sampling keeps a timed loop close to its unbracketed speed
 * while the launch duration is still measured live inside it. */
int gr_timing_set_sampling(gr_ctx *ctx, uint32_t every_nth);
/* Restrict bracketing to several launchers: gr_timing_set_filter also takes a comma-separated list ("lighting,output_gather").
 * gr_timing_span_begin / _end bracket work that is not one of this library's launches (a collective on its stream) under the caller's
 * name, into the same accumulator; *span is NULL when the name is not being timed (then _end is a no-op).  gr_timing_max_ms: the
 * longest single bracket under a name since the last reset. */
int gr_timing_span_begin(gr_ctx *ctx, gr_stream stream, const char *name, void **span);
int gr_timing_span_end(gr_ctx *ctx, gr_stream stream, void *span);
int gr_timing_max_ms(gr_ctx *ctx, const char *name, double *max_ms);
int gr_timing_reset(gr_ctx *ctx);
int gr_timing_query(gr_ctx *ctx, gr_timing_entry *entries, int max_entries); /* returns number of entries; syncs */

/* Render area of one launch: output rows [first, first + count) only.  A NULL pointer = the whole image; count == 0 = no rows
 * (the launcher returns GR_OK without launching: a rank whose band is empty must not touch the image).  The one embedded use,
 * gr_lighting_args.rows, keeps {0, 0} = whole image, as a zero-initialised argument struct has it.
 * The reference restricts draws with VkRect2D render areas / scissors (vulkan/command_buffer.cpp set_scissor); the
 * executor uses row bands to tile one frame across GPUs.  Coordinates stay those of the full image, so a
 * band computes bit-identical values to the same rows of a whole-image launch. */
typedef struct gr_rows
{
	uint32_t first;
	uint32_t count;
} gr_rows;

/* ---- HDR post chain (renderer/post/hdr.cpp) ---------------------------------------------------------------------- */

/* LuminanceData, 12 B (assets/shaders/post/luminance.comp:4-9): {log2 avg, avg, 1/avg}. */
typedef struct gr_luminance_data
{
	float average_log_luminance;
	float average_linear_luminance;
	float average_inv_linear_luminance;
} gr_luminance_data;

/* bloom_threshold_build_compute (hdr.cpp:115-144) + bloom_threshold.comp.  lum = device LuminanceData or NULL
 * (DYNAMIC_EXPOSURE=0).  hdr, out: R16G16B16A16_SFLOAT. */
typedef struct gr_push_bloom_threshold
{
	uint32_t threads[2];
	float inv_output_size[2];
} gr_push_bloom_threshold;
int gr_bloom_threshold(gr_ctx *ctx, gr_stream stream, const gr_image *hdr, const gr_image *out,
                       const gr_luminance_data *lum, const gr_push_bloom_threshold *push);
int gr_bloom_threshold_rows(gr_ctx *ctx, gr_stream stream, const gr_image *hdr, const gr_image *out,
                            const gr_luminance_data *lum, const gr_push_bloom_threshold *push, const gr_rows *rows);

/* bloom_downsample_build_compute (hdr.cpp:146-187) + bloom_downsample.comp.  history = previous frame's output
 * (FEEDBACK=1, NearestClamp) or NULL. */
typedef struct gr_push_bloom_downsample
{
	uint32_t threads[2];
	float inv_output_size[2];
	float inv_input_size[2];
	float lerp;
} gr_push_bloom_downsample;
int gr_bloom_downsample(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out,
                        const gr_image *history, const gr_push_bloom_downsample *push);
int gr_bloom_downsample_rows(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out,
                             const gr_image *history, const gr_push_bloom_downsample *push, const gr_rows *rows);

/* bloom_upsample_build_compute (hdr.cpp:189-216) + bloom_upsample.comp. */
typedef struct gr_push_bloom_upsample
{
	uint32_t threads[2];
	float inv_output_size[2];
	float inv_input_size[2];
} gr_push_bloom_upsample;
int gr_bloom_upsample(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out,
                      const gr_push_bloom_upsample *push);
int gr_bloom_upsample_rows(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out,
                           const gr_push_bloom_upsample *push, const gr_rows *rows);

/* luminance_build_compute (hdr.cpp:68-98) + luminance.comp: mean log-luminance of `in`.a over a size.x x size.y
 * bilinear grid, clamp, temporal lerp, read-modify-write of *lum. */
typedef struct gr_push_luminance
{
	uint32_t size[2];
	float lerp;
	float min_loglum;
	float max_loglum;
} gr_push_luminance;
int gr_luminance(gr_ctx *ctx, gr_stream stream, const gr_image *in, gr_luminance_data *lum,
                 const gr_push_luminance *push);

/* The coarse end of the pyramid as recorded by hdr.cpp:364-377 -- downsample-2, downsample-3 (+ feedback), luminance,
 * upsample-2, upsample-1 -- in two launches instead of five: every texel is computed by the same code as the separate entry
 * points above (values and fp16 roundings between levels are identical), the intermediate levels are still written.
 * gr_bloom_tail_supported() says whether a pyramid qualifies (whole levels, each level ceil(half) of the one above as
 * render_graph.cpp's InputRelative sizes are: 4K, 1080p, odd sizes alike); otherwise the five separate calls are the path. */
int gr_bloom_tail_supported(const gr_image *d1, const gr_image *d2, const gr_image *d3, const gr_image *u2, const gr_image *u1,
                            const gr_push_bloom_downsample *push_d2, const gr_push_bloom_downsample *push_d3,
                            const gr_push_bloom_upsample *push_u2, const gr_push_bloom_upsample *push_u1);
int gr_bloom_down_tail(gr_ctx *ctx, gr_stream stream, const gr_image *d1, const gr_image *d2, const gr_image *d3,
                       const gr_image *history, const gr_push_bloom_downsample *push_d2,
                       const gr_push_bloom_downsample *push_d3);
/* downsample-0 and downsample-1 (hdr.cpp:358-362) in one launch, the same way: a workgroup makes an 8 x 8 tile of downsample-1 from
 * the patch of downsample-0 under its taps, which it first makes from the threshold level and stores.  rows_d1 restricts
 * downsample-1 (row bands; downsample-0 is written under those rows' taps).  Values in both levels are those of two
 * gr_bloom_downsample calls, byte for byte.  gr_bloom_down_mid_supported(): whole levels whose patch fits (any pyramid of
 * InputRelative sizes) and a downsample-1 of at most 65536 texels -- frames up to 1440p, where the chain of dependent launches sets
 * the pace; above, the recomputed overlap costs more than the launch it saves (measured at 4K). */
int gr_bloom_down_mid_supported(const gr_image *threshold, const gr_image *d0, const gr_image *d1, const gr_push_bloom_downsample *push_d0,
                                const gr_push_bloom_downsample *push_d1);
int gr_bloom_down_mid(gr_ctx *ctx, gr_stream stream, const gr_image *threshold, const gr_image *d0, const gr_image *d1,
                      const gr_push_bloom_downsample *push_d0, const gr_push_bloom_downsample *push_d1, const gr_rows *rows_d1);
/* The threshold dispatch with downsample-0 and downsample-1 (hdr.cpp:354-362) in one launch: a workgroup makes an 8 x 8 tile of
 * downsample-1, under it the patch of downsample-0, under that the patch of the threshold level from the HDR target, every texel by the
 * code of the separate entry points (all three levels are written, byte for byte what gr_bloom_threshold + gr_bloom_down_mid leave).
 * gr_bloom_down_head_supported(): what gr_bloom_down_mid_supported() asks for, and every level exactly half of its input (the 2:1 forms
 * of gr_bloom_threshold and gr_bloom_downsample).  lum NULL: no dynamic exposure.  Whole images (row bands use the separate calls). */
int gr_bloom_down_head_supported(const gr_image *hdr, const gr_image *threshold, const gr_image *d0, const gr_image *d1,
                                 const gr_push_bloom_threshold *push_t, const gr_push_bloom_downsample *push_d0,
                                 const gr_push_bloom_downsample *push_d1);
int gr_bloom_down_head(gr_ctx *ctx, gr_stream stream, const gr_image *hdr, const gr_image *threshold, const gr_image *d0, const gr_image *d1,
                       const gr_luminance_data *lum, const gr_push_bloom_threshold *push_t, const gr_push_bloom_downsample *push_d0,
                       const gr_push_bloom_downsample *push_d1);
/* lum / push_lum both NULL: no dynamic exposure, no luminance reduction. */
int gr_bloom_up_tail(gr_ctx *ctx, gr_stream stream, const gr_image *d3, const gr_image *u2, const gr_image *u1,
                     gr_luminance_data *lum, const gr_push_bloom_upsample *push_u2, const gr_push_bloom_upsample *push_u1,
                     const gr_push_luminance *push_lum);

/* The whole upsample chain -- luminance, upsample-2, upsample-1, upsample-0 (hdr.cpp:368-379) -- in one launch: a workgroup makes a 32 x 32
 * tile of upsample-0 from the patch of upsample-1 under it, that from the patch of upsample-2, that from downsample-3; all three levels are
 * written, byte for byte what gr_bloom_up_tail + gr_bloom_upsample leave.  gr_bloom_up_all_supported(): whole levels of a pyramid of
 * InputRelative sizes, upsample-0 exactly twice upsample-1 and at most 960 x 540 (a 4K frame: above, the tiles' recomputed patches cost more than the launch saved).  lum / push_lum both NULL: no
 * dynamic exposure, no luminance reduction. */
int gr_bloom_up_all_supported(const gr_image *d3, const gr_image *u2, const gr_image *u1, const gr_image *u0, const gr_push_bloom_upsample *push_u2,
                              const gr_push_bloom_upsample *push_u1, const gr_push_bloom_upsample *push_u0);
/* flags: GR_BLOOM_BUSY_FRAME_BIT -- scheduling hint, no effect on any value: the rest of the frame's back (a temporal resolve, SMAA) fills the
 * machine beside the lighting launch.  The launch then runs 256-thread workgroups (one wave per SIMD: a workgroup starts wherever one lighting
 * workgroup has retired) instead of 1024-thread ones (which wait for four retirements on one CU and so end up in the idle time between two lighting
 * launches: best for a frame whose back is short).  Measured (profiles/r06_back_chain_beside_lighting.txt): the launch inside the 4K frame 23
 * against 64-68 us; the TAA + SMAA frame 0.548 against 0.558-0.573 ms, the lighting + bloom + tonemap frame 0.204 against 0.199 ms. */
#define GR_BLOOM_BUSY_FRAME_BIT 1u
int gr_bloom_up_all(gr_ctx *ctx, gr_stream stream, const gr_image *d3, const gr_image *u2, const gr_image *u1, const gr_image *u0,
                    gr_luminance_data *lum, const gr_push_bloom_upsample *push_u2, const gr_push_bloom_upsample *push_u1,
                    const gr_push_bloom_upsample *push_u0, const gr_push_luminance *push_lum, uint32_t flags);

/* The WHOLE bloom pass of a small frame -- every dispatch of bloom_build_compute (hdr.cpp:354-379): threshold, downsample-0 .. -3 (+ feedback),
 * luminance, upsample-2 .. -0 -- in ONE launch: the work of gr_bloom_down_head, gr_bloom_down_tail and gr_bloom_up_all as three block ranges of one
 * grid, a range starting when the one before it has published its levels (device-side counters in the context; workgroups wait for lower
 * workgroup ids only).  Every level is written, byte for byte what the separate launches leave.  gr_bloom_pyramid_supported(): what the three
 * launches require (whole levels of a pyramid of InputRelative sizes, threshold / downsample-0 / -1 exactly half of their inputs, upsample-0
 * exactly twice upsample-1, a feedback history) and a frame of at most 640 x 384 pixels -- where the host's runtime calls, not the device, set
 * the frame's pace; above, the device-side hand-overs between the ranges cost more than the launches they replace (gr_bloom_pyramid itself
 * accepts any size the three launches accept).  lum NULL: static exposure, no luminance reduction.  Launches of this entry point on one context must not
 * overlap in time (issue them on one stream, as the executor does); gr_debug_pyramid_giveups() synchronises the device and returns how many
 * workgroups ever gave up waiting for a predecessor (0 unless that rule was broken). */
typedef struct gr_bloom_pyramid_args
{
	gr_image hdr, threshold, d0, d1, d2, d3, history, u2, u1, u0;
	gr_luminance_data *lum;
	gr_push_bloom_threshold push_threshold;
	gr_push_bloom_downsample push_d0, push_d1, push_d2, push_d3;
	gr_push_bloom_upsample push_u2, push_u1, push_u0;
	gr_push_luminance push_luminance;
} gr_bloom_pyramid_args;
int gr_bloom_pyramid_supported(const gr_bloom_pyramid_args *args);
int gr_bloom_pyramid(gr_ctx *ctx, gr_stream stream, const gr_bloom_pyramid_args *args);
int gr_debug_pyramid_giveups(gr_ctx *ctx, uint32_t *count);

/* tonemap_build_render_pass (hdr.cpp:283-306) + tonemap.frag (full-screen quad).  out: R8G8B8A8_SRGB (linear value
 * is sRGB-encoded on store, as the attachment hardware does) or R8G8B8A8_UNORM.  lum NULL => DYNAMIC_EXPOSURE=0. */
typedef struct gr_push_tonemap
{
	float dynamic_exposure;
} gr_push_tonemap;
int gr_tonemap(gr_ctx *ctx, gr_stream stream, const gr_image *hdr, const gr_image *bloom, const gr_image *out,
               const gr_luminance_data *lum, const gr_push_tonemap *push);
int gr_tonemap_rows(gr_ctx *ctx, gr_stream stream, const gr_image *hdr, const gr_image *bloom, const gr_image *out,
                    const gr_luminance_data *lum, const gr_push_tonemap *push, const gr_rows *rows);

/* ---- clustered lighting (renderer/lights/clusterer.cpp, renderer/renderer.cpp) ------------------------------------- */

/* PositionalFragmentInfo (renderer/lights/light_info.hpp:35-44), 48 B. */
typedef struct gr_light_info
{
	float color[3];
	uint32_t spot_scale_bias; /* 2 x fp16: scale | bias << 16 */
	float position[3];
	uint32_t offset_radius;   /* 2 x fp16: offset | radius << 16 */
	float direction[3];
	float inv_radius;
} gr_light_info;

/* mat_affine (math/muglm/muglm.hpp:899-958): 3 rows of vec4. */
typedef struct gr_mat_affine
{
	float rows[3][4];
} gr_mat_affine;

/* ClustererParametersBindless, std140, 176 B (assets/shaders/lights/clusterer_data.h:20-39; math/render_parameters.hpp:90-108). */
typedef struct gr_cluster_params
{
	float transform[16];
	float clip_scale[4];
	float camera_base[3];
	float pad0;
	float camera_front[3];
	float pad1;
	float xy_scale[2];
	int32_t resolution_xy[2];
	float inv_resolution_xy[2];
	int32_t num_lights;
	int32_t num_lights_32;
	int32_t num_decals;
	int32_t num_decals_32;
	int32_t decals_texture_offset;
	int32_t z_max_index;
	float z_scale;
	float pad2[3];
} gr_cluster_params;

#define GR_MAX_LIGHTS_BINDLESS 4096
#define GR_CULL_SETUP_BYTES_PER_LIGHT 512        /* CullSetup {vec4 data[32]}, clusterer.cpp:1601 */
#define GR_TRANSFORMED_SPOT_BYTES_PER_LIGHT 96   /* TransformedSpot {vec4 clip[5]; vec4 z}, clusterer.cpp:1606 */

/* ClustererBindlessTransforms byte offsets (clusterer_data.h:46-53), total 852480 B (clusterer.cpp:1596). */
#define GR_TRANSFORMS_OFFSET_LIGHTS 0u
#define GR_TRANSFORMS_OFFSET_SHADOW 196608u
#define GR_TRANSFORMS_OFFSET_MODEL 458752u
#define GR_TRANSFORMS_OFFSET_TYPE_MASK 655360u
#define GR_TRANSFORMS_OFFSET_DECALS 655872u
#define GR_TRANSFORMS_SIZE 852480u

/* clusterer_bindless_spot_transform.comp; push = clusterer.cpp:1477-1493 (100 B). */
typedef struct gr_push_spot_transform
{
	float vp[16];
	float camera_pos[3];
	uint32_t num_lights;
	float camera_front[3];
	float z_near;
	float z_far;
} gr_push_spot_transform;
int gr_cluster_spot_transform(gr_ctx *ctx, gr_stream stream, const void *transforms, void *transformed_spots,
                              const gr_push_spot_transform *push);

/* clusterer_bindless_setup.comp; push = clusterer.cpp:1502-1509 (68 B).  params is passed by value (UBO). */
typedef struct gr_push_cluster_setup
{
	float view[16];
	uint32_t num_lights;
} gr_push_cluster_setup;
int gr_cluster_setup(gr_ctx *ctx, gr_stream stream, const void *transforms, const void *transformed_spots,
                     void *cull_setup, const gr_cluster_params *params, const gr_push_cluster_setup *push);

/* clusterer_bindless_binning.comp, SUBGROUPS variant at wave64 (8x8 cell tile per wave; clusterer.cpp:1516-1561).
 * bitmask[(y*res_x + x) * num_lights_32 + chunk]. */
int gr_cluster_binning(gr_ctx *ctx, gr_stream stream, const void *transforms, const void *cull_setup, uint32_t *bitmask,
                       const gr_cluster_params *params);

/* clusterer_bindless_z_range{,_opt}.comp; push = clusterer.cpp:1291-1300.  light_ranges: uvec2[num_volumes] slice
 * intervals (compute_uint_range, clusterer.cpp:1265-1275); out: uvec2[num_ranges] = [first, last] light index. */
typedef struct gr_push_z_range
{
	uint32_t num_volumes;
	uint32_t num_volumes_128;
	uint32_t num_ranges;
} gr_push_z_range;
int gr_cluster_z_range(gr_ctx *ctx, gr_stream stream, const uint32_t *light_ranges, uint32_t *out,
                       const gr_push_z_range *push);

/* The front of the cluster build as ONE launch: the four cmd.update_buffer of clusterer.cpp:1178-1207,1302, spot_transform.comp +
 * setup.comp (clusterer.cpp:1463-1510) and z_range.comp (:1277-1346) all depend on the frame's CPU-packed light data only.
 * src_* are the packed arrays in pinned host memory (gr_alloc_host) -- the launch copies them into `transforms` / `light_ranges`
 * as it reads them -- or NULL when the buffers already hold them.  Results are bit-identical to the separate launches above;
 * only gr_cluster_binning remains to be launched after it. */
typedef struct gr_cluster_front_args
{
	void *transforms;               /* device: GR_TRANSFORMS_SIZE bytes */
	const void *src_lights;         /* pinned: num_lights gr_light_info, or NULL */
	const void *src_models;         /* pinned: num_lights gr_mat_affine, or NULL */
	const void *src_type_mask;      /* pinned: num_lights_32 words, or NULL */
	void *transformed_spots;        /* device, out */
	void *cull_setup;               /* device, out */
	const gr_cluster_params *params;
	const gr_push_spot_transform *spot_push;
	const gr_push_cluster_setup *setup_push;
	const void *src_ranges;         /* pinned: z_push->num_volumes uvec2 slice intervals, or NULL */
	uint32_t *light_ranges;         /* device copy of the intervals */
	uint32_t *range_out;            /* device, out: uvec2[num_ranges] */
	const gr_push_z_range *z_push;
} gr_cluster_front_args;
int gr_cluster_front(gr_ctx *ctx, gr_stream stream, const gr_cluster_front_args *args);

/* DeferredLightRenderer::render_light (renderer.cpp:1004-1156): directional quad (directional.frag) then clustered quad
 * (clustering.frag), both additively blended into the RGBA16F HDR target with depth test NOT_EQUAL against z = 0.
 * One fused kernel; the intermediate blend result is rounded to fp16 exactly where the two reference draws round it:
 * hdr = rne16(rne16(emissive + directional) + clustered); alpha and far-plane pixels are copied through. */
typedef struct gr_push_directional /* renderer.cpp:1073-1103, 88 B used */
{
	float inv_view_proj_col2[4];
	float color[3];
	float environment_intensity;
	float camera_pos[3];
	float environment_mipscale;
	float direction[3];
	float cascade_log_bias;
	float camera_front[3];
	float pad0;
	float inv_resolution[2];
	float pad1[2];
} gr_push_directional;

typedef struct gr_push_clustering /* renderer.cpp:1110-1121 */
{
	float inv_view_proj_col2[4];
	float camera_pos[3];
	float pad0;
	float inv_resolution[2];
	float pad1[2];
} gr_push_clustering;

#define GR_LIGHTING_DIRECTIONAL_BIT 1u        /* draw the directional quad */
#define GR_LIGHTING_CLUSTERED_BIT 2u          /* draw the clustered quad */
#define GR_LIGHTING_AMBIENT_FALLBACK_BIT 4u   /* VOLUMETRIC_DIFFUSE_FALLBACK, renderer.cpp:1049-1055 */
#define GR_LIGHTING_AMBIENT_OCCLUSION_BIT 8u  /* AMBIENT_OCCLUSION (renderer.cpp:1050-1051): `ambient_occlusion` scales the
                                                 fallback ambient term, directional.frag:52-64.  Needs the fallback bit. */
/* Scheduling hint, no effect on any value: register-heavy passes of other streams run beside this launch (the temporal resolve and the
 * SMAA passes of the frame before: 512-thread workgroups of 64 registers, i.e. 128 per SIMD).  The launch then leaves them a quarter of each SIMD's register
 * file -- four resident workgroups per CU instead of five.  Measured (profiles/r05_lighting_instruction_diet.txt): five are 3 % faster
 * for a lighting + bloom + tonemap frame, 5-10 % slower for the TAA High + SMAA Ultra frame. */
#define GR_LIGHTING_SHARE_REGISTERS_BIT 16u

typedef struct gr_lighting_args
{
	gr_image albedo; /* R8G8B8A8_SRGB, a = ambient */
	gr_image normal; /* A2B10G10R10_UNORM_PACK32 */
	gr_image pbr;    /* R8G8_UNORM (metallic, roughness) */
	gr_image depth;  /* D32_SFLOAT, reverse-Z */
	gr_image emissive; /* R16G16B16A16_SFLOAT blend destination contents before the draws (G-buffer emissive) */
	gr_image hdr;    /* R16G16B16A16_SFLOAT result.  May alias `emissive` (same ptr): that is the reference's
	                    add_color_output("HDR", info, "emissive") read-modify-write; distinct buffers give the same
	                    values and bytes without clobbering the G-buffer. */
	float inv_view_projection[16]; /* DirectionalLightUBO / clustering.vert UBO */
	gr_push_directional directional;
	gr_push_clustering clustering;
	gr_cluster_params cluster;     /* UBO, by value */
	const void *transforms;        /* cluster-transforms buffer */
	const uint32_t *bitmask;       /* cluster-bitmask */
	const uint32_t *range;         /* cluster-range, uvec2[res_z] */
	uint32_t flags;
	gr_rows rows;                  /* render area; {0, 0} = whole target */
	gr_image ambient_occlusion;    /* R8_UNORM, any size, sampled LinearClamp at the pixel centre (LightingParameters::
	                                  ambient_occlusion, renderer.cpp:611-612); read only with the AMBIENT_OCCLUSION bit */
	/* The fog quad render_light draws last when LightingParameters::fog.falloff > 0 (renderer.cpp:1179-1196, lights/fog.{vert,frag},
	 * fog.h): src = (fog_color, exp2(-|world_pos - camera_pos|^2 * falloff)) blended ONE_MINUS_SRC_ALPHA / SRC_ALPHA into the target
	 * (colour and alpha), under the lighting quads' depth test.  falloff <= 0 = no fog (a zeroed struct). */
	float fog_color[3];
	float fog_falloff;
} gr_lighting_args;
/* Two pixels per lane where the width is even and pitch and ptr of every attachment are multiples of two texels, else one pixel per lane.
 * The kernel forms byte offsets in 32 bits: each of hdr, emissive, albedo, normal, pbr and depth with
 * pitch_bytes * height above 2^32 - 1 is refused with GR_ERR_INVALID_ARGUMENT and its name (ambient_occlusion has no such limit). */
int gr_lighting(gr_ctx *ctx, gr_stream stream, const gr_lighting_args *args);

/* 24-bit transport form of an RGBA8 target whose alpha byte is 255 everywhere (a tonemapped frame): the row-band executor
 * all-gathers its finished bands in this form (3/4 of the bytes over xGMI) and restores the RGBA8 rows on arrival.  `packed` is a
 * width x height x 3 byte image (row y at y * width * 3); *_rows restrict the rows as everywhere else (16-byte accesses where pitch, base and
 * width allow, bytes otherwise).  No reference counterpart (Granite renders a frame on one device). */
int gr_pack_rgb8_rows(gr_ctx *ctx, gr_stream stream, const gr_image *image, const gr_rows *rows, void *packed);
int gr_unpack_rgb8_rows(gr_ctx *ctx, gr_stream stream, const void *packed, const gr_image *image, const gr_rows *rows);

/* builtin://shaders/blit.frag over a full-screen quad (FragColor = textureLod(uTex, vUV, 0)): the copy between targets of
 * different size / format that Granite's tools record (tools/aa_bench.cpp:97-105 into the HDR target with LinearClamp,
 * :138-147 into the swapchain with NearestClamp).  in / out: R16G16B16A16_SFLOAT, R8G8B8A8_UNORM or R8G8B8A8_SRGB (decoded on
 * the fetch / encoded by the store, as the image views would); linear != 0 = StockSampler::LinearClamp, else NearestClamp.
 * 32-bit byte offsets: `in` or `out` with pitch_bytes * height above 2^32 - 1 is refused (GR_ERR_INVALID_ARGUMENT, by name). */
int gr_blit(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, int linear);

/* ---- anti-aliasing (renderer/post/{fxaa,smaa,temporal}.cpp) ------------------------------------------------------------
 * The kernels of every launcher of this section (gr_fxaa, gr_smaa_edge_detection, gr_smaa_blend_weight, gr_smaa_neighbor_blend,
 * gr_taa_resolve and their *_rows / *_band forms) form byte offsets in 32 bits: any image argument with pitch_bytes * height above
 * 2^32 - 1 is refused with GR_ERR_INVALID_ARGUMENT and its name, before anything is launched. */

/* setup_fxaa_postprocess (fxaa.cpp:28-55) + fxaa.frag.  `in` is read through its UNORM alias (cmd.set_unorm_texture):
 * the stored bytes of the tonemapped R8G8B8A8_SRGB image.  out: R8G8B8A8_SRGB or _UNORM (same bytes either way: the
 * shader's decode_srgb and the attachment's encode cancel). */
typedef struct gr_push_fxaa
{
	float inv_resolution[2];
} gr_push_fxaa;
int gr_fxaa(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, const gr_push_fxaa *push);
/* The anti-aliasing passes over a render area (row bands): *_rows = the same pass restricted to output
 * rows [first, first + count); what a pass reads above and below its band is the executor's business (StripPlan). */
int gr_fxaa_rows(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, const gr_push_fxaa *push, const gr_rows *rows);

/* SMAA 1x (smaa.cpp:32-208 + SMAA.hlsl).  quality 0..3 = SMAA_PRESET_LOW..ULTRA (smaa_common.h).
 * rt_metrics = (1/w, 1/h, w, h) (smaa.cpp:129-133). */
typedef struct gr_push_smaa
{
	float rt_metrics[4];
} gr_push_smaa;
/* AreaTex 160x560 R8G8_UNORM and SearchTex 64x16 R8_UNORM payloads (assets/textures/smaa/{area,search}.gtx), host pointers. */
int gr_smaa_set_luts(gr_ctx *ctx, const void *area_rg8, const void *search_r8);
/* smaa-edge pass: SMAALumaEdgeDetectionPS.  edges: R8G8_UNORM; every pixel is written (0 where the shader discards). */
int gr_smaa_edge_detection(gr_ctx *ctx, gr_stream stream, const gr_image *color, const gr_image *edges, const gr_push_smaa *push, int quality);
/* smaa-weights pass: SMAABlendingWeightCalculationPS, SMAA_SUBPIXEL_MODE 0.  weights: R8G8B8A8_UNORM.  The reference's
 * D16 "smaa-mask" depth-EQUAL test is equivalent to "edge texel != 0", which is what the kernel tests. */
int gr_smaa_blend_weight(gr_ctx *ctx, gr_stream stream, const gr_image *edges, const gr_image *weights, const gr_push_smaa *push, int quality);
/* smaa-blend pass: SMAANeighborhoodBlendingPS.  Four pixels per lane where the width is a multiple of 4 and pitch and ptr of all three
 * images are multiples of 16 bytes, else one. */
int gr_smaa_neighbor_blend(gr_ctx *ctx, gr_stream stream, const gr_image *color, const gr_image *weights, const gr_image *out,
                           const gr_push_smaa *push);
int gr_smaa_edge_detection_rows(gr_ctx *ctx, gr_stream stream, const gr_image *color, const gr_image *edges, const gr_push_smaa *push,
                                int quality, const gr_rows *rows);
int gr_smaa_blend_weight_rows(gr_ctx *ctx, gr_stream stream, const gr_image *edges, const gr_image *weights, const gr_push_smaa *push,
                              int quality, const gr_rows *rows);
int gr_smaa_neighbor_blend_rows(gr_ctx *ctx, gr_stream stream, const gr_image *color, const gr_image *weights, const gr_image *out,
                                const gr_push_smaa *push, const gr_rows *rows);
/* setup_taa_resolve (temporal.cpp:199-266) + taa_resolve.frag.  quality 0..2 = TAAQuality Low/Medium/High.
 * history NULL => REPROJECTION_HISTORY = 0 (first frame).  current/out_color/history: R16G16B16A16_SFLOAT,
 * depth D32_SFLOAT, mv R16G16_SFLOAT.  reproj = T(.5,.5,0) S(.5,.5,1) VP_prev inv(VP_cur) (temporal.cpp:239-243). */
typedef struct gr_push_taa
{
	float reproj[16];
	float rt_metrics[4];
} gr_push_taa;
int gr_taa_resolve(gr_ctx *ctx, gr_stream stream, const gr_image *current, const gr_image *depth, const gr_image *mv,
                   const gr_image *history, const gr_image *out_color, const gr_image *out_history, const gr_push_taa *push, int quality);
int gr_taa_resolve_rows(gr_ctx *ctx, gr_stream stream, const gr_image *current, const gr_image *depth, const gr_image *mv,
                        const gr_image *history, const gr_image *out_color, const gr_image *out_history, const gr_push_taa *push, int quality,
                        const gr_rows *rows);
/* Row bands whose history only holds the rows around the band (no reference analogue): history_rows = the rows of
 * `history` that carry last frame's values on this device.  A resolved pixel whose reprojection (motion vector, or depth + reproj)
 * fetches a history row outside them stores 1 to *reach_flag, which must be memory the device can write and the host can read
 * (gr_alloc_host): such a frame is not the single-device frame, and the caller has to say so.  Both NULL = gr_taa_resolve_rows. */
int gr_taa_resolve_band(gr_ctx *ctx, gr_stream stream, const gr_image *current, const gr_image *depth, const gr_image *mv,
                        const gr_image *history, const gr_image *out_color, const gr_image *out_history, const gr_push_taa *push, int quality,
                        const gr_rows *rows, const gr_rows *history_rows, uint32_t *reach_flag);

/* ---- depth hierarchy ---------------------------------------------------------------------------------------------------
 * HiZPassState::build_render_pass (renderer/post/spd.cpp:141-194) + assets/shaders/post/hiz.comp: turns the depth
 * attachment into a full max-reduction mip chain of linearised depth.  Workgroups reduce 64 x 64 tiles down to one texel
 * (mips 0..6); one more workgroup reduces what is left, folding in the odd row / column of non-power-of-two levels.  The
 * shader hands over inside one dispatch through an atomic counter (hiz.comp:355-365); with eight XCD-private L2s that
 * hand-over is cheaper as a second, one-workgroup launch on the same stream, so the counter is accepted for interface
 * parity but not touched.
 *
 * Mip chains live in one allocation, level after level, each level tightly packed; level l of a w x h chain is
 * max(w >> l, 1) x max(h >> l, 1) texels (gr_mip_chain_offset / gr_mip_chain_size, in bytes). */
size_t gr_mip_chain_offset(uint32_t width, uint32_t height, uint32_t bytes_per_texel, uint32_t level);
size_t gr_mip_chain_size(uint32_t width, uint32_t height, uint32_t bytes_per_texel, uint32_t levels);

typedef struct gr_hiz_args
{
	gr_image depth;            /* D32_SFLOAT / R32_SFLOAT; texels past its edge repeat the edge (NearestClamp) */
	void *chain;               /* R32_SFLOAT mip chain */
	uint32_t chain_width;      /* level 0 of the chain: the input size rounded up to multiples of 64 (spd.cpp:214-215), */
	uint32_t chain_height;     /* halved when output_downsample */
	uint32_t chain_levels;     /* spd.cpp:212: max(1, floor_log2(max(w, h)) - output_downsample) */
	uint32_t output_downsample; /* 1: the transformed full-resolution level is not stored; chain level 0 is mip 1 */
	float z_transform[4];      /* column-major mat2, spd.cpp:164-165: depth -> (num, den), stored value min(num / den, 1e30) */
	uint32_t *counter;         /* the pass's "-counter" buffer (one uint32); never written, stays zero */
} gr_hiz_args;
int gr_hiz(gr_ctx *ctx, gr_stream stream, const gr_hiz_args *args);

/* ---- screen-space reflections ------------------------------------------------------------------------------------------------
 * SSRState::build_render_pass (renderer/post/ssr.cpp:84-173) with ffx-sssr/{classify,build_indirect,trace_primary}.comp, and
 * the apply pass (ssr.cpp:286-322, apply.frag).  gr_ssr_trace = classify (clears `output` / `ray_confidence`, lists one ray per
 * glossy (roughness < 0.2), reflective (hierarchy level 0 < 1) pixel -- one per 2 x 2 quad phase for non-mirror surfaces, with
 * copy flags), build_indirect (the counter buffer: indirect.xyzw, atomic_count = 0, copied_count) and trace_primary (GGX VNDF
 * reflection direction from the blue-noise dither layer `frame`, hierarchical traversal of the depth chain from mip 1,
 * hit validation, radiance from `light`) in one call.  The ray list is in tile order (8 x 8 tiles row-major, Z-order inside a
 * tile) -- one of the orders the shader's atomic append can produce -- so the wave-level early exit of the traversal is
 * reproducible.  texelFetch outside a level reads 0.  scratch: gr_ssr_scratch_bytes(width, height) bytes. */
typedef struct gr_ssr_args
{
	const void *depth_chain;      /* R32_SFLOAT mip chain as gr_hiz writes it ("<depth>-hier") */
	uint32_t chain_width, chain_height, chain_levels;
	gr_image pbr;                 /* R8G8_UNORM */
	gr_image normal;              /* A2B10G10R10_UNORM_PACK32 */
	gr_image light;               /* R16G16B16A16_SFLOAT: the lit target rays fetch radiance from */
	const void *dither_lut;       /* R8G8_UNORM 128 x 128 x 64 layers (ssr.cpp:178-205) */
	uint32_t frame;               /* dither layer, 0..63 (ssr.cpp:161) */
	float view_projection[16];    /* column-major */
	float inv_view_projection[16];
	float camera_position[3];
	gr_image output;              /* R16G16B16A16_SFLOAT "<output>-sssr" */
	gr_image ray_length;          /* R16_SFLOAT */
	gr_image ray_confidence;      /* R8_UNORM */
	uint32_t *ray_list;           /* width * height dwords */
	uint32_t *ray_counter;        /* >= 6 dwords */
	void *scratch;
} gr_ssr_args;
size_t gr_ssr_scratch_bytes(uint32_t width, uint32_t height);
int gr_ssr_trace(gr_ctx *ctx, gr_stream stream, const gr_ssr_args *args);

typedef struct gr_ssr_apply_args
{
	gr_image hdr;       /* R16G16B16A16_SFLOAT, read-modify-write: blend ONE / ONE, fp16 rounding of the sum */
	gr_image reflected; /* "<output>-sssr", NearestClamp at the pixel centre */
	gr_image albedo;    /* R8G8B8A8_SRGB */
	gr_image normal;
	gr_image pbr;
	gr_image depth;     /* D32_SFLOAT: pixels at exactly 1.0 are skipped (depth test NOT_EQUAL against the quad at z = 1) */
	gr_image brdf_lut;  /* R16G16_SFLOAT split-sum table (builtin://textures/ibl_brdf_lut.gtx), LinearClamp at (NoV, roughness) */
	float inv_view_projection[16];
	float camera_position[3];
} gr_ssr_apply_args;
int gr_ssr_apply(gr_ctx *ctx, gr_stream stream, const gr_ssr_apply_args *args);

/* ---- single-pass downsampler ----------------------------------------------------------------------------------------------
 * emit_single_pass_downsample (renderer/post/spd.cpp:56-102) + assets/shaders/post/ffx-spd/spd.comp (AMD FidelityFX SPD):
 * fills an RGBA16F mip chain from an RGBA16F image in one call -- SPDInfo's input, output_mips[0..num_mips), num_components,
 * filter_mod and mode.  Level 0 of the chain is width x height (the size of output_mips[0]: half the input when the input
 * is the level above it, as in the reference's use), written from one LinearClamp tap per texel at the centre of its 2 x 2
 * source footprint (NearestClamp of the co-located texel in depth mode); levels 1.. are 2 x 2 averages (minima of .x in
 * depth mode) with SPD's rounding points: fp32 inside a 64 x 64 source tile down to level 5, level 6 from level 5 as
 * stored.  Every store is multiplied by filter_mods[level] (mips x vec4, host memory, NULL = none) and cut to `components`
 * channels (the rest written as 0).  Texels of a level that lie outside max(size >> level, 1) do not exist; the chain is
 * laid out as gr_mip_chain_offset(width, height, 8, level) says.  The shader's atomic counter buffer has no counterpart:
 * the last-workgroup stage is a second launch on the same stream. */
#define GR_SPD_REDUCTION_COLOR 0u
#define GR_SPD_REDUCTION_DEPTH 1u
typedef struct gr_spd_args
{
	gr_image input;            /* R16G16B16A16_SFLOAT */
	void *chain;               /* R16G16B16A16_SFLOAT mip chain, `mips` levels */
	uint32_t width, height;    /* level 0 of the chain = push.base_image_resolution (spd.cpp:85-86) */
	uint32_t mips;             /* 1..12 */
	uint32_t components;       /* 1..4: COMPONENTS */
	uint32_t reduction_mode;   /* GR_SPD_REDUCTION_* */
	const float *filter_mods;  /* FILTER_MOD: mips x 4 floats in host memory, or NULL */
} gr_spd_args;
int gr_spd_downsample(gr_ctx *ctx, gr_stream stream, const gr_spd_args *args);

/* ---- spatial upscaling after the post chain ---------------------------------------------------------------------------
 * setup_after_post_chain_upscaling (renderer/post/aa.cpp:75-174).  Both images R8G8B8A8_{UNORM,SRGB}.
 * gr_fsr_upscale: the "-scale" pass, upscale.{vert,frag} + FsrEasu{F,H} with the constants of FsrEasuCon (viewport = input
 * size): reads the stored (gamma-space) bytes of `in`, writes out->width x out->height.  fp16 != 0 selects the FP16 shader
 * variant (the reference's choice on hardware with fp16 arithmetic, aa.cpp:118-119).  The value written is the gamma-space
 * result for either output format (TARGET_SRGB decodes and the *_SRGB store re-encodes).
 * gr_fsr_sharpen: the "-sharpen" pass, sharpen.{vert,frag} + FsrRcasF; sharpness = exp2(-stops), FsrRcasCon (aa.cpp:64-74,
 * 0.5 stops at :157).  With an *_SRGB output the input is read through its sRGB view (linear) and the store encodes
 * (aa.cpp:147-151); with a UNORM output bytes go straight through. */
int gr_fsr_upscale(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, int fp16);
int gr_fsr_sharpen(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, float sharpness);

/* ---- HDR10 output ---------------------------------------------------------------------------------------------------------
 * setup_hdr10_pq_encoding (renderer/post/hdr.cpp:595-658) + pq10_encode.frag: out = PQ(soft-clip(primary_conversion *
 * (hdr * hdr_pre_exposure * ui.a + ui.rgb * ui_pre_exposure) / max) * max) in the display's primaries.  hdr R16G16B16A16_SFLOAT
 * (texel fetch), ui R8G8B8A8 read through its sRGB view, out A2B10G10R10_UNORM_PACK32 (alpha 1); all the same size.  The
 * push block is byte-identical to the shader's UBO (hdr.cpp:626-633). */
typedef struct gr_push_pq10
{
	float primary_conversion[16]; /* mat4(compute_rec709_to_st2020(metadata)), column major; the 3 x 3 part is used */
	float hdr_pre_exposure;
	float ui_pre_exposure;
	float max_light_level;        /* VkHdrMetadataEXT::maxContentLightLevel */
	float inv_max_light_level;
} gr_push_pq10;
int gr_pq10_encode(gr_ctx *ctx, gr_stream stream, const gr_image *hdr, const gr_image *ui, const gr_image *out, const gr_push_pq10 *push);
/* ---- video frame conversion -----------------------------------------------------------------------------------------------
 * VideoScaler::rescale (video/scaler.cpp) + assets/shaders/util/scaler.comp: what the headless runner's --video-encode-path does
 * to every frame before FFmpeg encodes it.  input: R8G8B8A8_UNORM / _SRGB (an *_SRGB input is decoded as its sampled view does),
 * A2B10G10R10_UNORM_PACK32 or R16G16B16A16_SFLOAT.  planes:
 *   1 plane   R8G8B8A8 / B8G8R8A8 (UNORM or SRGB; stored as UNORM like the reference's storage view), 4 x 4 ordered dither;
 *   2 planes  R8 + R8G8 (NV12) or R16_UNORM + R16G16_UNORM (P010 / P016): Y and interleaved Cb Cr;
 *   3 planes  R8 x 3 or R16_UNORM x 3: Y, Cb, Cr.
 * The chroma planes have the luma plane's size (4:4:4) or half of it rounded up (4:2:0: the mean of each 2 x 2 block).  YCbCr is
 * full range, BT.2020 for an HDR10 output and BT.709 otherwise.  When planes[0] differs in size from the input, the frame is
 * rescaled with the reference's 8-tap, 256-phase Hann-windowed sinc (above a ratio of 2: a bilinear prefilter to twice the target
 * size first).  Colour spaces are VkColorSpaceKHR values.  The first call with a new pair of sizes builds that size's fp16 weight
 * table on the device (an allocation: not inside a graph capture; its upload is ordered on `stream`); the table is kept with the context.
 * Stores outside a plane are dropped; out-of-frame input texels read as zero on the same-size path. */
#define GR_COLOR_SPACE_SRGB_NONLINEAR 0u
#define GR_COLOR_SPACE_EXTENDED_SRGB_LINEAR 1000104002u
#define GR_COLOR_SPACE_HDR10_ST2084 1000104008u
/* scaler.comp CONTROL bits and transfer functions */
#define GR_VIDEO_CONTROL_SKIP_RESCALE_BIT 1u
#define GR_VIDEO_CONTROL_DOWNSCALING_BIT 2u
#define GR_VIDEO_CONTROL_SAMPLED_DOWNSCALING_BIT 4u
#define GR_VIDEO_CONTROL_CLAMP_COORD_BIT 8u
#define GR_VIDEO_CONTROL_CHROMA_SUBSAMPLE_BIT 16u
#define GR_VIDEO_CONTROL_PRIMARY_CONVERSION_BIT 32u
#define GR_VIDEO_CONTROL_DITHER_BIT 64u
#define GR_VIDEO_TRANSFER_IDENTITY 0u
#define GR_VIDEO_TRANSFER_SRGB 1u
#define GR_VIDEO_TRANSFER_PQ 2u
/* scaler.comp Registers (push constants), byte-identical */
typedef struct gr_push_video
{
	int32_t resolution[2];        /* input size */
	float scaling_to_input[2];    /* input / output size, at most 2 */
	float inv_input_resolution[2];
	float dither_strength;
} gr_push_video;
/* Everything VideoScaler::rescale decides for one conversion */
typedef struct gr_video_plan
{
	uint32_t flags;                  /* GR_VIDEO_CONTROL_* */
	uint32_t eotf, oetf;             /* GR_VIDEO_TRANSFER_* (both identity when they cancel on a same-size conversion) */
	uint32_t num_planes;
	gr_push_video push;
	float gamma_space_transform[12]; /* row major 3 x 4: rows Cr, Y, Cb of [R G B 1] */
	float primary_transform[9];      /* column major, sdr_scale included; identity without PRIMARY_CONVERSION */
} gr_video_plan;
int gr_video_scale(gr_ctx *ctx, gr_stream stream, const gr_image *input, const gr_image *planes, uint32_t num_planes,
                   uint32_t input_color_space, uint32_t output_color_space);
/* Host-only (no device): the plan gr_video_scale would launch (image pointers are not read), and the fp16 weight table of
 * update_weights for these sizes, out[2][256][8] (horizontal, vertical).  Negative on arguments gr_video_scale refuses. */
int gr_video_scale_plan(const gr_image *input, const gr_image *planes, uint32_t num_planes, uint32_t input_color_space,
                        uint32_t output_color_space, gr_video_plan *plan);
int gr_video_scaler_weights(uint32_t input_width, uint32_t input_height, uint32_t output_width, uint32_t output_height, uint16_t *out);

/* ---- video frame playback -------------------------------------------------------------------------------------------------
 * VideoDecoder::Impl::init_yuv_to_rgb + dispatch_conversion (video/ffmpeg_decode.cpp) + assets/shaders/util/yuv_to_rgb.comp: what
 * the decoder does to every decoded frame, minus the decoder.  planes:
 *   1 plane   R8_UNORM / R16_UNORM luma only (chroma is the constant 128 / 255);
 *   2 planes  R8 + R8G8 (NV12 / NV21) or R16_UNORM + R16G16_UNORM (P010 / P016): Y and interleaved chroma;
 *   3 planes  R8 x 3 or R16_UNORM x 3: Y, Cb, Cr.
 * Chroma planes have the luma plane's size (4:4:4) or half of it rounded up (4:2:0).  Luma is fetched nearest, chroma bilinearly
 * (LinearClamp, the library's sampler model) at min((coord + chroma_siting) * inv_resolution, chroma_clamp).  out has the luma
 * plane's size and is
 *   R8G8B8A8_UNORM / _SRGB        (info.pq == 0) the non-linear code, stored through the UNORM view, 4 x 4 ordered dither;
 *   A2B10G10R10_UNORM_PACK32      (info.pq != 0) PQ content left encoded, dither still added as the reference does;
 *   R16G16B16A16_SFLOAT           (info.pq != 0) ST 2084 EOTF, scaled to scRGB (80 nits = 1), then primary_conversion.
 * Any row pitch and byte offset; everything else is refused with GR_ERR_INVALID_ARGUMENT before anything is launched. */
#define GR_VIDEO_MATRIX_UNSPECIFIED 0u /* by height: < 625 BT.601-525, < 720 BT.601-625, < 2160 BT.709, else BT.2020 */
#define GR_VIDEO_MATRIX_BT601_525 1u
#define GR_VIDEO_MATRIX_BT601_625 2u
#define GR_VIDEO_MATRIX_BT709 3u
#define GR_VIDEO_MATRIX_BT2020 4u
#define GR_VIDEO_MATRIX_SMPTE240M 5u
#define GR_VIDEO_CHROMA_CENTER 0u      /* chroma_siting (0.5, 0.5); also what an unspecified location means */
#define GR_VIDEO_CHROMA_LEFT 1u        /* (1.0, 0.5) */
#define GR_VIDEO_CHROMA_TOPLEFT 2u     /* (1.0, 1.0) */
#define GR_VIDEO_CHROMA_TOP 3u         /* (0.5, 1.0) */
#define GR_VIDEO_CHROMA_BOTTOMLEFT 4u  /* (1.0, 0.0) */
#define GR_VIDEO_CHROMA_BOTTOM 5u      /* (0.5, 0.0) */
/* yuv_to_rgb.comp UBO (std140), byte-identical */
typedef struct gr_push_yuv_to_rgb
{
	float yuv_to_rgb[16];         /* column major: M * scale(yuv_scale) * translate(yuv_bias) */
	float primary_conversion[16]; /* column major: source primaries -> BT.709 */
	uint32_t resolution[2];
	float inv_resolution[2];
	float chroma_siting[2];
	float chroma_clamp[2];
	float unorm_rescale;
} gr_push_yuv_to_rgb;
/* What the decoder knows about the stream */
typedef struct gr_video_yuv_info
{
	uint32_t bit_depth;       /* 8 (R8 planes), 10 or 16 (R16 planes) */
	uint32_t msb_aligned;     /* 10 bits only: 1 = in the high bits (P010), 0 = in the low bits (software decoders' YUV420P10) */
	uint32_t full_range;
	uint32_t matrix;          /* GR_VIDEO_MATRIX_* */
	uint32_t chroma_location; /* GR_VIDEO_CHROMA_* */
	uint32_t pq;              /* transfer function is ST 2084 */
	uint32_t nv21;            /* 2 planes: the chroma plane holds Cr Cb */
} gr_video_yuv_info;
/* Everything init_yuv_to_rgb and dispatch_conversion decide for one conversion: the UBO and the three specialization constants.
 * (A struct tag without a typedef: the function below carries the same name.) */
struct gr_video_yuv_plan
{
	gr_push_yuv_to_rgb push;
	uint32_t spec_pq, spec_num_planes, spec_nv21;
	uint32_t matrix;              /* the GR_VIDEO_MATRIX_* an unspecified one resolved to */
};
int gr_video_yuv_to_rgb(gr_ctx *ctx, gr_stream stream, const gr_image *planes, uint32_t num_planes, const gr_image *out,
                        const gr_video_yuv_info *info);
/* Host-only (no device): the plan gr_video_yuv_to_rgb would launch (image pointers are not read).  Negative on arguments
 * gr_video_yuv_to_rgb refuses. */
int gr_video_yuv_plan(const gr_image *planes, uint32_t num_planes, const gr_image *out, const gr_video_yuv_info *info,
                      struct gr_video_yuv_plan *plan);

/* ---- Block-compressed texture decode (vulkan/texture/texture_decoder.cpp, assets/shaders/decode/{s3tc,rgtc,bc7,bc6,astc}.comp) ---- */

/* Host-only. Decoded format of a block format as compressed_format_to_decoded_format (texture_decoder.cpp:28-129):
 * BC1/2/3/7 -> R8G8B8A8_UNORM or _SRGB (same bytes; the view differs), BC4 -> R8_UNORM, BC5 -> R8G8_UNORM,
 * BC6H -> R16G16B16A16_SFLOAT.  GR_FORMAT_UNDEFINED for anything else. */
uint32_t gr_texture_decoded_format(uint32_t block_format);
/* Host-only. Bytes per 4x4 block (8 or 16), 0 if not a block format handled here.
 * These two queries answer for BC1-BC7 only, as they always have: they give GR_FORMAT_UNDEFINED / 0 for every other number, the ASTC
 * formats included.  gr_texture_block_dim and gr_texture_block_info below answer for every format gr_texture_decode takes. */
uint32_t gr_texture_block_bytes(uint32_t block_format);
/* Host-only. Texels per block: 4 x 4 for BC1-BC7, the footprint (4 x 4 ... 12 x 12) for ASTC.  GR_ERR_UNSUPPORTED_FORMAT for a format
 * gr_texture_decode does not take, GR_ERR_INVALID_ARGUMENT for a NULL pointer. */
int gr_texture_block_dim(uint32_t block_format, uint32_t *width, uint32_t *height);
/* Host-only. Bytes per block and the decoded format (what out->format of gr_texture_decode must be) of BC1-BC7 and of the ASTC LDR
 * formats: ASTC _UNORM -> R8G8B8A8_UNORM, _SRGB -> R8G8B8A8_SRGB, 16 bytes.  Same codes as gr_texture_block_dim. */
int gr_texture_block_info(uint32_t block_format, uint32_t *block_bytes, uint32_t *decoded_format);
/* One level of one layer.  `blocks`: device pointer, ceil(w/bw) x ceil(h/bh) blocks of bw x bh texels (gr_texture_block_dim), rows
 * `block_row_pitch_bytes` apart (>= ceil(w/bw) * block bytes).  out->width/height are texel extents (at most 65536), out->format must
 * be the decoded format (gr_texture_block_info).
 * Texels outside out->width x out->height are not written.  Any out pitch >= the row's bytes and any byte alignment of
 * either pointer; everything else is refused with GR_ERR_INVALID_ARGUMENT / GR_ERR_UNSUPPORTED_FORMAT before a launch.
 * width or height 0 returns GR_OK without launching.
 * BC1 RGB stores alpha 255 everywhere, BC1 RGBA stores the punch-through texel as (0, 0, 0, 0); BC2 / BC3 colours are always four-colour;
 * BC6H stores alpha 0x3C00; reserved BC6H / BC7 modes store what the shaders store (zero endpoints); _SRGB formats store the _UNORM bytes.
 * ASTC decodes as astc.comp does in its 8-bit mode: endpoints interpolated in 16 bits as (c << 8) | 0x80 and the top byte stored, for
 * UNORM and SRGB alike; the error colour (0xff, 0, 0xff, 0xff) for an illegal block and, texel by texel, for the texels of a partition
 * whose endpoint mode is an HDR one; a void extent stores the top bytes of its colour whether or not its HDR flag is set. */
int gr_texture_decode(gr_ctx *ctx, gr_stream stream, uint32_t block_format, const void *blocks,
                      uint32_t block_row_pitch_bytes, const gr_image *out);

/* ---- Block-compressed texture encode and mip generation (scene-export/rgtc_compressor.cpp, texture_compression.cpp's
 * enqueue_compression_block_rgtc, texture_utils.cpp's generate_mipmaps).  Integer rules for the blocks, fp32 with one rounding an operation
 * for the mips: both give the bytes the reference's code gives on a CPU. ---- */

/* Host-only. 1 where gr_texture_encode takes the pair, 0 otherwise: GR_FORMAT_BC4_UNORM_BLOCK from R8_UNORM, R8G8_UNORM, R8G8B8A8_UNORM
 * or R8G8B8A8_SRGB; GR_FORMAT_BC5_UNORM_BLOCK from the last three.  No other block format is encoded. */
int gr_texture_encode_supported(uint32_t block_format, uint32_t input_format);
/* One level of one layer.  `in`: width x height texels (at most 65536 an axis) of one of the four formats above; its raw bytes are read,
 * component 0 for BC4, components 0 and 1 for BC5, so an _SRGB image is encoded as the numbers it holds.  Any in->pitch_bytes >= the
 * row's bytes and any byte alignment of in->ptr.
 * `blocks`: device pointer, receives ceil(w/4) x ceil(h/4) blocks of 8 (BC4) or 16 (BC5: the red block, then the green one) bytes, rows
 * `block_row_pitch_bytes` apart.  The pointer and the pitch must be multiples of the block size and the pitch >= ceil(w/4) blocks.
 * Exactly those blocks are written: no byte between the end of a row of blocks and the next row.  A block that reaches past the right or
 * bottom edge is filled with the last column / row of the image.
 * width or height 0 returns GR_OK without launching.  Refused before a launch, with the argument and the rule in gr_last_error:
 * a block format or input format other than the above and BC5 from R8_UNORM (GR_ERR_UNSUPPORTED_FORMAT); null pointers, an extent above
 * 65536, a pitch that does not cover a row, a misaligned `blocks` or block pitch (GR_ERR_INVALID_ARGUMENT). */
int gr_texture_encode(gr_ctx *ctx, gr_stream stream, uint32_t block_format, const gr_image *in, void *blocks,
                      uint32_t block_row_pitch_bytes);
/* One mip level of one layer: dst_level is the bilinear reduction of src_level as generate_mipmaps computes it, each destination texel
 * filtered from four taps of the source around its own centre, stored with round-half-away-from-zero.  Both images have the same format,
 * R8_UNORM, R8G8_UNORM or R8G8B8A8_UNORM, and dst_level is max(src >> 1, 1) texels an axis.  Any pitch that covers a row and any byte
 * alignment.  Refused before a launch: R8G8B8A8_SRGB (its filter works in linear light, which is not built), every other format and
 * two different formats (GR_ERR_UNSUPPORTED_FORMAT); null pointers, an empty image, a source above 65536 texels an axis, a dst_level of
 * another extent, a pitch that does not cover a row, images that share bytes (GR_ERR_INVALID_ARGUMENT). */
int gr_texture_generate_mipmap(gr_ctx *ctx, gr_stream stream, const gr_image *src_level, const gr_image *dst_level);

/* ---- environment baking ---------------------------------------------------------------------------------------------------
 * renderer/utils/image_utils.cpp: convert_equirect_to_cube, convert_cube_to_ibl_specular, convert_cube_to_ibl_diffuse
 * (skybox.vert + skybox_latlon.frag / util/ibl_specular.frag / util/ibl_diffuse.frag per face and level, generate_mipmap).
 * A cube is an R16G16B16A16_SFLOAT mip chain laid out as a GTX payload: levels in order, each starting 16-byte aligned; inside a
 * level the faces +X -X +Y -Y +Z -Z follow each other, rows tightly packed; level l is max(size >> l, 1) texels a side.
 * Cube pointers must be 16-byte aligned.  How a cube is sampled (face selection, seamless edges, trilinear) is DESIGN.md 7.8.
 * Refused before anything is launched: null pointers, size 0 or above 16384, levels 0 or beyond the chain of the size, unaligned
 * pointers (GR_ERR_INVALID_ARGUMENT), an equirect that is not R16G16B16A16_SFLOAT (GR_ERR_UNSUPPORTED_FORMAT). */
typedef struct gr_cube
{
	const void *ptr; /* device pointer */
	uint32_t size;   /* texels a side at level 0 */
	uint32_t levels;
} gr_cube;
/* Host-only. Bytes of a chain of `levels` levels, and the offset of a face of a level in it. */
uint64_t gr_cube_chain_bytes(uint32_t size, uint32_t levels);
uint64_t gr_cube_chain_offset(uint32_t size, uint32_t level, uint32_t face);
/* Level 0: the lat-long lookup of skybox_latlon.frag (LinearWrap, LOD 0) along each texel's direction; levels 1 and up: each a
 * linear-filter blit of the one above, per face, rounded to fp16 before the next reads it.  Alpha is 1. */
int gr_env_equirect_to_cube(gr_ctx *ctx, gr_stream stream, const gr_image *equirect, void *cube, uint32_t size, uint32_t levels);
/* GGX-prefiltered reflection chain: level l with roughness mix(0.001, 1, l / (out_levels - 1)), 1024 Hammersley samples read through
 * TrilinearWrap at lod = log2(src size) - log2(out_size) + l.  One launch for all faces and levels. */
int gr_env_specular(gr_ctx *ctx, gr_stream stream, const gr_cube *src, void *out, uint32_t out_size, uint32_t out_levels);
/* Irradiance: 252 x 63 hemisphere taps per texel through LinearWrap at lod = max(log2(out_size) - 5, 0); one level. */
int gr_env_diffuse(gr_ctx *ctx, gr_stream stream, const gr_cube *src, void *out, uint32_t out_size);

/* ---- FFT (renderer/fft/fft.{hpp,cpp}) ------------------------------------------------------------------------------------------
 * Complex-to-complex, real-to-complex and complex-to-real transforms in 1 to 3 dimensions, FP32 or FP16 in memory (arithmetic is fp32).
 * Forward C2C and R2C use the exponent sign -1, inverse C2C and C2R +1; nothing is normalised (inverse of forward gives N x).
 * nx, ny, nz: a dimension above `dimensions` with extent > 1 is a batch.  Transformed extents are powers of two of at least 4; for R2C
 * and C2R nx is the real length and at least 8.  R2C writes, and C2R reads, columns 0 .. nx / 2 of a row (nx / 2 + 1 complex numbers)
 * and nothing else of it; C2R does not read the imaginary parts of columns 0 and nx / 2 of its input rows (they are taken as zero
 * after the transforms along y and z, which makes a 2-D or 3-D C2R numpy's irfftn times N).
 * gr_fft_plan_create refuses (GR_ERR_INVALID_ARGUMENT): such extents, nx * ny * nz of 2^31 or more, texture input, texture output with
 * nz > 1 or with a real mode in one dimension or wider than 65536.  A plan owns its twiddle table and scratch buffers; creating one
 * allocates and synchronises, executing does neither.  A plan may be in flight on ONE stream at a time (the scratch is the plan's).
 * gr_fft_execute checks both resources before it launches anything (GR_ERR_INVALID_ARGUMENT, nothing launched): null pointers, a type
 * other than the plan's, misaligned pointers, a byte size below what the strides span, an odd stride on an FP16 real side, a row
 * stride below the row or a layer stride below the layer, source and destination byte ranges that overlap; an image of another
 * format than the mode stores (GR_ERR_UNSUPPORTED_FORMAT).  Every load and store lies inside the stated sizes. */
typedef enum gr_fft_mode
{
	GR_FFT_FORWARD_COMPLEX_TO_COMPLEX = 0,
	GR_FFT_INVERSE_COMPLEX_TO_COMPLEX = 1,
	GR_FFT_REAL_TO_COMPLEX = 2,
	GR_FFT_COMPLEX_TO_REAL = 3
} gr_fft_mode;
typedef enum gr_fft_data_type
{
	GR_FFT_FP32 = 0, /* float2; float on a real side */
	GR_FFT_FP16 = 1  /* half2; half on a real side */
} gr_fft_data_type;
typedef enum gr_fft_resource_type
{
	GR_FFT_RESOURCE_TEXTURE = 0,
	GR_FFT_RESOURCE_BUFFER = 1
} gr_fft_resource_type;
typedef struct gr_fft_options
{
	uint32_t nx, ny, nz;
	uint32_t dimensions;      /* 1 .. 3 */
	uint32_t mode;            /* gr_fft_mode */
	uint32_t data_type;       /* gr_fft_data_type */
	uint32_t input_resource;  /* gr_fft_resource_type; only buffers are accepted */
	uint32_t output_resource; /* gr_fft_resource_type */
} gr_fft_options;
/* A buffer (ptr, size_bytes, strides) or an image (image, output_offset).  Strides count elements: scalars on a real side, complex
 * numbers otherwise.  Texture output: R32G32_SFLOAT / R16G16_SFLOAT, or R32_SFLOAT / R16_SFLOAT for C2R, where complex column i goes to
 * texels 2 i and 2 i + 1; output_offset is added to the texel coordinate and a store outside the image is dropped. */
typedef struct gr_fft_resource
{
	uint32_t type; /* gr_fft_resource_type */
	void *ptr;     /* device pointer */
	uint64_t size_bytes;
	uint32_t row_stride;
	uint32_t layer_stride;
	gr_image image;
	int32_t output_offset[2];
} gr_fft_resource;
typedef enum gr_fft_pass_kind
{
	GR_FFT_PASS_C2C = 0,
	GR_FFT_PASS_R2C_RESOLVE = 1,
	GR_FFT_PASS_C2R_RESOLVE = 2
} gr_fft_pass_kind;
typedef enum gr_fft_buffer_id
{
	GR_FFT_BUFFER_SRC = 0,
	GR_FFT_BUFFER_DST = 1,
	GR_FFT_BUFFER_SCRATCH_A = 2,
	GR_FFT_BUFFER_SCRATCH_B = 3
} gr_fft_buffer_id;
typedef struct gr_fft_pass
{
	uint32_t kind;           /* gr_fft_pass_kind */
	uint32_t dimension;      /* 0 = x */
	uint32_t points;         /* points of one workgroup transform (the radix of the pass); 0 for a resolve */
	uint32_t p;              /* product of the radices of the earlier passes of this dimension; 0 for a resolve */
	uint32_t columns;        /* adjacent columns a workgroup holds */
	uint32_t workgroup_size;
	uint32_t grid_size;      /* workgroups */
	uint32_t lds_bytes;
	uint32_t reads, writes;  /* gr_fft_buffer_id */
} gr_fft_pass;
typedef struct gr_fft_plan gr_fft_plan;
/* Host-only (no context, no device): the passes a plan of these options runs, in order.  Returns their number (also when it exceeds
 * `capacity`; at most `capacity` are written), or GR_ERR_INVALID_ARGUMENT for options gr_fft_plan_create refuses. */
int gr_fft_describe(const gr_fft_options *options, gr_fft_pass *out, uint32_t capacity);
int gr_fft_plan_create(gr_ctx *ctx, const gr_fft_options *options, gr_fft_plan **plan);
void gr_fft_plan_destroy(gr_ctx *ctx, gr_fft_plan *plan);
uint32_t gr_fft_plan_iterations(const gr_fft_plan *plan);
int gr_fft_execute(gr_ctx *ctx, gr_stream stream, const gr_fft_plan *plan, const gr_fft_resource *dst, const gr_fft_resource *src);
/* One pass of the plan; all of them in order are gr_fft_execute. */
int gr_fft_execute_iteration(gr_ctx *ctx, gr_stream stream, const gr_fft_plan *plan, const gr_fft_resource *dst, const gr_fft_resource *src,
                             uint32_t iteration);

/* ---- ocean: the FFT update (renderer/ocean.cpp Ocean::update_fft_pass, assets/shaders/ocean/{generate_fft,bake_maps,mipmap}.comp) ----
 * The three dispatches of the pass that are neither an FFT nor the single-pass downsampler.  Push blocks are byte-identical to the
 * shaders'.  Images are linear fp16 images (gr_image) of the stated format, any pitch that covers a row; sampling is LinearWrap by the
 * model of DESIGN.md 7.10.  Everything refused is refused with GR_ERR_INVALID_ARGUMENT before anything is launched. */
#define GR_OCEAN_VARIANT_HEIGHT 0u
#define GR_OCEAN_VARIANT_GRADIENT_NORMAL 1u
#define GR_OCEAN_VARIANT_GRADIENT_DISPLACEMENT 2u
#define GR_OCEAN_NUM_FREQ_BANDS 8u
typedef struct gr_push_ocean_generate /* generate_fft.comp Registers, ocean.cpp:421-428 */
{
	float mod_factor[2]; /* 2 pi / world size */
	uint32_t N[2];
	float freq_to_band_mod;
	float time;
	float period;
} gr_push_ocean_generate;
typedef struct gr_push_ocean_bake /* bake_maps.comp Registers, ocean.cpp:519-523 */
{
	float inv_size[4]; /* 1 / height map size, 1 / displacement map size */
	float scale[4];    /* 1 / sample distance of the height map (xy) and of the displacement map (zw) */
} gr_push_ocean_bake;
typedef struct gr_push_ocean_mipmap /* mipmap.comp Registers, ocean.cpp:553-559 */
{
	float result_mod[4];
	float inv_resolution[2]; /* 1 / size of `in` */
	uint32_t count[2];       /* size of `out` */
	float lod;               /* accepted and unused: `in` is a single-level view */
} gr_push_ocean_mipmap;
/* One bin per lane: distribution N.x * N.y float2 (device), out N.x * N.y packed half2 (device), rows of N.x.  out[i] = (h0(i) e^{iwt} +
 * conj(h0(-i) e^{iwt})) times the variant's gradient factor and the band amplitude, w = round(sqrt(9.81 |k|) period) / period.
 * freq_bands: GR_OCEAN_NUM_FREQ_BANDS floats in host memory (FREQ_BAND_MODULATION), or NULL.  Refused: null pointers, N.x or N.y not a
 * power of two, N.x < 64, N.x * N.y >= 2^31, period <= 0, an unknown variant, a distribution not 8-byte or an out not 4-byte aligned.
 * All three entry points refuse an output that shares bytes with an input or with the other output: lanes would read what other lanes
 * of the same launch have written.  A NaN freq_to_band_mod selects band 0. */
int gr_ocean_generate_fft(gr_ctx *ctx, gr_stream stream, const void *distribution, void *out, const gr_push_ocean_generate *push,
                          uint32_t variant, const float *freq_bands);
/* height R16_SFLOAT, displacement R16G16_SFLOAT (any power-of-two size), grad_jacobian R16G16B16A16_SFLOAT of height's size =
 * (gradient.xy, jacobian, 0); height_displacement the same or NULL (VERTEX_TEXTURE = 0) = (height, 1.2 displacement.xy, 0). */
int gr_ocean_bake_maps(gr_ctx *ctx, gr_stream stream, const gr_image *height, const gr_image *displacement, const gr_image *grad_jacobian,
                       const gr_image *height_displacement, const gr_push_ocean_bake *push);
/* in and out of one format, R16_SFLOAT / R16G16_SFLOAT / R16G16B16A16_SFLOAT; out is push->count texels: one tap at
 * (2 gid + 1) * inv_resolution, times result_mod. */
int gr_ocean_mipmap(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, const gr_push_ocean_mipmap *push);

/* ---- ocean: the LOD update (renderer/ocean.cpp Ocean::update_lod_pass, assets/shaders/ocean/{update_lod,init_counter_buffer,cull_blocks}.comp) ----
 * One entry point per dispatch; push blocks are byte-identical to the shaders' std140 blocks.  All three refuse, before a launch: null
 * pointers; num_threads that is not square, not a power of two or outside 4 .. 128; a LOD image that is not R16_SFLOAT of exactly
 * num_threads; max_lod that is not an integer in 0 .. 7. */
typedef struct gr_push_ocean_update_lod /* update_lod.comp Registers, ocean.cpp:285-294 */
{
	float shifted_camera_pos[3];
	float max_lod;
	int32_t image_offset[2];
	int32_t num_threads[2];
	float grid_base[2];
	float grid_size[2];
	float lod_bias;
	uint32_t padding[3];
} gr_push_ocean_update_lod;
typedef struct gr_push_ocean_cull /* cull_blocks.comp Registers, ocean.cpp:335-349 */
{
	float world_offset[3];
	uint32_t padding0;
	int32_t image_offset[2];
	uint32_t num_threads[2];
	float inv_num_threads[2]; /* accepted and unused: the taps address texels */
	float grid_base[2];
	float grid_size[2];
	float grid_resolution[2];
	float heightmap_range[2];
	float guard_band;
	uint32_t lod_stride; /* patches per LOD bucket */
	float max_lod;
	int32_t handle_edge_lods;
	uint32_t padding1[2];
} gr_push_ocean_cull;
typedef struct gr_ocean_patch /* PatchData, ocean.inc */
{
	float offsets[2];
	float inner_lod;
	float padding;
	float lods[4]; /* -x, +x, -y, +y */
} gr_ocean_patch;
typedef struct gr_ocean_indirect_draw /* IndirectDraw, ocean.inc */
{
	uint32_t index_count, instance_count, first_index;
	int32_t vertex_offset;
	uint32_t first_instance, padding0, padding1, padding2;
} gr_ocean_indirect_draw;
typedef struct gr_ocean_buffer /* a storage buffer: device pointer and size */
{
	void *ptr;
	uint64_t size_bytes;
} gr_ocean_buffer;
/* lod_image(id + image_offset & (num_threads - 1)) = clamp(0.5 log2(d2 + 1) + lod_bias, 0, max_lod), d2 the least squared distance from
 * shifted_camera_pos to the block's centre and four corners at height 0. */
int gr_ocean_update_lod(gr_ctx *ctx, gr_stream stream, const gr_image *lod_image, const gr_push_ocean_update_lod *push);
/* Eight gr_ocean_indirect_draw: index_count from the first eight of counts16 (sixteen uint32_t in host memory, the shader's uniform
 * block), everything else zero.  Refused: counters below 8 * 32 bytes. */
int gr_ocean_init_counter_buffer(gr_ctx *ctx, gr_stream stream, const gr_ocean_buffer *counters, const uint32_t *counts16);
/* Per block that passes the box test against frustum (six float[4] planes in host memory): one gr_ocean_patch appended at
 * lod_stride * lod + slot, slot from counters[lod].instance_count.  wrap: the five nearest taps use NearestWrap (non-zero) or
 * NearestClamp (0).  Slots inside one 8 x 8 group are in row order; the order across groups is arbitrary.  Also refused: lod_stride <
 * num_threads.x * num_threads.y; patches below lod_stride * (max_lod + 1) * 32 bytes; counters below 8 * 32 bytes; buffers that overlap
 * each other or the image.  A bucket is kept inside 0 .. max_lod and a slot at or past lod_stride is not written, whatever the image and
 * the counters hold. */
int gr_ocean_cull_blocks(gr_ctx *ctx, gr_stream stream, const gr_image *lod_image, uint32_t wrap, const gr_ocean_buffer *patches,
                         const gr_ocean_buffer *counters, const gr_push_ocean_cull *push, const float *frustum);

/* ---- mesh decode (vulkan/mesh/meshlet.cpp decode_mesh, assets/shaders/decode/meshlet_decode.comp) ----------------------------------------
 * One launch expands the bit-packed streams of a MESHLET4 file into an index buffer, positions, {normal, tangent, uv} records and skin
 * records.  32 lanes per meshlet, eight meshlets per workgroup as in the shader; the grid is ceil(meshlet_count / 8) - wg_offset groups
 * (wg_offset is the shader's: the first group of this launch; the reference uses it to split a dispatch, here one launch always suffices).
 * Capacities are in elements (primitives for the index buffer, vertices for the rest) counted from the buffer's start, the push block's
 * offsets included: an element at or past its capacity is not written, a payload word at or past payload_words reads as 0, and counts
 * above 32 are clamped, whatever the device data holds.  Window, padding-word and rounding rules: granite_amd/csrc/meshlet_decode.hpp,
 * DESIGN.md 7.12. */
#define GR_MESHLET_DECODE_UNROLLED_MESH 1u /* DECODE_MODE_UNROLLED_MESH: 32-bit indices */
#define GR_MESHLET_DECODE_INDEX_16 2u      /* DECODE_MODE_INDEX_16: 16-bit indices; neither flag: 8-bit */
#define GR_MESHLET_STYLE_WIREFRAME 0u      /* streams 0-1 */
#define GR_MESHLET_STYLE_TEXTURED 1u       /* streams 0-3 */
#define GR_MESHLET_STYLE_SKINNED 2u        /* streams 0-5 */
typedef struct gr_push_meshlet_decode /* meshlet_decode.comp Registers, meshlet.cpp:247-253 */
{
	uint32_t primitive_offset;
	uint32_t vertex_offset;
	uint32_t meshlet_count;
	uint32_t wg_offset;
} gr_push_meshlet_decode;
typedef struct gr_meshlet_stream /* Meshlet::Stream, meshlet.hpp:47-56 */
{
	uint32_t base_value[2]; /* stream 0 of a meshlet: {prim_count, vert_count} */
	uint32_t bits;          /* low byte: bits per component; bits >> 16: auxiliary field */
	uint32_t offset_in_words;
} gr_meshlet_stream;
typedef struct gr_meshlet_offsets /* decode_mesh's Offsets, meshlet.cpp:209-214 */
{
	uint32_t primitive_output_offset;
	uint32_t vertex_output_offset;
	uint32_t index_offset;
} gr_meshlet_offsets;
typedef struct gr_meshlet_decode_args /* every pointer is a device pointer */
{
	const gr_meshlet_stream *streams; /* meshlet_count * stream_count, 16-byte aligned */
	const uint32_t *payload;
	uint32_t payload_words;
	uint32_t stream_count; /* 2, 4 or 6 */
	const gr_meshlet_offsets *offsets; /* meshlet_count */
	void *indices;                     /* 3 x uint32_t, uint16_t or uint8_t per primitive; any byte alignment */
	uint64_t index_capacity;
	float *positions; /* 3 floats per vertex, tightly packed */
	uint64_t position_capacity;
	void *attributes; /* {uint32 normal, uint32 tangent, float uv[2]} per vertex, 16-byte aligned; target_style >= 1 */
	uint64_t attribute_capacity;
	void *skin; /* {uint32 indices, uint32 weights} per vertex, 8-byte aligned; target_style 2 */
	uint64_t skin_capacity;
	uint32_t target_style; /* GR_MESHLET_STYLE_*, not above what stream_count provides */
	uint32_t flags;        /* GR_MESHLET_DECODE_* */
} gr_meshlet_decode_args;
/* Refused with GR_ERR_INVALID_ARGUMENT before anything is launched: null pointers the style needs, stream_count not 2, 4 or 6 or too
 * small for target_style, target_style above 2, unknown flags, payload_words of 0, pointers below their alignment.  meshlet_count 0, or
 * wg_offset at or past the last group, returns GR_OK without launching. */
int gr_meshlet_decode(gr_ctx *ctx, gr_stream stream, const gr_meshlet_decode_args *args, const gr_push_meshlet_decode *push);

/* ---- meshlet culling (renderer/scene_renderer.cpp build_mdi_culling_pass, assets/shaders/meshlet_cull.comp) -------------------------------
 * One launch tests `count` tasks of up to 32 chunks each: the task's AABB against the frustum, every chunk's bounding sphere and normal
 * cone against the frustum and the camera (inc/meshlet_render.h), in phase 2 both against the depth hierarchy, and compacts the
 * survivors into five-dword records {index_count, 1, first_index, vertex_offset, task_index} (VkDrawIndexedIndirectCommand) at
 * output[draw_indirect_offset + 5 * slot], slot from an atomic add on output[mdi_count_offset].  The records of one task are contiguous
 * and in chunk order; the order of tasks among each other is whatever the atomics give and is not specified.  The caller zeroes the
 * count word.  A record that would end past output_dwords is not written; the count still includes it.
 *   phase 0 (CullingPhase::OneShot)              no occluder word is read or written
 *   phase 1 (First, MotionVector)                reads: a task is skipped when its word is 0, a chunk when its bit is clear
 *   phase 2 (Second)                             writes: 0 for an invisible task, else the chunks visible now; chunks whose old bit was set
 *                                                are not drawn again unless FORCE_VISIBLE; adds the HiZ tests
 * The chain is the one gr_hiz writes with output_downsample = 1 (R32_SFLOAT, gr_mip_chain_offset(chain_width, chain_height, 4, level)).
 * Every index read from device data is held to the element count given here; what falls outside is not visible and is not read.
 * Arithmetic and its order: granite_amd/csrc/meshlet_cull.hpp. */
#define GR_MESHLET_CULL_ORTHO 1u         /* constant_id 0: projection[3].w == 1 */
#define GR_MESHLET_CULL_SKINNED 2u       /* constant_id 1: no per-chunk test, the AABB test only */
#define GR_MESHLET_CULL_FORCE_VISIBLE 4u /* constant_id 2, phase 2 only: draw what phase 1 drew as well */
typedef struct gr_push_meshlet_cull /* meshlet_cull.comp:23-29, scene_renderer.cpp:983-989 */
{
	uint32_t offset;               /* first task */
	uint32_t count;                /* tasks */
	uint32_t mdi_count_offset;     /* dword of the count word in the output buffer */
	uint32_t draw_indirect_offset; /* dword of the first record */
} gr_push_meshlet_cull;
typedef struct gr_meshlet_task /* MeshAssetDrawTaskInfo, inc/meshlet_render_types.h:15-22 */
{
	uint32_t aabb_instance;
	uint32_t occluder_state_offset;
	uint32_t node_instance;
	uint32_t mesh_index_count; /* first chunk (a multiple of 32) + chunks - 1 */
	uint32_t material_flags;
} gr_meshlet_task;
typedef struct gr_meshlet_aabb /* inc/meshlet_render_types.h:4-7 */
{
	float lo[3], pad0, hi[3], pad1;
} gr_meshlet_aabb;
typedef struct gr_meshlet_bound /* Meshlet::Bound, vulkan/mesh/meshlet.hpp:79-84; inc/meshlet_render_types.h:9-13 */
{
	float center[3];
	float radius;
	float cone_axis_cutoff[4];
} gr_meshlet_bound;
typedef struct gr_meshlet_draw /* RuntimeHeaderDecodedMDI, vulkan/mesh/meshlet.hpp:72-77; meshlet_cull.comp:16-21 */
{
	uint32_t index_count;
	uint32_t first_index;
	int32_t vertex_offset;
} gr_meshlet_draw;
typedef struct gr_meshlet_frustum /* inc/meshlet_ubos.h:4-14 (std140), renderer.cpp:540-572 */
{
	float viewport[4];
	float planes[6][4];
	float view[16]; /* column major */
	float viewport_scale_bias[4];
	int32_t hiz_resolution[2];
	float winding;
	int32_t hiz_min_lod;
	int32_t hiz_max_lod;
	uint32_t pad[3];
} gr_meshlet_frustum;
typedef struct gr_meshlet_cull_args /* every pointer is a device pointer; counts are in elements */
{
	const gr_meshlet_task *tasks;
	uint32_t task_count;
	uint32_t aabb_count;
	const gr_meshlet_aabb *aabbs;           /* 16-byte aligned */
	const gr_mat_affine *transforms;        /* mat_affine of inc/affine.h:4-7 (gr_mat_affine above); 16-byte aligned; not read when SKINNED */
	const gr_meshlet_bound *bounds;         /* 16-byte aligned, one per chunk; not read when SKINNED */
	uint32_t transform_count;
	uint32_t bound_count;
	const gr_meshlet_draw *draws;           /* one per chunk */
	uint32_t draw_count;
	uint32_t occluder_count;
	uint32_t *occluders;                    /* phases 1 and 2 */
	uint32_t *output;                       /* count words and records */
	uint64_t output_dwords;
	const void *chain;                      /* phase 2 */
	uint32_t chain_width, chain_height, chain_levels;
	uint32_t phase;                         /* 0, 1 or 2 */
	uint32_t flags;                         /* GR_MESHLET_CULL_* */
	float camera_position[3];
	gr_meshlet_frustum frustum;
} gr_meshlet_cull_args;
/* ceil(count / 64) waves; count 0 returns GR_OK without a launch.  Refused with GR_ERR_INVALID_ARGUMENT before anything is launched, the
 * message naming the field: a phase above 2, unknown flags, a null or misaligned pointer the phase and flags need (occluders in phases 1
 * and 2, chain in phase 2, transforms and bounds unless SKINNED), in phase 2 a frustum whose hiz_resolution is not
 * (chain_width, chain_height) << hiz_min_lod or whose hiz_max_lod is not chain_levels - 1 + hiz_min_lod, and mdi_count_offset or
 * draw_indirect_offset outside output_dwords. */
int gr_meshlet_cull(gr_ctx *ctx, gr_stream stream, const gr_meshlet_cull_args *args, const gr_push_meshlet_cull *push);

/* ---- volumetric decals: the clusterer's second client (renderer/lights/clusterer.cpp:1348-1461,1564-1573) ----------------------------------
 * A decal is the unit box under a transform, with a texture; it acts on base colour from the world position alone.  Arithmetic, the
 * sampler and LOD model: granite_amd/csrc/decal_core.hpp, DESIGN.md 7.14. */
#define GR_MAX_DECALS_BINDLESS 4096 /* CLUSTERER_MAX_DECALS */

/* clusterer_bindless_binning_decal.comp in its SUBGROUPS form at 64 lanes (8 x 8 cell tile per wave, decals in lanes 0-31 of a chunk).
 * mvps: column-major mat4[num_decals] on the device (view_projection x world).  bitmask[(y * res_x + x) * num_decals_32 + chunk]; no other
 * word is written.  num_decals 0 returns GR_OK without a launch.  Refused with GR_ERR_INVALID_ARGUMENT: null pointers, a resolution that
 * is not a positive multiple of 8, num_decals outside 0 .. GR_MAX_DECALS_BINDLESS, num_decals_32 that is not ceil(num_decals / 32).
 * The decal z ranges are gr_cluster_z_range over a second pair of buffers. */
int gr_cluster_binning_decal(gr_ctx *ctx, gr_stream stream, const float *mvps, uint32_t *bitmask, const gr_cluster_params *params);

/* One decal texture: R8G8B8A8_SRGB or R8G8B8A8_UNORM; level i is max(1, width >> i) x max(1, height >> i) texels, levels tightly packed
 * one after another from `levels` (device memory, 4-byte aligned).  The records live in device memory, so gr_decal_apply cannot look at them:
 * it is the caller's contract that every record a decal can name has width and height of at least 1, num_levels of 1 .. the full chain's
 * count (floor(log2(max(width, height))) + 1), one of the two formats, and `levels` covering all of its levels.  A record that breaks it
 * makes the kernel read outside the texture (gra_set_decal_texture refuses such a texture before it reaches the device). */
typedef struct gr_decal_texture
{
	const void *levels;
	uint32_t width, height, num_levels, format;
} gr_decal_texture;

/* lights/volumetric_decal.h (apply_volumetric_decals) on a G-buffer already written: per pixel with depth != 0, the decals of the pixel's
 * cluster cell and z slice in ascending index order, rgb = mix(rgb, decal.rgb, decal.a).  Alpha is never changed; a pixel no decal reaches
 * is not written.  Decal i samples textures[cluster.decals_texture_offset + i]; an index outside [0, num_textures) skips the decal.
 * cluster.num_decals 0 returns GR_OK without a launch.  Refused with GR_ERR_INVALID_ARGUMENT before anything is launched: an image that
 * breaks the gr_image contract, albedo and depth of different sizes, a null transforms, bitmask_decal, range_decal or textures, a cluster
 * block whose resolution, num_decals, num_decals_32 or z_max_index is out of range. */
typedef struct gr_decal_apply_args
{
	gr_image albedo;               /* R8G8B8A8_SRGB, read-modify-write */
	gr_image depth;                /* D32_SFLOAT, reverse-Z: 0 is the far plane */
	float inv_view_projection[16]; /* column-major */
	gr_cluster_params cluster;     /* UBO, by value */
	const void *transforms;        /* GR_TRANSFORMS_SIZE bytes; world_to_texture rows at GR_TRANSFORMS_OFFSET_DECALS */
	const uint32_t *bitmask_decal; /* gr_cluster_binning_decal's output */
	const uint32_t *range_decal;   /* uvec2[z_max_index + 1] */
	const gr_decal_texture *textures; /* device array */
	uint32_t num_textures;
	uint32_t pad0;
} gr_decal_apply_args;
int gr_decal_apply(gr_ctx *ctx, gr_stream stream, const gr_decal_apply_args *args);

/* ---- the sky pass (renderer/mesh_util.cpp:1046-1142 Skybox, skybox.vert / skybox.frag, lights/atmospheric_scatter.h) ------------------------
 * The reference draws the skybox as a full-screen quad at z = 0 with depth test GREATER_OR_EQUAL against a depth buffer cleared to 0: it
 * writes the emissive attachment exactly where depth == 0.  Arithmetic, the pixel's direction and the cube LOD model:
 * granite_amd/csrc/sky_core.hpp, DESIGN.md 7.15.
 * Where depth == 0.0f (a float compare: -0.0 is far) rgb is written: without a cube color * rayleigh_mie_scatter(normalize(direction),
 * sun_direction, camera_height, 16, 8), with a cube texture(cube, direction).rgb * color through LinearClamp.  The alpha of an
 * R16G16B16A16_SFLOAT texel keeps its value; a B10G11R11 store rounds as every attachment store of this library.  No other pixel is stored
 * to.  The cube is absent when ptr, size and levels are all 0.
 * Refused with GR_ERR_INVALID_ARGUMENT before anything is launched: an image that breaks the gr_image contract (emissive of another format
 * than the two, depth that is not D32_SFLOAT or not of the emissive's size, null pointers); a cube with a null ptr, size 0 or above 16384,
 * levels 0 or beyond the chain of the size, or a ptr that is not 16-byte aligned. */
typedef struct gr_sky_args
{
	gr_image emissive;                   /* R16G16B16A16_SFLOAT or B10G11R11_UFLOAT_PACK32; far pixels are written */
	gr_image depth;                      /* D32_SFLOAT, reverse-Z: 0 is the far plane */
	float inv_local_view_projection[16]; /* column-major: inverse(projection * view with its translation zeroed) */
	float color[3];
	float camera_height;
	float sun_direction[3];
	float pad0;
	gr_cube cube; /* optional: the gr_env_* chain layout */
} gr_sky_args;
int gr_sky_apply(gr_ctx *ctx, gr_stream stream, const gr_sky_args *args);

/* lights/volumetric_light_setup_sky.comp: the atmosphere along base_dirs + pos_du * u + pos_dv * v of inc/cube_coordinates.h, 32 primary
 * and 16 light steps, six faces of `size` texels in R16G16B16A16_SFLOAT with alpha 1: level 0 of the gr_env_* chain layout (6 * size^2 * 8
 * bytes), which gr_env_diffuse / gr_env_specular read as a cube of one level.  inv_resolution is 1.0f / size.
 * Refused with GR_ERR_INVALID_ARGUMENT before a launch: null pointers, size 0 or above 16384, out_chain not 16-byte aligned. */
typedef struct gr_sky_cube_params
{
	float sun_color[3];
	float camera_y;
	float sun_direction[3];
	float pad0;
} gr_sky_cube_params;
int gr_sky_cube(gr_ctx *ctx, gr_stream stream, void *out_chain, uint32_t size, const gr_sky_cube_params *params);

/* ---- directional-light shadows (lights/directional.frag with SHADOWS, lights/lighting_resources.h, pcf.h, vsm.h) ---------------------------
 * The shadowed directional quad as a launch of its own, the way DeferredLightRenderer::render_light draws it: per pixel with depth != 0
 * hdr = rne16(emissive + compute_lighting(.., shadow_term) [+ the ambient fallback]); far-plane pixels and alpha are copied through.
 * Followed by gr_lighting with GR_LIGHTING_CLUSTERED_BIT alone and emissive = hdr it gives the reference's own rounding sequence,
 * rne16(rne16(emissive + directional) + clustered).  Nothing rasterises here: the shadow maps are inputs, as the G-buffer is.
 * Arithmetic and the LinearShadow sampler model (compare GREATER_OR_EQUAL, linear, clamp to edge): granite_amd/csrc/shadow_core.hpp,
 * DESIGN.md 7.17.
 *   mode      GR_SHADOW_PCF: one LinearShadow fetch; GR_SHADOW_PCF_WIDE: SHADOW_MAP_PCF_KERNEL_WIDE, the 6 x 6 windowed kernel of nine
 *             gathers; both take D16_UNORM or D32_SFLOAT maps.  GR_SHADOW_VSM: R32G32_SFLOAT moments through LinearClamp and vsm().
 *   layers    4: SHADOW_CASCADES, cascade = log2(view_z) + directional.cascade_log_bias; 1: the plain variant, transforms[0] alone.
 *   flags     GR_LIGHTING_AMBIENT_FALLBACK_BIT, GR_LIGHTING_AMBIENT_OCCLUSION_BIT (needs the fallback bit); no other bit.
 * Every layer has the size, the format and the pitch rules of the first; a map is at most 16384 texels each way.
 * Refused with GR_ERR_INVALID_ARGUMENT before anything is launched: an image that breaks the gr_image contract -- hdr that is not
 * R16G16B16A16_SFLOAT (a B10G11R11_UFLOAT_PACK32 target is refused by name: its blend rounds differently and is not built), emissive, albedo,
 * normal, pbr or depth of another format or size, shadow_maps[i] of a format that does not fit the mode or unlike shadow_maps[0] -- a mode
 * other than the three, layers other than 1 or 4, a flag this entry point does not take, hdr sharing bytes with emissive other than by an
 * equal pointer or with any input.  The kernel forms byte offsets into the six frame attachments in 32 bits: each with pitch_bytes * height
 * above 2^32 - 1 is refused likewise (shadow maps and ambient_occlusion have no such limit). */
#define GR_SHADOW_PCF 1u
#define GR_SHADOW_PCF_WIDE 2u
#define GR_SHADOW_VSM 3u
#define GR_SHADOW_NUM_CASCADES 4
#define GR_SHADOW_MAX_EXTENT 16384u
typedef struct gr_directional_light_args
{
	gr_image albedo;   /* R8G8B8A8_SRGB */
	gr_image normal;   /* A2B10G10R10_UNORM_PACK32 */
	gr_image pbr;      /* R8G8_UNORM (metallic, roughness) */
	gr_image depth;    /* D32_SFLOAT, reverse-Z */
	gr_image emissive; /* R16G16B16A16_SFLOAT: the blend destination's contents before the draw */
	gr_image hdr;      /* R16G16B16A16_SFLOAT result; may be `emissive` (same ptr) */
	float inv_view_projection[16];
	gr_push_directional directional;
	uint32_t flags;
	uint32_t mode;   /* GR_SHADOW_* */
	uint32_t layers; /* 1 or 4 */
	uint32_t pad0;
	gr_image ambient_occlusion; /* R8_UNORM, any size; read only with GR_LIGHTING_AMBIENT_OCCLUSION_BIT */
	gr_image shadow_maps[GR_SHADOW_NUM_CASCADES];
	float transforms[GR_SHADOW_NUM_CASCADES][16]; /* DirectionalLightUBO::transforms, column-major: world -> (u, v, z) of a layer */
} gr_directional_light_args;
int gr_directional_light(gr_ctx *ctx, gr_stream stream, const gr_directional_light_args *args);

/* lights/resolve_vsm.frag: moments = (z, z * z) of a D16_UNORM or D32_SFLOAT map into an R32G32_SFLOAT image of the same size.  The
 * reference's own 4x MSAA average in front of it has no counterpart: nothing is rasterised here.
 * Refused with GR_ERR_INVALID_ARGUMENT: an image that breaks the gr_image contract or shares bytes with the other. */
int gr_vsm_moments(gr_ctx *ctx, gr_stream stream, const gr_image *depth, const gr_image *moments);

/* post/vsm_down_blur.frag (up = 0: taps at +-1.75 texels of `in`) and post/vsm_up_blur.frag (up != 0: +-0.875): nine LinearClamp taps around
 * the output pixel's centre, weights 0.25 / 0.125 / 0.0625, R32G32_SFLOAT to R32G32_SFLOAT of any size; one call per layer.
 * Refused with GR_ERR_INVALID_ARGUMENT: an image that breaks the gr_image contract or shares bytes with the other. */
int gr_vsm_blur(gr_ctx *ctx, gr_stream stream, const gr_image *in, const gr_image *out, int up);

/* ---- SSAO: FidelityFX CACAO as the reference runs it (renderer/post/ssao.cpp, renderer/post/ffx-cacao) -----------------------------------
 * One configuration and its non-adaptive sibling: native resolution, normals from the G-buffer, quality HIGHEST (adaptive, shader level 3)
 * or HIGH (shader level 2), 0 .. 8 blur passes.  One entry point per shader of FFX_CACAO_GraniteDraw (ffx_cacao_impl.cpp:767-1026); the
 * four per-pass dispatches of a stage are one launch.  Every intermediate lives in one caller-owned workspace of gr_cacao_workspace_bytes
 * bytes, 256-byte aligned, laid out as gr_cacao_workspace_describe says: layers and mips tightly packed, mip k of an extent n is
 * max(1, n >> k).  Sampler models, rounding rules and store conversions: granite_amd/csrc/cacao_core.hpp, DESIGN.md 7.11.
 * Refused with GR_ERR_INVALID_ARGUMENT (a wrong image format alone: GR_ERR_UNSUPPORTED_FORMAT) before anything is launched: null
 * pointers, a workspace that is not 256-byte aligned, a width or height of 0 or above GR_CACAO_MAX_EXTENT, images that do not have the
 * size of the call, constants whose buffer dimensions are not those of width x height, and what each entry point names. */
#define GR_CACAO_QUALITY_HIGH 3u    /* FFX_CACAO_QUALITY_HIGH: shader level 2, 12 tap pairs */
#define GR_CACAO_QUALITY_HIGHEST 4u /* FFX_CACAO_QUALITY_HIGHEST: shader level 3, adaptive, 5 + 1 .. 32 tap pairs */
#define GR_CACAO_MAX_BLUR_PASSES 8u
#define GR_CACAO_MAX_EXTENT 16384u
#define GR_CACAO_FORMAT_R8G8B8A8_SNORM 38u /* VkFormat values of two intermediates that no gr_image argument takes */
#define GR_CACAO_FORMAT_R32_UINT 98u
typedef struct gr_cacao_settings /* FFX_CACAO_Settings, ffx_cacao.h:52-70 */
{
	float radius;
	float shadow_multiplier;
	float shadow_power;
	float shadow_clamp;
	float horizon_angle_threshold;
	float fade_out_from;
	float fade_out_to;
	uint32_t quality_level; /* GR_CACAO_QUALITY_* */
	float adaptive_quality_limit;
	uint32_t blur_pass_count;
	float sharpness;
	float temporal_supersampling_angle_offset;  /* unused, as in the reference */
	float temporal_supersampling_radius_offset; /* unused, as in the reference */
	float detail_shadow_strength;
	uint32_t generate_normals; /* must be 0 */
	float bilateral_sigma_squared;
	float bilateral_similarity_distance_sigma;
} gr_cacao_settings;
typedef struct gr_cacao_constants /* FFX_CACAO_Constants, ffx_cacao.h:95-154 = ffx_cacao_bindings.hlsl:27-87 */
{
	float DepthUnpackConsts[2];
	float CameraTanHalfFOV[2];
	float NDCToViewMul[2];
	float NDCToViewAdd[2];
	float DepthBufferUVToViewMul[2];
	float DepthBufferUVToViewAdd[2];
	float EffectRadius;
	float EffectShadowStrength;
	float EffectShadowPow;
	float EffectShadowClamp;
	float EffectFadeOutMul;
	float EffectFadeOutAdd;
	float EffectHorizonAngleThreshold;
	float EffectSamplingRadiusNearLimitRec;
	float DepthPrecisionOffsetMod;
	float NegRecEffectRadius;
	float LoadCounterAvgDiv;
	float AdaptiveSampleCountLimit;
	float InvSharpness;
	int32_t PassIndex;
	float BilateralSigmaSquared;
	float BilateralSimilarityDistanceSigma;
	float PatternRotScaleMatrices[5][4];
	float NormalsUnpackMul;
	float NormalsUnpackAdd;
	float DetailAOStrength;
	float Dummy0;
	float SSAOBufferDimensions[2];
	float SSAOBufferInverseDimensions[2];
	float DepthBufferDimensions[2];
	float DepthBufferInverseDimensions[2];
	int32_t DepthBufferOffset[2];
	float PerPassFullResUVOffset[2];
	float InputOutputBufferDimensions[2];
	float InputOutputBufferInverseDimensions[2];
	float ImportanceMapDimensions[2];
	float ImportanceMapInverseDimensions[2];
	float DeinterleavedDepthBufferDimensions[2];
	float DeinterleavedDepthBufferInverseDimensions[2];
	float DeinterleavedDepthBufferOffset[2];
	float DeinterleavedDepthBufferNormalisedOffset[2];
	float NormalsWorldToViewspaceMatrix[4][4];
} gr_cacao_constants;
typedef struct gr_cacao_buffer_sizes /* FFX_CACAO_BufferSizeInfo, ffx_cacao.h:159-183 */
{
	uint32_t inputOutputBufferWidth, inputOutputBufferHeight;
	uint32_t ssaoBufferWidth, ssaoBufferHeight;
	uint32_t depthBufferXOffset, depthBufferYOffset;
	uint32_t depthBufferWidth, depthBufferHeight;
	uint32_t deinterleavedDepthBufferXOffset, deinterleavedDepthBufferYOffset;
	uint32_t deinterleavedDepthBufferWidth, deinterleavedDepthBufferHeight;
	uint32_t importanceMapWidth, importanceMapHeight;
	uint32_t downsampledSsaoBufferWidth, downsampledSsaoBufferHeight;
} gr_cacao_buffer_sizes;
typedef struct gr_cacao_intermediate
{
	char name[32];          /* the reference's texture name (ffx_cacao_impl.cpp:71-79) */
	uint32_t format;        /* gr_format or GR_CACAO_FORMAT_* */
	uint32_t width, height; /* of mip 0 */
	uint32_t layers, mips;
	uint64_t mip_offset[4]; /* bytes from the workspace's start to layer 0 of mip k; layer l follows at l * mip width * mip height * texel size */
	uint64_t bytes;
} gr_cacao_intermediate;
#define GR_CACAO_INTERMEDIATE_COUNT 7u
/* Host-only.  The settings setup_ffx_cacao installs (renderer/post/ssao.cpp:73-91). */
void gr_cacao_reference_settings(gr_cacao_settings *settings);
/* Host-only.  FFX_CACAO_UpdateBufferSizeInfo with useDownsampledSsao = false. */
int gr_cacao_update_buffer_sizes(uint32_t width, uint32_t height, gr_cacao_buffer_sizes *sizes);
/* Host-only.  FFX_CACAO_UpdateConstants + FFX_CACAO_UpdatePerPassConstants for the four passes (ffx_cacao.cpp:108-269).  proj and
 * normals_to_view are column-major 4x4 matrices in memory, RenderParameters::projection and ::view.  ctx may be NULL (it only receives the
 * message).  Refused: generate_normals != 0, a quality_level other than GR_CACAO_QUALITY_HIGH / HIGHEST, blur_pass_count above 8. */
int gr_cacao_update_constants(gr_ctx *ctx, gr_cacao_constants constants[4], const gr_cacao_settings *settings, const gr_cacao_buffer_sizes *sizes,
                              const float proj[16], const float normals_to_view[16]);
/* Host-only.  0 for a width or height of 0 or above GR_CACAO_MAX_EXTENT. */
size_t gr_cacao_workspace_bytes(uint32_t width, uint32_t height);
/* Host-only.  Fills out[0 .. GR_CACAO_INTERMEDIATE_COUNT): deinterleaved depths (R16_SFLOAT, 4 layers, 4 mips), deinterleaved normals
 * (R8G8B8A8_SNORM, 4 layers), SSAO ping and pong (R8G8_UNORM, 4 layers), importance map and its pong (R8_UNORM), load counter (R32_UINT). */
int gr_cacao_workspace_describe(uint32_t width, uint32_t height, gr_cacao_intermediate *out, uint32_t capacity);
/* ClearLoadCounter + PrepareNativeDepthsAndMips: depth D32_SFLOAT width x height. */
int gr_cacao_prepare_depths(gr_ctx *ctx, gr_stream stream, const gr_image *depth, void *workspace, const gr_cacao_constants *constants);
/* PrepareNativeNormalsFromInputNormals: normal A2B10G10R10_UNORM_PACK32 width x height.  A texel past an odd extent reads as zero. */
int gr_cacao_prepare_normals(gr_ctx *ctx, gr_stream stream, const gr_image *normal, void *workspace, const gr_cacao_constants *constants);
/* GenerateQ3Base x 4: depths and normals -> SSAO pong (obscurance, weight / 20). */
int gr_cacao_generate_base(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants constants[4]);
/* GenerateImportanceMap (pong -> importance), PostprocessImportanceMapA (importance -> its pong), PostprocessImportanceMapB (-> importance,
 * and the load counter: integer atomic adds of every texel with x % 3 + y % 3 == 0). */
int gr_cacao_importance_generate(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants);
int gr_cacao_importance_postprocess_a(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants);
int gr_cacao_importance_postprocess_b(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants);
/* GenerateQ2 x 4 (quality GR_CACAO_QUALITY_HIGH) or GenerateQ3 x 4 (HIGHEST; reads pong, importance and the load counter) -> SSAO ping
 * (occlusion, packed edges).  Any other quality is refused. */
int gr_cacao_generate(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants constants[4], uint32_t quality);
/* EdgeSensitiveBlur<blur_passes> x 4: ping -> pong.  blur_passes 1 .. 8; 0 has no dispatch and is refused. */
int gr_cacao_blur(gr_ctx *ctx, gr_stream stream, void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *constants, uint32_t blur_passes);
/* Apply: SSAO pong (from_pong != 0: after a blur) or ping -> out, R8_UNORM width x height. */
int gr_cacao_apply(gr_ctx *ctx, gr_stream stream, const void *workspace, const gr_image *out, const gr_cacao_constants *constants, uint32_t from_pong);

/* Fill with a 32-bit pattern (count dwords): attachment clears to a colour. */
int gr_fill_u32(gr_ctx *ctx, gr_stream stream, void *dst, uint32_t value, size_t count);
/* Executor self-test operation (no counterpart in the reference): out[i] = hash(i, salt, one dword of each of up to four
 * inputs).  Used by tests/cpp/graph_cases.cpp --execute to run random frame graphs on the executor's streams and compare the
 * swapchain image with a serial run. */
/* fp32 (r, g, b) triples -> B10G11R11_UFLOAT_PACK32 words: the attachment store conversion the lighting and TAA kernels apply
 * when their target has that format (closest finite packed value, ties to even; negative -> 0; +inf -> +inf; NaN -> NaN). */
int gr_pack_b10g11r11(gr_ctx *ctx, gr_stream stream, const float *rgb, uint32_t *out, uint32_t texels);
int gr_debug_mix(gr_ctx *ctx, gr_stream stream, void *out, size_t out_dwords, const void *const *inputs, const size_t *input_dwords,
                 uint32_t input_count, uint32_t salt);
/* VkPhysicalDeviceProperties::deviceName / driverVersion as the headless runner reports them in its --stat file
 * (application_headless.cpp:634-635): HIP device name and hipDriverGetVersion. */
int gr_get_device_info(gr_ctx *ctx, char *name, size_t name_capacity, uint32_t *driver_version);

/* ---- layout contracts, checked where the structs are declared: the push-constant blocks and the
 * cluster UBO are byte-identical to what the reference's host code pushes and its shaders declare. ------------------------------------ */
#include <stddef.h>
#ifdef __cplusplus
#define GR_STATIC_ASSERT(cond, what) static_assert(cond, what)
#else
#define GR_STATIC_ASSERT(cond, what) _Static_assert(cond, what)
#endif
#define GR_ASSERT_SIZE(type, bytes) GR_STATIC_ASSERT(sizeof(type) == (bytes), #type ": size differs from the reference's block")
#define GR_ASSERT_OFFSET(type, member, bytes) GR_STATIC_ASSERT(offsetof(type, member) == (bytes), #type "." #member ": offset differs from the reference's block")
GR_ASSERT_SIZE(gr_luminance_data, 12);        /* luminance.comp:4-9 */
GR_ASSERT_SIZE(gr_push_luminance, 20);        /* hdr.cpp:85-96 */
GR_ASSERT_OFFSET(gr_push_luminance, lerp, 8);
GR_ASSERT_OFFSET(gr_push_luminance, min_loglum, 12);
GR_ASSERT_OFFSET(gr_push_luminance, max_loglum, 16);
GR_ASSERT_SIZE(gr_push_bloom_threshold, 16);  /* hdr.cpp:133-142 */
GR_ASSERT_OFFSET(gr_push_bloom_threshold, inv_output_size, 8);
GR_ASSERT_SIZE(gr_push_bloom_downsample, 28); /* hdr.cpp:169-185 */
GR_ASSERT_OFFSET(gr_push_bloom_downsample, inv_output_size, 8);
GR_ASSERT_OFFSET(gr_push_bloom_downsample, inv_input_size, 16);
GR_ASSERT_OFFSET(gr_push_bloom_downsample, lerp, 24);
GR_ASSERT_SIZE(gr_push_bloom_upsample, 24);   /* hdr.cpp:202-214 */
GR_ASSERT_OFFSET(gr_push_bloom_upsample, inv_input_size, 16);
GR_ASSERT_SIZE(gr_push_tonemap, 4);           /* hdr.cpp:297-302 */
GR_ASSERT_SIZE(gr_push_fxaa, 8);              /* fxaa.cpp:45-47 */
GR_ASSERT_SIZE(gr_push_smaa, 16);             /* smaa.cpp:129-133 */
GR_ASSERT_SIZE(gr_push_taa, 80);              /* temporal.cpp:232-250 */
GR_ASSERT_OFFSET(gr_push_taa, rt_metrics, 64);
GR_ASSERT_SIZE(gr_push_clustering, 48);       /* renderer.cpp:1110-1121: 40 B used, 48 in C++ */
GR_ASSERT_OFFSET(gr_push_clustering, camera_pos, 16);
GR_ASSERT_OFFSET(gr_push_clustering, inv_resolution, 32);
GR_ASSERT_SIZE(gr_push_directional, 96);      /* renderer.cpp:1073-1103: 88 B used */
GR_ASSERT_OFFSET(gr_push_directional, color, 16);
GR_ASSERT_OFFSET(gr_push_directional, environment_intensity, 28);
GR_ASSERT_OFFSET(gr_push_directional, camera_pos, 32);
GR_ASSERT_OFFSET(gr_push_directional, environment_mipscale, 44);
GR_ASSERT_OFFSET(gr_push_directional, direction, 48);
GR_ASSERT_OFFSET(gr_push_directional, cascade_log_bias, 60);
GR_ASSERT_OFFSET(gr_push_directional, camera_front, 64);
GR_ASSERT_OFFSET(gr_push_directional, inv_resolution, 80);
GR_ASSERT_SIZE(gr_push_spot_transform, 100);  /* clusterer.cpp:1477-1493 */
GR_ASSERT_OFFSET(gr_push_spot_transform, camera_pos, 64);
GR_ASSERT_OFFSET(gr_push_spot_transform, num_lights, 76);
GR_ASSERT_OFFSET(gr_push_spot_transform, camera_front, 80);
GR_ASSERT_OFFSET(gr_push_spot_transform, z_near, 92);
GR_ASSERT_OFFSET(gr_push_spot_transform, z_far, 96);
GR_ASSERT_SIZE(gr_push_cluster_setup, 68);    /* clusterer.cpp:1502-1509 */
GR_ASSERT_OFFSET(gr_push_cluster_setup, num_lights, 64);
GR_ASSERT_SIZE(gr_push_z_range, 12);          /* clusterer.cpp:1291-1300 */
GR_ASSERT_SIZE(gr_light_info, 48);            /* light_info.hpp:35-44 */
GR_ASSERT_OFFSET(gr_light_info, spot_scale_bias, 12);
GR_ASSERT_OFFSET(gr_light_info, position, 16);
GR_ASSERT_OFFSET(gr_light_info, offset_radius, 28);
GR_ASSERT_OFFSET(gr_light_info, direction, 32);
GR_ASSERT_OFFSET(gr_light_info, inv_radius, 44);
GR_ASSERT_SIZE(gr_mat_affine, 48);            /* muglm.hpp:899-958 */
GR_ASSERT_SIZE(gr_cluster_params, 176);       /* clusterer_data.h:20-39, std140 */
GR_ASSERT_OFFSET(gr_cluster_params, clip_scale, 64);
GR_ASSERT_OFFSET(gr_cluster_params, camera_base, 80);
GR_ASSERT_OFFSET(gr_cluster_params, camera_front, 96);
GR_ASSERT_OFFSET(gr_cluster_params, xy_scale, 112);
GR_ASSERT_OFFSET(gr_cluster_params, resolution_xy, 120);
GR_ASSERT_OFFSET(gr_cluster_params, inv_resolution_xy, 128);
GR_ASSERT_OFFSET(gr_cluster_params, num_lights, 136);
GR_ASSERT_OFFSET(gr_cluster_params, num_lights_32, 140);
GR_ASSERT_OFFSET(gr_cluster_params, num_decals, 144);
GR_ASSERT_OFFSET(gr_cluster_params, decals_texture_offset, 152);
GR_ASSERT_OFFSET(gr_cluster_params, z_max_index, 156);
GR_ASSERT_OFFSET(gr_cluster_params, z_scale, 160);
GR_ASSERT_SIZE(gr_push_pq10, 80);             /* hdr.cpp:626-633 */
GR_ASSERT_SIZE(gr_push_video, 28);            /* scaler.comp:78-84, scaler.cpp:184-190 */
GR_ASSERT_OFFSET(gr_push_video, dither_strength, 24);
GR_ASSERT_SIZE(gr_push_yuv_to_rgb, 164);      /* yuv_to_rgb.comp:9-18, ffmpeg_decode.cpp:588-598 */
GR_ASSERT_OFFSET(gr_push_yuv_to_rgb, primary_conversion, 64);
GR_ASSERT_OFFSET(gr_push_yuv_to_rgb, resolution, 128);
GR_ASSERT_OFFSET(gr_push_yuv_to_rgb, inv_resolution, 136);
GR_ASSERT_OFFSET(gr_push_yuv_to_rgb, chroma_siting, 144);
GR_ASSERT_OFFSET(gr_push_yuv_to_rgb, chroma_clamp, 152);
GR_ASSERT_OFFSET(gr_push_yuv_to_rgb, unorm_rescale, 160);
GR_ASSERT_SIZE(gr_push_ocean_generate, 28);   /* generate_fft.comp:23-30, ocean.cpp:421-428 */
GR_ASSERT_OFFSET(gr_push_ocean_generate, N, 8);
GR_ASSERT_OFFSET(gr_push_ocean_generate, freq_to_band_mod, 16);
GR_ASSERT_OFFSET(gr_push_ocean_generate, time, 20);
GR_ASSERT_OFFSET(gr_push_ocean_generate, period, 24);
GR_ASSERT_SIZE(gr_push_ocean_bake, 32);       /* bake_maps.comp:4-8, ocean.cpp:519-523 */
GR_ASSERT_OFFSET(gr_push_ocean_bake, scale, 16);
GR_ASSERT_SIZE(gr_push_ocean_mipmap, 36);     /* mipmap.comp:17-23, ocean.cpp:553-559 */
GR_ASSERT_OFFSET(gr_push_ocean_mipmap, inv_resolution, 16);
GR_ASSERT_OFFSET(gr_push_ocean_mipmap, count, 24);
GR_ASSERT_OFFSET(gr_push_ocean_mipmap, lod, 32);
GR_ASSERT_SIZE(gr_push_ocean_update_lod, 64); /* update_lod.comp:6-15, ocean.cpp:285-294 */
GR_ASSERT_OFFSET(gr_push_ocean_update_lod, max_lod, 12);
GR_ASSERT_OFFSET(gr_push_ocean_update_lod, image_offset, 16);
GR_ASSERT_OFFSET(gr_push_ocean_update_lod, num_threads, 24);
GR_ASSERT_OFFSET(gr_push_ocean_update_lod, grid_base, 32);
GR_ASSERT_OFFSET(gr_push_ocean_update_lod, grid_size, 40);
GR_ASSERT_OFFSET(gr_push_ocean_update_lod, lod_bias, 48);
GR_ASSERT_SIZE(gr_push_ocean_cull, 96);       /* cull_blocks.comp:6-20, ocean.cpp:335-349 */
GR_ASSERT_OFFSET(gr_push_ocean_cull, image_offset, 16);
GR_ASSERT_OFFSET(gr_push_ocean_cull, num_threads, 24);
GR_ASSERT_OFFSET(gr_push_ocean_cull, inv_num_threads, 32);
GR_ASSERT_OFFSET(gr_push_ocean_cull, grid_base, 40);
GR_ASSERT_OFFSET(gr_push_ocean_cull, grid_size, 48);
GR_ASSERT_OFFSET(gr_push_ocean_cull, grid_resolution, 56);
GR_ASSERT_OFFSET(gr_push_ocean_cull, heightmap_range, 64);
GR_ASSERT_OFFSET(gr_push_ocean_cull, guard_band, 72);
GR_ASSERT_OFFSET(gr_push_ocean_cull, lod_stride, 76);
GR_ASSERT_OFFSET(gr_push_ocean_cull, max_lod, 80);
GR_ASSERT_OFFSET(gr_push_ocean_cull, handle_edge_lods, 84);
GR_ASSERT_SIZE(gr_ocean_patch, 32);           /* ocean.inc:4-10 */
GR_ASSERT_OFFSET(gr_ocean_patch, lods, 16);
GR_ASSERT_SIZE(gr_ocean_indirect_draw, 32);   /* ocean.inc:12-22 */
GR_ASSERT_OFFSET(gr_ocean_indirect_draw, instance_count, 4);
GR_ASSERT_SIZE(gr_push_meshlet_decode, 16);   /* meshlet_decode.comp:77-83, meshlet.cpp:247-253 */
GR_ASSERT_OFFSET(gr_push_meshlet_decode, meshlet_count, 8);
GR_ASSERT_OFFSET(gr_push_meshlet_decode, wg_offset, 12);
GR_ASSERT_SIZE(gr_meshlet_stream, 16);        /* meshlet.hpp:47-57 */
GR_ASSERT_OFFSET(gr_meshlet_stream, bits, 8);
GR_ASSERT_SIZE(gr_meshlet_offsets, 12);       /* meshlet.cpp:209-214 */
GR_ASSERT_SIZE(gr_push_meshlet_cull, 16);     /* meshlet_cull.comp:23-29 */
GR_ASSERT_OFFSET(gr_push_meshlet_cull, mdi_count_offset, 8);
GR_ASSERT_OFFSET(gr_push_meshlet_cull, draw_indirect_offset, 12);
GR_ASSERT_SIZE(gr_meshlet_task, 20);          /* inc/meshlet_render_types.h:15-22 */
GR_ASSERT_OFFSET(gr_meshlet_task, mesh_index_count, 12);
GR_ASSERT_SIZE(gr_meshlet_aabb, 32);          /* inc/meshlet_render_types.h:4-7 */
GR_ASSERT_OFFSET(gr_meshlet_aabb, hi, 16);
GR_ASSERT_SIZE(gr_meshlet_bound, 32);         /* vulkan/mesh/meshlet.hpp:79-84 */
GR_ASSERT_OFFSET(gr_meshlet_bound, cone_axis_cutoff, 16);
GR_ASSERT_SIZE(gr_meshlet_draw, 12);          /* vulkan/mesh/meshlet.hpp:72-77 */
GR_ASSERT_OFFSET(gr_meshlet_draw, vertex_offset, 8);
GR_ASSERT_SIZE(gr_meshlet_frustum, 224);      /* inc/meshlet_ubos.h:4-14, std140 */
GR_ASSERT_OFFSET(gr_meshlet_frustum, viewport, 0);
GR_ASSERT_OFFSET(gr_meshlet_frustum, planes, 16);
GR_ASSERT_OFFSET(gr_meshlet_frustum, view, 112);
GR_ASSERT_OFFSET(gr_meshlet_frustum, viewport_scale_bias, 176);
GR_ASSERT_OFFSET(gr_meshlet_frustum, hiz_resolution, 192);
GR_ASSERT_OFFSET(gr_meshlet_frustum, winding, 200);
GR_ASSERT_OFFSET(gr_meshlet_frustum, hiz_min_lod, 204);
GR_ASSERT_OFFSET(gr_meshlet_frustum, hiz_max_lod, 208);
GR_ASSERT_SIZE(gr_cacao_constants, 384);      /* ffx_cacao.h:95-154, ffx_cacao_bindings.hlsl:27-87 */
GR_ASSERT_OFFSET(gr_cacao_constants, EffectRadius, 48);
GR_ASSERT_OFFSET(gr_cacao_constants, InvSharpness, 96);
GR_ASSERT_OFFSET(gr_cacao_constants, PassIndex, 100);
GR_ASSERT_OFFSET(gr_cacao_constants, PatternRotScaleMatrices, 112);
GR_ASSERT_OFFSET(gr_cacao_constants, NormalsUnpackMul, 192);
GR_ASSERT_OFFSET(gr_cacao_constants, SSAOBufferDimensions, 208);
GR_ASSERT_OFFSET(gr_cacao_constants, DepthBufferOffset, 240);
GR_ASSERT_OFFSET(gr_cacao_constants, PerPassFullResUVOffset, 248);
GR_ASSERT_OFFSET(gr_cacao_constants, InputOutputBufferDimensions, 256);
GR_ASSERT_OFFSET(gr_cacao_constants, ImportanceMapDimensions, 272);
GR_ASSERT_OFFSET(gr_cacao_constants, DeinterleavedDepthBufferDimensions, 288);
GR_ASSERT_OFFSET(gr_cacao_constants, DeinterleavedDepthBufferNormalisedOffset, 312);
GR_ASSERT_OFFSET(gr_cacao_constants, NormalsWorldToViewspaceMatrix, 320);
GR_ASSERT_SIZE(gr_cacao_settings, 68);        /* ffx_cacao.h:52-70 */
GR_ASSERT_OFFSET(gr_cacao_settings, quality_level, 28);
GR_ASSERT_OFFSET(gr_cacao_settings, generate_normals, 56);
GR_ASSERT_SIZE(gr_cacao_buffer_sizes, 64);    /* ffx_cacao.h:159-183 */
GR_ASSERT_SIZE(gr_decal_texture, 24);
GR_ASSERT_OFFSET(gr_decal_texture, width, 8);
GR_ASSERT_OFFSET(gr_decal_texture, format, 20);
GR_ASSERT_SIZE(gr_decal_apply_args, 328);
GR_ASSERT_OFFSET(gr_decal_apply_args, depth, 24);
GR_ASSERT_OFFSET(gr_decal_apply_args, inv_view_projection, 48);
GR_ASSERT_OFFSET(gr_decal_apply_args, cluster, 112);
GR_ASSERT_OFFSET(gr_decal_apply_args, transforms, 288);
GR_ASSERT_OFFSET(gr_decal_apply_args, bitmask_decal, 296);
GR_ASSERT_OFFSET(gr_decal_apply_args, range_decal, 304);
GR_ASSERT_OFFSET(gr_decal_apply_args, textures, 312);
GR_ASSERT_OFFSET(gr_decal_apply_args, num_textures, 320);
GR_ASSERT_SIZE(gr_sky_args, 160);
GR_ASSERT_OFFSET(gr_sky_args, depth, 24);
GR_ASSERT_OFFSET(gr_sky_args, inv_local_view_projection, 48);
GR_ASSERT_OFFSET(gr_sky_args, color, 112);
GR_ASSERT_OFFSET(gr_sky_args, camera_height, 124);
GR_ASSERT_OFFSET(gr_sky_args, sun_direction, 128);
GR_ASSERT_OFFSET(gr_sky_args, cube, 144);
GR_ASSERT_SIZE(gr_sky_cube_params, 32); /* volumetric_light_setup_sky.comp's UBO */
GR_ASSERT_OFFSET(gr_sky_cube_params, camera_y, 12);
GR_ASSERT_OFFSET(gr_sky_cube_params, sun_direction, 16);
GR_ASSERT_SIZE(gr_directional_light_args, 696);
GR_ASSERT_OFFSET(gr_directional_light_args, inv_view_projection, 144);
GR_ASSERT_OFFSET(gr_directional_light_args, directional, 208);
GR_ASSERT_OFFSET(gr_directional_light_args, flags, 304);
GR_ASSERT_OFFSET(gr_directional_light_args, layers, 312);
GR_ASSERT_OFFSET(gr_directional_light_args, ambient_occlusion, 320);
GR_ASSERT_OFFSET(gr_directional_light_args, shadow_maps, 344);
GR_ASSERT_OFFSET(gr_directional_light_args, transforms, 440);
GR_STATIC_ASSERT(GR_TRANSFORMS_OFFSET_SHADOW ==GR_MAX_LIGHTS_BINDLESS * 48u, "ClustererBindlessTransforms: lights[4096] of 48 B");
GR_STATIC_ASSERT(GR_TRANSFORMS_OFFSET_MODEL + GR_MAX_LIGHTS_BINDLESS * 48u == GR_TRANSFORMS_OFFSET_TYPE_MASK, "ClustererBindlessTransforms: model[4096] of 48 B");
GR_STATIC_ASSERT(GR_TRANSFORMS_OFFSET_TYPE_MASK + GR_MAX_LIGHTS_BINDLESS / 8u == GR_TRANSFORMS_OFFSET_DECALS, "ClustererBindlessTransforms: type_mask[128]");
#undef GR_ASSERT_SIZE
#undef GR_ASSERT_OFFSET

#ifdef __cplusplus
}
#endif
#endif
