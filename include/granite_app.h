/* granite_app.h — C ABI of the headless harness that composes Granite's image-space graph on the HIP executor.
 *
 * Mirrors what application/scene_viewer_application.cpp:876-991,1167-1318 (graph composition) and
 * application/platforms/application_headless.cpp:581-671 (warm-up, timed loop, readback) do for the reference, with the
 * scene/mesh renderer replaced by synthetic G-buffer uploads.  Used by bench.py and the parity tests (ctypes); a
 * Granite application would call the C++ classes in granite_amd/csrc/host directly.
 */
#ifndef GRANITE_APP_H_
#define GRANITE_APP_H_

#include <stddef.h>
#include <stdint.h>
#include "granite_hip.h" /* gr_video_yuv_info */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gra_app gra_app;

/* PostAAType (renderer/post/aa.hpp:33-47) subset that is live in the reference. */
typedef enum gra_post_aa
{
	GRA_POST_AA_NONE = 0,
	GRA_POST_AA_FXAA = 1,
	GRA_POST_AA_SMAA_LOW = 2,
	GRA_POST_AA_SMAA_MEDIUM = 3,
	GRA_POST_AA_SMAA_HIGH = 4,
	GRA_POST_AA_SMAA_ULTRA = 5,
	GRA_POST_AA_TAA_LOW = 6,
	GRA_POST_AA_TAA_MEDIUM = 7,
	GRA_POST_AA_TAA_HIGH = 8
} gra_post_aa;

typedef struct gra_config
{
	int32_t device;            /* HIP device index */
	uint32_t width, height;    /* backbuffer = R8G8B8A8_SRGB width x height (application_headless.cpp:207-229) */
	int32_t enable_lighting;   /* 0: config-1 style graph (HDR input -> bloom -> tonemap); 1: gbuffer + clustering + lighting */
	int32_t hdr_bloom;         /* viewer_config "hdrBloom" */
	int32_t dynamic_exposure;  /* "hdrBloomDynamicExposure" */
	int32_t compute_post;      /* ImplementationQuirks::use_async_compute_post: 1 = setup_hdr_postprocess_compute */
	int32_t post_aa;           /* gra_post_aa applied after the post chain (fxaa / smaa) */
	int32_t pre_aa;            /* gra_post_aa applied before the post chain (taa) */
	int32_t rmw_emissive;      /* 1: lighting declared add_color_output("HDR", info, "emissive") exactly like the reference
	                              (G-buffer emissive restored every frame); 0: emissive is a 5th attachment input */
	uint32_t cluster_res[3];   /* LightClusterer::set_resolution; viewer default 128 x 64 x 4096 */
	float frame_time;          /* FrameParameters::frame_time fed to the lerps; headless default 0.01 */
	float directional_color[3];
	float directional_direction[3];
	int32_t enable_timestamps; /* RenderGraph::enable_timestamps */
	/* Row-band tiling of the frame across executors: this instance is rank strip_index of strip_count.
	 * 0 / 1 = the whole frame here.  Needs enable_lighting, hdr_bloom, compute_post and no AA; the band exchanges go
	 * through gra_set_exchange_callback. */
	uint32_t strip_index, strip_count;
	/* 0 (reference behaviour): attachment images of identical geometry with disjoint lifetimes inside the frame share
	 * one allocation (RenderGraph::build_aliases, render_graph.cpp:1548-1746); 1: every image gets its own. */
	int32_t disable_image_aliasing;
	/* Depth hierarchy of the frame's depth attachment (setup_depth_hierarchy_pass, renderer/post/spd.cpp:196-232), resource
	 * "depth-hiz": 0 = none, 1 = full chain, 2 = output_downsample (no full-resolution level).  Needs enable_lighting.
	 * The pass is tied to the end of the frame through a proxy resource, as its consumers (occlusion culling, SSR) live
	 * outside this build. */
	int32_t depth_hierarchy;
	/* viewer_config "resolutionScale" / "resolutionScaleSharpen" (scene_viewer_application.cpp:248-250,758-761,1263-1268):
	 * with 0 < resolution_scale < 1 the G-buffer, lighting, post chain and AA run at ceil(size * scale) and
	 * setup_after_post_chain_upscaling (FSR 1.0 EASU, + RCAS when resolution_scale_sharpen) brings the result to the
	 * backbuffer size; uploads are then render-sized.  0 or 1 = off.  fsr_fp32 = 1 forces the FP16 = 0 shader variant. */
	float resolution_scale;
	int32_t resolution_scale_sharpen;
	int32_t fsr_fp32;
	/* viewer_config "ssao" on the deferred path (scene_viewer_application.cpp:950-980,1571): the lighting pass takes the
	 * R8_UNORM texture "ssao-output-main" as LightingParameters::ambient_occlusion.  Its producer in Granite is FidelityFX CACAO
	 * (setup_ffx_cacao).  GRA_AMBIENT_OCCLUSION_UPLOAD (1): the pass "ssao-main" fills the texture from
	 * gra_upload_ambient_occlusion like the G-buffer (white until an image arrives).  GRA_AMBIENT_OCCLUSION_CACAO (2): "ssao-main" computes
	 * it from the G-buffer's depth and normals every frame (host/post/ssao.cpp, csrc/cacao.hip) with the reference's settings; an upload
	 * is refused, and so are row bands (strip_count > 1). */
	int32_t ambient_occlusion;
#define GRA_AMBIENT_OCCLUSION_UPLOAD 1
#define GRA_AMBIENT_OCCLUSION_CACAO 2
	/* HDR10 output (setup_hdr10_pq_encoding, renderer/post/hdr.cpp:595-658): the backbuffer is A2B10G10R10_UNORM_PACK32 and the
	 * frame ends lighting -> "ui" (an R8G8B8A8_SRGB layer cleared to transparent: (0, 0, 0, 1) = scene fully visible) -> "pq10"
	 * with ST.2020 primaries, maxContentLightLevel 1000, hdr / ui pre-exposure 500 / 400 (scene_viewer_application.cpp:1283-1285).
	 * Replaces bloom + tonemap (hdr_bloom must be 0); no AA, no resolution scaling, no row bands.  Note: the viewer itself
	 * declares the UI layer as a colour read-modify-write of the HDR target with another format, which its own validation
	 * rejects (scene_viewer_application.cpp:1279-1287); the layer is its own attachment here. */
	int32_t hdr10;
	/* viewer_config "ssr" on the deferred path (scene_viewer_application.cpp:1206-1212): setup_ssr_pass between lighting and
	 * the post chain -- depth hierarchy "depth-transient-main-hier", "SSR-trace" (classify + trace), "SSR" (apply, blended into
	 * the lit target).  Needs enable_lighting and gra_install_ssr_tables before the first frame. */
	int32_t ssr;
	/* The frame graph of Granite's AA benchmark (tools/aa_bench.cpp:65-161) instead of the viewer's: "main" blits one of two
	 * input images (alternating per frame, gra_upload_aa_bench_images) into "HDR-main" with LinearClamp and clears "depth-main",
	 * pre_aa (TAA) resolves it, "tonemap" blits the result into a swapchain-sized target with NearestClamp, post_aa (FXAA /
	 * SMAA) follows, and with 0 < resolution_scale < 1 FSR 1.0 (+ sharpen) ends the frame.  Identity camera matrices feed the
	 * temporal jitter (aa_bench.cpp:52), timestamps are on.  enable_lighting and hdr_bloom must be 0. */
	int32_t aa_bench;
	/* Row bands: the finished frame's bands meet in every rank's output image as RGB888 (packed before, unpacked after the
	 * all-gather; the alpha byte of a tonemapped / FXAA'd frame is 255) -- 3/4 of the bytes per xGMI link.  1 = send the RGBA8 rows
	 * as they are (A/B).  An SMAA output always travels as RGBA8. */
	int32_t output_gather_rgba;
	/* viewer_config "renderTargetFp16" = false, the reference's shipped default (viewer/viewer_config.json:15,
	 * scene_viewer_application.cpp:881-883): emissive / HDR-main are B10G11R11_UFLOAT_PACK32 instead of R16G16B16A16_SFLOAT
	 * (4 bytes per texel; both lighting blends round to the packed floats), and a TAA resolve in front of the post chain writes
	 * its colour in the same format (temporal.cpp:211-213; its history stays RGBA16F).  The emissive upload is then one
	 * 32-bit word per texel.  0 = RGBA16F everywhere (SURVEY.md 8d fixes the headline configuration on it).  Not with ssr / hdr10
	 * (those passes read-modify-write the lit target as RGBA16F here). */
	int32_t hdr_packed_float;
	/* Row bands with a TAA resolve (no reference analogue): > 0 = how many rows a resolved pixel's history fetch may
	 * lie away from the pixel (vertical motion in rows + 3 for the Catmull-Rom footprint).  The history bands then only exchange
	 * their boundary rows with their neighbours (gra_get_strip_plan_taa_history says how many) instead of meeting whole in every
	 * rank.  A frame in which some pixel reaches further is NOT the single-device frame: the resolve notices (gr_taa_resolve_band),
	 * and the next gra_render_frame / gra_sync / read-back fails with an error that says so.  0 = whole bands are all-gathered
	 * (any motion).  Every rank must be given the same value. */
	uint32_t taa_history_reach_rows;
	/* Volumetric decals (lights/volumetric_decal.h): the clusterer also bins the decals of gra_set_decals, and the G-buffer pass applies them
	 * to base colour, from the world position alone, before lighting reads it.  The pass then rewrites "albedo" from the uploaded image every
	 * frame, so decals do not accumulate.  Needs enable_lighting; not with strip_count > 1 or aa_bench.  0 = off: no graph, launch or byte
	 * changes. */
	int32_t volumetric_decals;
} gra_config;

/* Settings that came after gra_config's layout was fixed (its last member stays volumetric_decals): handed to gra_create_ext beside the
 * config.  struct_size is sizeof(gra_config_ext) as the caller was compiled; members beyond it read as 0, so the structure can grow.
 * sky -- the sky pass (Skybox, renderer/mesh_util.cpp:1046-1142): the G-buffer pass writes "emissive" where depth == 0, after the decals
 * and before lighting, and then rewrites "emissive" from the uploaded image every frame.  GRA_SKY_ATMOSPHERE: the procedural Rayleigh /
 * Mie atmosphere (the viewer's background for a scene without one), sun direction and colour those of gra_set_directional_light /
 * the config, camera height camera_position.y.  GRA_SKY_CUBE: the cube of gra_set_sky_cube times its colour; a frame rendered before a
 * cube is set fails with a message that says so.  Needs enable_lighting; not with strip_count > 1 or aa_bench.  0 = off: no graph,
 * launch or byte changes. */
typedef struct gra_config_ext
{
	uint32_t struct_size;
	int32_t sky;
} gra_config_ext;
#define GRA_SKY_OFF 0
#define GRA_SKY_ATMOSPHERE 1
#define GRA_SKY_CUBE 2

/* One volumetric decal: the world transform of its unit box and the texture (gra_set_decal_texture) it projects along its z axis. */
typedef struct gra_decal_desc
{
	float transform[12]; /* mat_affine rows */
	uint32_t texture;
} gra_decal_desc;

/* Scene-level light description (one PositionalLight + its node transform). */
typedef struct gra_light_desc
{
	int32_t type;            /* 0 = spot, 1 = point */
	float color[3];
	float inner_cone, outer_cone;
	float cutoff_range;      /* PositionalLight::set_maximum_range */
	float pad;
	float transform[12];     /* mat_affine rows */
} gra_light_desc;

/* RenderParameters subset, tightly packed: projection, view, view_projection, inv_projection, inv_view,
 * inv_view_projection (column-major mat4 each), camera_position[3], camera_front[3], z_near, z_far = 104 floats. */
#define GRA_RENDER_PARAMS_FLOATS 104

gra_app *gra_create(const gra_config *config, char *error, size_t error_size);
/* gra_create with the settings of gra_config_ext; ext == NULL is gra_create. */
gra_app *gra_create_ext(const gra_config *config, const gra_config_ext *ext, char *error, size_t error_size);
void gra_destroy(gra_app *app);
const char *gra_last_error(gra_app *app);

/* RenderContext::set_camera(projection, view): derives inverses etc. on the host like the reference. */
int gra_set_camera(gra_app *app, const float *projection16, const float *view16);
/* The eye moves by `translation` (world units) every frame, applied to the view matrix of gra_set_camera before each frame
 * (BASELINE config 4: "camera translates 0.01 units/frame" -- the TAA reprojection and the cluster build then really change from
 * frame to frame).  (0, 0, 0) = a static camera.  Needs gra_set_camera. */
int gra_set_camera_motion(gra_app *app, const float translation[3]);
/* Installs precomputed parameters verbatim (so that the CPU oracle and the device see bit-identical inputs). */
int gra_set_render_parameters(gra_app *app, const float *params104);
int gra_get_render_parameters(gra_app *app, float *params104);
/* Size the G-buffer is rendered (and uploaded) at: the backbuffer size unless resolution_scale is in use. */
int gra_get_render_size(gra_app *app, uint32_t *width, uint32_t *height);

int gra_set_lights(gra_app *app, const gra_light_desc *lights, uint32_t count);

/* Decals (config.volumetric_decals).  A texture is width x height RGBA8 texels (format: VK_FORMAT_R8G8B8A8_SRGB 43 or _UNORM 37) with
 * `levels` mip levels, level i = max(1, width >> i) x max(1, height >> i), tightly packed one after another in `texels` (host pointer).
 * Indices are dense: index may be an existing one (replaced) or the next free one.  gra_set_decals replaces the list; a decal that names a
 * texture that has not been set is refused, the message says which.  Beyond 4096 decals the farthest are dropped. */
int gra_set_decal_texture(gra_app *app, uint32_t index, uint32_t width, uint32_t height, uint32_t levels, uint32_t format, const void *texels);
int gra_set_decals(gra_app *app, const gra_decal_desc *decals, uint32_t count);
/* The sky's cube (gra_config_ext.sky == GRA_SKY_CUBE): an R16G16B16A16_SFLOAT chain of `levels` levels in the gr_env_* layout (host pointer,
 * gr_cube_chain_bytes(size, levels) bytes), and the colour it is multiplied by.  The _gtx form takes a cube .gtx as gra_environment_bake
 * writes it (6 layers, square, R16G16B16A16_SFLOAT, any number of levels of its chain). */
int gra_set_sky_cube(gra_app *app, uint32_t size, uint32_t levels, const void *rgba16f_chain, const float color[3]);
int gra_set_sky_cube_gtx(gra_app *app, const char *cube_gtx, const float color[3]);
/* What the next frame's sky would be drawn with: RenderParameters::local_view_projection and its inverse (column-major), and the Skybox's
 * push values (a cube: its colour, 0, 0; none: the directional light's colour, camera_position.y, the light's direction).  Any pointer
 * may be NULL.  Needs no device. */
int gra_get_sky_state(gra_app *app, float local_view_projection16[16], float inv_local_view_projection16[16], float color[3], float *camera_height,
                      float direction[3]);
/* CPU-side state of the last refresh, decals in sorted order: order[i] = index into the gra_set_decals list, 12 floats of world_to_texture,
 * 16 of the mvp and the two slice-interval words per decal.  Any pointer may be NULL; *count is always written. */
int gra_get_decal_state(gra_app *app, uint32_t *count, uint32_t *order, float *world_to_texture, float *mvps, uint32_t *ranges);

/* Synthetic G-buffer (host pointers, tightly packed rows, width x height of the config).  Any pointer may be NULL to
 * leave that attachment unchanged.  Graphs without lighting take `emissive` as the HDR input. */
int gra_upload_gbuffer(gra_app *app, const void *emissive_rgba16f, const void *albedo_rgba8, const void *normal_a2b10g10r10,
                       const void *pbr_rg8, const void *depth_d32f, const void *motion_vectors_rg16f);

/* Render-sized R8_UNORM ambient-occlusion image (host pointer, tightly packed); needs config.ambient_occlusion ==
 * GRA_AMBIENT_OCCLUSION_UPLOAD (declared below the aa_bench upload). */
/* The two input images of the aa_bench graph: R8G8B8A8_SRGB, tightly packed, any size (both the same). */
int gra_upload_aa_bench_images(gra_app *app, const void *rgba8_first, const void *rgba8_second, uint32_t width, uint32_t height);
int gra_upload_ambient_occlusion(gra_app *app, const void *ao_r8);

/* ---- GTX ("GRANITE TEXFMT1", vulkan/texture/memory_mapped_texture.cpp:29-44): the container Granite keeps textures and
 * image dumps in -- the wire format on either side of this path.  Header fields as stored; payload = mip levels in order,
 * each at a 16-byte aligned offset (vulkan/texture/texture_format.cpp:349-387). */
typedef struct gra_gtx_info
{
	uint32_t type, format, width, height, depth, layers, levels, flags;
	uint64_t payload_size;
} gra_gtx_info;
int gra_gtx_probe(const char *path, gra_gtx_info *info, char *error, size_t error_size);
int gra_gtx_read(const char *path, void *payload, uint64_t payload_capacity, char *error, size_t error_size);
int gra_gtx_write(const char *path, const gra_gtx_info *info, const void *payload, char *error, size_t error_size);
/* gra_upload_gbuffer from .gtx files (2-D, one layer, level 0 is used).  Formats must be the attachment's own:
 * emissive / HDR R16G16B16A16_SFLOAT, albedo R8G8B8A8_SRGB or _UNORM, normal A2B10G10R10_UNORM_PACK32, pbr R8G8_UNORM,
 * depth D32_SFLOAT or R32_SFLOAT, motion vectors R16G16_SFLOAT; sizes must equal the configured frame.  NULL = unchanged.
 * A block-compressed file is accepted where its decoded format (gr_texture_decoded_format) is the attachment's own -- albedo as
 * BC1 / BC2 / BC3 / BC7 or ASTC LDR, pbr as BC5, emissive as BC6H with RGBA16F targets: its blocks are uploaded and decoded into the
 * attachment. */
int gra_upload_gbuffer_gtx(gra_app *app, const char *emissive, const char *albedo, const char *normal, const char *pbr,
                           const char *depth, const char *motion_vectors);
/* Decodes a block-compressed .gtx (BC1-BC7 without SNORM, ASTC LDR; no 3-D) on the application's device, every level and layer
 * (Granite::decode_compressed_image, one gr_texture_decode each), and writes an uncompressed .gtx of the decoded format with the
 * same extents, layers, levels and flags. */
int gra_gtx_decode(gra_app *app, const char *src_path, const char *dst_path);
/* What tools/gtx_convert.cpp does for the formats this build encodes, on the application's device.  The .gtx `src_path` (R8_UNORM,
 * R8G8_UNORM, R8G8B8A8_UNORM; R8G8B8A8_SRGB for a block target without generate_mipmaps; no 3-D) gets, with generate_mipmaps != 0, a full
 * mip chain made from its level 0 (Granite::generate_mipmaps; a chain it has is made again), then every level and layer is compressed to
 * `format` (Granite::compress_texture): VK_FORMAT_BC4_UNORM_BLOCK (139), VK_FORMAT_BC5_UNORM_BLOCK (141, not from R8_UNORM), or the
 * input's own format for a copy.  `dst_path` keeps the extents, layers and flags (less the mipgen-on-load bit where mips were made). */
int gra_gtx_encode(gra_app *app, const char *src_path, const char *dst_path, uint32_t format, int generate_mipmaps);
/* Needs no device.  Granite::string_to_format for the names gra_gtx_encode handles (bc4_unorm, bc5_unorm, r8_unorm, rg8_unorm,
 * rgba8_unorm); 0 (VK_FORMAT_UNDEFINED) for every other name and for NULL. */
uint32_t gra_string_to_format(const char *name);
/* Needs no device.  The layout gra_gtx_encode gives an image described by `input` (payload_size is not read): *output is its header for
 * `format`, with generate_mipmaps != 0 for the full chain, and level_offsets[l], l < level_capacity and l < output->levels, the payload
 * offset of level l.  level_offsets may be NULL. */
int gra_gtx_encode_layout(const gra_gtx_info *input, uint32_t format, int generate_mipmaps, gra_gtx_info *output, uint64_t *level_offsets,
                          uint32_t level_capacity, char *error, size_t error_size);
/* Environment baking on the application's device, what tools/convert_equirect_to_environment.cpp does: the 2-D R16G16B16A16_SFLOAT
 * .gtx `equirect_gtx` becomes a cube of unsigned(cube_scale * max(width / 3, height / 2)) texels with a full mip chain
 * (Granite::convert_equirect_to_cube), from which the 128-texel, 8-level GGX reflection cube (convert_cube_to_ibl_specular) and the
 * 32-texel irradiance cube (convert_cube_to_ibl_diffuse) are made.  Each is written as a cube .gtx (6 layers, the cube bit set in
 * flags) where its path is not NULL; a bake nobody asked for is not run. */
int gra_environment_bake(gra_app *app, const char *equirect_gtx, float cube_scale, const char *cube_path, const char *reflection_path,
                         const char *irradiance_path);
/* One FFT on the application's device through Granite::FFT (host/fft/fft.hpp; renderer/fft/fft.hpp): upload, plan, execute, download.
 * nx, ny, nz, dimensions, mode (gr_fft_mode) and data_type (gr_fft_data_type) as gr_fft_options has them; strides in elements.
 * `input` and `output` are host memory.  `output` is uploaded before the transform and downloaded after it, so bytes the transform
 * does not write come back as they went in.  With image_width == 0 the output is a buffer of output_bytes with the output strides.
 * Otherwise it is a texture: a tightly packed image_width x image_height image of the format the mode stores (gr_fft_resource),
 * image_byte_offset bytes into the output_bytes block, written at output_offset; the bytes of the block before and after the image are
 * guard bytes no store may touch.  Fails (gra_last_error) where the plan or the library refuses. */
typedef struct gra_fft_request
{
	uint32_t nx, ny, nz, dimensions, mode, data_type;
	const void *input;
	uint64_t input_bytes;
	uint32_t input_row_stride, input_layer_stride;
	void *output;
	uint64_t output_bytes;
	uint32_t output_row_stride, output_layer_stride;
	uint32_t image_width, image_height;
	uint64_t image_byte_offset;
	int32_t output_offset[2];
} gra_fft_request;
int gra_fft_transform(gra_app *app, const gra_fft_request *request);
/* ---- the ocean's FFT and LOD updates (Granite::Ocean, host/ocean.hpp) ----------------------------------------------------------
 * gra_ocean_create derives the constructor's values, generates the three Phillips distributions and uploads them, plans the three
 * FFTs and allocates the pass's nine resources; it fails (gra_last_error) for an fft_resolution that is no power of two, for
 * fft_resolution >> displacement_downsample below 64, for a zero grid_count or grid_resolution and for a zero wind velocity, before
 * anything is allocated.  With through_render_graph the pass is added to a render graph of the ocean's own (add_fft_update_pass),
 * baked and executed by the graph; otherwise update_fft_pass runs directly on the generic stream.  Either way gra_ocean_update
 * returns after the pass has completed.  time = fmod(elapsed_time, 256), period = 256 / (2 pi), both narrowed to float.
 *
 * With lod_update the ocean also owns the reference's second per-frame pass, `ocean-update-lods` (add_lod_update_pass / update_lod_pass):
 * gra_ocean_update then runs both passes, and both are complete on return.  It adds the resources ocean-lods (R16_SFLOAT, grid_count
 * squared), ocean-lod-counter (eight 32-byte indirect draws) and ocean-lod-data (grid_count^2 * 8 patches of 32 bytes), ids 9 .. 11 of
 * gra_ocean_describe / gra_ocean_read; without lod_update they do not exist.  gra_ocean_create refuses lod_update without a heightmap and
 * with a grid_count or grid_resolution that is not a power of two in 4 .. 128, before anything is allocated.  With fixed_position the
 * grid stays around center_position (the reference's scene node): no image offset, clamped LOD taps, no edge LODs, no border mesh.
 * A configuration whose last three fields are zero is the ocean of before they existed. */
#define GRA_OCEAN_HEIGHT_FFT_INPUT 0u
#define GRA_OCEAN_NORMAL_FFT_INPUT 1u
#define GRA_OCEAN_DISPLACEMENT_FFT_INPUT 2u
#define GRA_OCEAN_HEIGHT_FFT_OUTPUT 3u
#define GRA_OCEAN_DISPLACEMENT_FFT_OUTPUT 4u
#define GRA_OCEAN_NORMAL_FFT_OUTPUT 5u
#define GRA_OCEAN_SPD_COUNTER 6u
#define GRA_OCEAN_GRADIENT_JACOBIAN_OUTPUT 7u
#define GRA_OCEAN_HEIGHT_DISPLACEMENT_OUTPUT 8u
#define GRA_OCEAN_RESOURCE_COUNT 9u /* of the FFT update */
#define GRA_OCEAN_LODS 9u
#define GRA_OCEAN_LOD_COUNTER 10u
#define GRA_OCEAN_LOD_DATA 11u
#define GRA_OCEAN_TOTAL_RESOURCE_COUNT 12u
#define GRA_OCEAN_MESH_BORDER 0xffffffffu /* gra_ocean_mesh_*: the border mesh, after the plane grid when there is no heightmap */
#define GRA_OCEAN_DISTRIBUTION_HEIGHT 0u
#define GRA_OCEAN_DISTRIBUTION_DISPLACEMENT 1u
#define GRA_OCEAN_DISTRIBUTION_NORMAL 2u
typedef struct gra_ocean_config /* OceanConfig, renderer/ocean.hpp:40-75, and two switches of this executor */
{
	uint32_t fft_resolution, displacement_downsample, grid_count, grid_resolution;
	float ocean_size[2], wind_velocity[2];
	float normal_mod, amplitude;
	uint32_t heightmap;
	float lod_bias;
	uint32_t force_mipmap_shader;  /* every mip chain level by level through gr_ocean_mipmap */
	uint32_t through_render_graph; /* run the pass inside a RenderGraph */
	uint32_t freq_band_modulation;
	float frequency_bands[8];
	uint32_t lod_update;      /* the LOD update, its three resources and the meshes on the device */
	uint32_t fixed_position;  /* the grid stays around center_position */
	float center_position[3];
} gra_ocean_config;
typedef struct gra_ocean gra_ocean;
typedef struct gra_ocean_resource_info
{
	uint32_t exists, is_image, width, height, format, levels;
	uint64_t size_bytes; /* of a buffer, or of level 0 of an image */
} gra_ocean_resource_info;
void gra_ocean_default_config(gra_ocean_config *config);
int gra_ocean_create(gra_app *app, const gra_ocean_config *config, gra_ocean **ocean);
int gra_ocean_update(gra_ocean *ocean, double elapsed_time);
int gra_ocean_describe(gra_ocean *ocean, uint32_t which, gra_ocean_resource_info *info);
/* Level `level` of resource `which` (0 for a buffer), tightly packed, `size` bytes exactly.  Fails for a resource or level that does
 * not exist (ocean-height-displacement-output without a heightmap) and for a size that is not the level's. */
int gra_ocean_read(gra_ocean *ocean, uint32_t which, uint32_t level, void *out, uint64_t size);
/* The host's copy of a distribution: N * N float2, N = fft_resolution (>> displacement_downsample for the displacement one). */
int gra_ocean_distribution(gra_ocean *ocean, uint32_t which, void *out);
/* Heightmap and normal map world sizes, wind direction, Phillips L and the normalised amplitude: 8 floats. */
int gra_ocean_parameters(gra_ocean *ocean, float *out8);
/* Stands in for the reference's camera refresh and visibility frustum: position, and six planes (x, y, z, w; a point is inside where
 * dot(plane.xyz, point) + plane.w >= 0) for the next gra_ocean_update.  Before the first call the camera is at the origin and every
 * block is in view.  Fails for non-finite input and for a position whose snapped grid coordinate lies beyond +-2^20 blocks. */
int gra_ocean_set_camera(gra_ocean *ocean, const float position[3], const float planes[24]);
/* What a rasteriser needs beside the buffers and maps (renderer/ocean.cpp:826-860, 1082-1092).  The structure shares its name with the
 * call that fills it, so it is a tag without a typedef: `struct gra_ocean_draw_info info;`. */
struct gra_ocean_draw_info
{
	float data[16];        /* OceanData, std140: world_offset at 0, coord_offset at 4, inv_heightmap_size at 6, inv_ocean_grid_size at 8,
	                          normal_uv_scale at 10, integer_to_world_mod at 12, heightmap_range at 14 */
	uint32_t lods;         /* buckets in use and LOD meshes */
	uint32_t lod_stride;   /* bytes between two buckets of ocean-lod-data */
	uint32_t border_count; /* indices of the border mesh */
	uint32_t index_type;   /* 0: VK_INDEX_TYPE_UINT16, restart index 0xffff */
};
int gra_ocean_draw_info(gra_ocean *ocean, struct gra_ocean_draw_info *out);
typedef struct gra_ocean_mesh_info
{
	uint32_t exists, on_device; /* on_device: read from the ocean's vertex and index buffers (lod_update), else from the host's copy */
	uint32_t vertex_count, vertex_stride, index_count, index_stride;
} gra_ocean_mesh_info;
/* which = 0 .. lods - 1: a LOD mesh, vertices of uint8 pos[4] + uint8 weights[4]; GRA_OCEAN_MESH_BORDER: positions of three floats.
 * Both have 16-bit indices in triangle strips.  gra_ocean_mesh_read fills vertex_count * vertex_stride and index_count * index_stride
 * bytes. */
int gra_ocean_mesh_describe(gra_ocean *ocean, uint32_t which, gra_ocean_mesh_info *info);
int gra_ocean_mesh_read(gra_ocean *ocean, uint32_t which, void *vbo_out, void *ibo_out);
void gra_ocean_destroy(gra_ocean *ocean);

/* ---- MESHLET4 mesh files (host/mesh/meshlet.hpp; vulkan/mesh/meshlet.hpp) ----
 * gra_meshlet_describe needs no device: it maps the file through Granite::Meshlet::create_mesh_view and fails, with the view's reason
 * in `error`, for a file the view refuses. */
typedef struct gra_meshlet_info
{
	uint32_t style;        /* 0 Wireframe, 1 Textured, 2 Skinned */
	uint32_t stream_count; /* 2, 4, 6 */
	uint32_t meshlet_count;
	uint32_t payload_size_words;
	uint32_t total_primitives;
	uint32_t total_vertices;
	uint32_t chunk_count; /* ceil(meshlet_count / 8) */
	uint32_t padding;
} gra_meshlet_info;
int gra_meshlet_describe(const char *path, gra_meshlet_info *info, char *error, size_t error_size);
/* Decodes the file on the application's device (Granite::Meshlet::decode_mesh, one gr_meshlet_decode launch) into host arrays.  Each
 * array that is not NULL is uploaded first and downloaded afterwards, so bytes the decode does not write come back as they went in.
 * Sizes in bytes, with P = primitive_offset + total_primitives and V = vertex_offset + total_vertices as the least element counts:
 * indices P * 3 * (4 with GR_MESHLET_DECODE_UNROLLED_MESH, 2 with GR_MESHLET_DECODE_INDEX_16, else 1); positions V * 12; attributes
 * V * 16 (target_style >= 1); skin V * 8 (target_style 2); indirect, optional, chunk_count * (128 for the Meshlet runtime style: eight
 * {primitive_offset, vertex_offset, primitive_count, vertex_count}; 12 for MDI: {indexCount, firstIndex, vertexOffset}).  A larger
 * array is taken whole: what lies past the last element is not written.  Fails for an array the style needs that is NULL or too small. */
typedef struct gra_meshlet_request
{
	uint32_t flags;         /* GR_MESHLET_DECODE_* */
	uint32_t target_style;  /* not above the file's */
	uint32_t runtime_style; /* 0 MDI, 1 Meshlet */
	uint32_t primitive_offset, vertex_offset;
	uint32_t padding;
	void *indices, *positions, *attributes, *skin, *indirect;
	uint64_t indices_bytes, positions_bytes, attributes_bytes, skin_bytes, indirect_bytes;
} gra_meshlet_request;
int gra_meshlet_decode(gra_app *app, const char *path, const gra_meshlet_request *request, gra_meshlet_info *result);

/* Writes a graph texture (all its mip levels) or, with name == NULL, the last rendered backbuffer as .gtx. */
int gra_save_resource_gtx(gra_app *app, const char *name, const char *path);

/* Application::run_frame x count; asynchronous unless sync != 0. */
int gra_render_frames(gra_app *app, uint32_t count, int32_t sync);
int gra_sync(gra_app *app);

/* Resource access by render-graph name ("HDR-main", "tonemapped", "upsample-0", "cluster-bitmask", ...). */
typedef struct gra_resource_info
{
	void *device_ptr;
	uint32_t width, height, format; /* 0 x 0 for buffers */
	uint64_t size_bytes;            /* whole mip chain when levels > 1 (gr_mip_chain_size) */
	int32_t physical_index;
	uint32_t levels;                /* 1 unless the attachment was declared with a mip chain; 0 for buffers */
} gra_resource_info;
int gra_get_resource(gra_app *app, const char *name, gra_resource_info *info);
int gra_read_resource(gra_app *app, const char *name, void *dst_host, uint64_t size_bytes);
/* The write-side twin of gra_read_resource: replaces the contents of a graph resource with `size_bytes` of host data (the whole
 * resource).  Meant for the state a frame inherits from the one before it -- "average-luminance" (exposure adaptation),
 * "downsample-3" (bloom feedback), "<output>-history" of a TAA resolve: what gra_read_resource returned after frame N, written into
 * a fresh application before its first frame (or into a running one), is what frame N + 1 reads as "previous" (persistent
 * buffers in place; an image with a history copy becomes the history at the next frame's swap, render_graph.cpp:2704-2708).
 * Together with gra_get / set_frame_state a run can be resumed bit for bit (checkpoint / replay). */
int gra_write_resource(gra_app *app, const char *name, const void *src_host, uint64_t size_bytes);
/* Host-side state a frame inherits: elapsed time, swapchain ring position, the (moving) camera's view matrix and the temporal
 * jitter's phase with its saved view-projection ring (temporal.cpp:40-196). */
typedef struct gra_frame_state
{
	uint64_t frames;
	double elapsed;
	uint32_t swapchain_index;
	uint32_t jitter_phase;
	float base_view[16];
	float jittered_projection[16];
	float view_proj[16][16], inv_view_proj[16][16], jittered_view_proj[16][16]; /* first jitter_count entries */
} gra_frame_state;
int gra_get_frame_state(gra_app *app, gra_frame_state *state);
int gra_set_frame_state(gra_app *app, const gra_frame_state *state);
/* The swapchain image the last frame was rendered into (external to the graph, 4-image ring).  The image is complete only after
 * gra_sync (gra_read_backbuffer syncs itself) or, for work on a stream of the caller's, behind the executor stream that wrote it last:
 * gra_render_frames with sync == 0 returns while the frame is still being rendered, and the image is rewritten four frames later.
 * Recorded frames (gra_video_*, below) are the supported way to consume frames asynchronously. */
int gra_get_backbuffer(gra_app *app, gra_resource_info *info);
int gra_read_backbuffer(gra_app *app, void *dst_host, uint64_t size_bytes);

/* Clusterer CPU-side state of the last refresh, for parity tests.  Returns the number of lights. */
int gra_get_cluster_state(gra_app *app, void *lights48, void *models48, uint32_t *type_mask128, void *params176,
                          uint32_t *light_ranges_uvec2);

/* JSON dump of the baked graph (pass order, physical resources).  Returns the length needed. */
size_t gra_dump_graph(gra_app *app, char *buffer, size_t size);

/* GPU time per physical pass accumulated since creation or the last gra_reset_timestamps (enable_timestamps): tags are the
 * reference's (render_graph.cpp:2274-2289, "a + b" for passes it runs as subpasses of one render pass), one accumulation per
 * physical pass and frame.  Fills up to max entries, returns the count. */
typedef struct gra_timestamp
{
	char tag[64];
	uint64_t count;
	double total_ms;
} gra_timestamp;
int gra_collect_timestamps(gra_app *app, gra_timestamp *entries, int max_entries);
/* emit_single_pass_downsample (renderer/post/spd.cpp:56-102) the way the reference uses it (renderer/ocean.cpp:579-601): an
 * RGBA16F image of `levels` mip levels whose level 0 is the source and whose levels 1.. are written by the single-pass
 * downsampler (`components` channels, optional per-level filter_mods = (levels - 1) x vec4).  level0: width x height texels in;
 * chain: all levels out, tightly packed (gr_mip_chain_offset).  Runs on the application's device. */
int gra_generate_mipmaps(gra_app *app, const void *level0_rgba16f, uint32_t width, uint32_t height, uint32_t levels,
                         uint32_t components, const float *filter_mods, void *chain_rgba16f);

/* Device::timestamp_log_reset (application_headless.cpp:591): forget what was accumulated, e.g. the warm-up frame. */
int gra_reset_timestamps(gra_app *app);
/* The scene's DirectionalLightComponent (read_lights, scene_viewer_application.cpp:58-77): replaces the values of
 * gra_config for the frames that follow; direction is normalised here. */
int gra_set_directional_light(gra_app *app, const float direction[3], const float color[3]);
/* LightingParameters::fog (renderer/lights/lights.hpp; the scene's "fog" entry in Granite): with falloff > 0 render_light ends with
 * the fog quad (renderer.cpp:1179-1196).  falloff = 0 switches it off again. */
int gra_set_fog(gra_app *app, const float color[3], float falloff);
/* The directional light's shadow map (LightingParameters::shadows and ::shadow).  There is no rasteriser here: the caller uploads the
 * map as it uploads the G-buffer, and the lighting pass then draws the shadowed directional quad (gr_directional_light) followed by the
 * clustered lights in place.  Runtime state, not a member of gra_config: NULL, or mode 0, switches shadows off again, and the frames that
 * follow are those of an application that never had them.
 *   mode      GR_SHADOW_PCF (1), GR_SHADOW_PCF_WIDE (2) or GR_SHADOW_VSM (3)
 *   layers    1, or 4 for cascades; `texels` holds them one after another, each width x height, tightly packed
 *   format    GR_FORMAT_D16_UNORM or GR_FORMAT_D32_SFLOAT; with GR_SHADOW_VSM also GR_FORMAT_R32G32_SFLOAT (finished moments).  A depth
 *             format with GR_SHADOW_VSM runs the VSM chain on upload: moments, the down blur to half size, the up blur
 *   transforms, cascade_log_bias   world -> (u, v, z) per layer, column-major, and the bias of log2(view_z)
 * Refused with a message, nothing launched and the state unchanged: an application without lighting, aa_bench, strip_count > 1,
 * hdr_packed_float, layers other than 1 or 4, a format that does not fit the mode, a width or height of 0 or above 16384, a
 * struct_size other than sizeof(gra_directional_shadows), null texels. */
typedef struct gra_directional_shadows
{
	uint32_t struct_size;
	uint32_t mode;
	uint32_t layers;
	uint32_t width;
	uint32_t height;
	uint32_t format;
	const void *texels;
	float transforms[4][16];
	float cascade_log_bias;
	uint32_t pad0;
} gra_directional_shadows;
int gra_set_directional_shadows(gra_app *app, const gra_directional_shadows *desc);
/* T(.5,.5,0) S(.5,.5,1) VP_prev inv(VP_cur) as pushed to the last taa-resolve (temporal.cpp:239-243). */
int gra_get_taa_reprojection(gra_app *app, float *reproj16);
/* SMAA AreaTex (160x560 RG8) / SearchTex (64x16 R8) payloads, host pointers; needed before a frame with an SMAA pass. */
int gra_set_smaa_luts(gra_app *app, const void *area_rg8, const void *search_r8);
/* Row-band tiling.  The executor calls `fn` where the bands of all ranks must meet (after the 1/8 bloom level, after
 * tonemap): an in-place all-gather of `rank_count` chunks of `chunk_bytes` bytes laid out back to back from `device_ptr`
 * (this rank's chunk already sits at device_ptr + strip_index * chunk_bytes), to be enqueued on `stream` (hipStream_t).
 * bench.py implements it with torch.distributed (RCCL); tests with local copies. */
typedef void (*gra_exchange_fn)(void *user, const char *tag, void *device_ptr, uint64_t chunk_bytes, uint32_t rank_count, void *stream);
int gra_set_exchange_callback(gra_app *app, gra_exchange_fn fn, void *user);
/* RCCL transport for the band exchanges: rank 0 creates a 128-byte id (gra_comm_create_unique_id), the launcher ships it
 * to every rank (bench.py: torch.distributed broadcast), every rank calls gra_comm_init; from then on the exchange points
 * are in-place ncclAllGather calls on the executor's stream (xGMI between the GPUs of one node).  ranks must equal the
 * config's strip_count and rank its strip_index. */
int gra_comm_create_unique_id(uint8_t *id128);
int gra_comm_init(gra_app *app, const uint8_t *id128, int32_t rank, int32_t ranks);
/* Optional second communicator (its own id from gra_comm_create_unique_id, after gra_comm_init): the all-gather of the
 * tonemapped bands then runs on a stream of its own behind each frame's tonemap and overlaps the following frames instead of
 * sitting on the back-of-frame stream.  gra_sync / readbacks wait for it. */
/* What the in-frame communicator reports about itself, for run records: nranks = ncclCommCount, version = ncclGetVersion (each -1
 * when the loaded library has no such entry point), stand_in = 1 when GRANITE_RCCL_LIBRARY replaced librccl.so.1. */
int gra_comm_info(gra_app *app, int32_t *nranks, int32_t *version, int32_t *stand_in);
int gra_comm_init_output(gra_app *app, const uint8_t *id128, int32_t rank, int32_t ranks);
/* The band plan of this instance: out[0..3] = index, count, width, height; then {whole, first, count} for lighting,
 * threshold, downsample-0, downsample-1, upsample-0, tonemap; then d1_chunk_rows, out_chunk_rows (24 values). */
int gra_get_strip_plan(gra_app *app, uint32_t *out24);
/* The anti-aliasing part of the plan (config.pre_aa / post_aa under row bands): {whole, first, count} for the TAA resolve,
 * smaa-edge, smaa-weights and the post-AA output band (12 values).  The tonemap and lighting ranges of gra_get_strip_plan
 * already include the rows these passes read around the band. */
int gra_get_strip_plan_aa(gra_app *app, uint32_t *out12);
/* The TAA history under row bands: out[0] = config.taa_history_reach_rows, out[1] = rows every rank hands to each neighbour per
 * frame (0 = the bands are all-gathered whole: reach 0, or bands thinner than the exchange), out[2..4] = {whole, first, count} of
 * the history rows this rank holds after the exchange. */
int gra_get_strip_plan_taa_history(gra_app *app, uint32_t *out5);

/* Host-side frame-loop cost since creation: out[0] = frames, out[1] = seconds spent inside the frame loop (light
 * refresh + graph execution = launches), out[2] = seconds of those spent blocked on GPU back-pressure. */
/* The constant tables of the SSR pass (process-wide): the blue-noise sampler's 128 x 128 x 2 integer values and the
 * R16G16_SFLOAT split-sum BRDF table (width x height texels); see csrc/host/post/ssr.hpp. */
int gra_install_ssr_tables(const uint8_t *blue_noise_128x128_rg8, const uint16_t *brdf_lut_rg16f, uint32_t brdf_width, uint32_t brdf_height);
int gra_get_host_stats(gra_app *app, double *out3);
/* Row bands with the output gather beside the frame (gra_comm_init_output): out[0] = times a pass was about to overwrite an output
 * image, out[1] = of those, how often the all-gather that last read it was still in flight (the pass waits: the gather was not hidden
 * behind the following frames).  The collectives' device times are gr_timing_* names "inframe_gather" / "output_gather". */
int gra_get_output_gather_stats(gra_app *app, uint64_t *out2);
/* Frames whose light sort + pack (LightClusterer::refresh) had already been done by the clusterer's helper thread while the
 * previous frame was being enqueued (the reference runs its refreshes as TaskComposer tasks beside command recording). */
int gra_get_prefetched_refreshes(gra_app *app, uint64_t *out);
/* Pre-recorded launch sequences replayed so far (HIP::CommandBuffer::replayable, opt-in with GRANITE_LAUNCH_GRAPHS=1: the bloom
 * pass's six launches and the cluster build's four go out as one hipGraph launch each once their arguments repeat; less host
 * time, but a slower frame on this runtime -- see hip_device.hpp -- so the default launches every kernel directly). */
int gra_get_launch_graph_replays(gra_app *app, uint64_t *out);
/* compute_rec709_to_st2020 (hdr.cpp:580-593) for display primaries r, g, b, white (CIE xy, 8 floats): column-major 3 x 3. */
int gra_compute_rec709_to_display(const float *primaries8, float *out9);
/* Bytes of HBM currently held by the executor's images and buffers (graph attachments, hand-over rings, uploads). */
int gra_get_allocated_bytes(gra_app *app, uint64_t *out);
/* Per-kernel timing lives in the kernel library: gr_timing_* on this context. */
void *gra_get_kernel_context(gra_app *app); /* gr_ctx* */
void *gra_get_stream(gra_app *app);         /* hipStream_t of the generic queue */

/* ---- frame recording (the headless runner's --video-encode-path: application_headless.cpp, VideoEncoder::process_rgb) ------------
 * While recording, every frame's backbuffer is converted by gr_video_scale (VideoScaler::rescale) on a stream of the recorder's own,
 * behind the frame fences of the executor streams that rendered it (no device sync), and copied into a ring of pinned host buffers.
 * The swapchain image is rewritten four frames later only after its conversion has read it.  gra_render_frames fails, before it
 * enqueues anything for that frame, when `ring_frames` frames are unread: frames are never overwritten or dropped.  Input colour
 * space: HDR10 when the app renders hdr10, sRGB otherwise.  Not available with row bands (strip_count > 1). */
typedef enum gra_video_format
{
	GRA_VIDEO_NV12 = 0,      /* Y + interleaved CbCr, 8 bits, 4:2:0 */
	GRA_VIDEO_YUV420P = 1,   /* Y, Cb, Cr, 8 bits, 4:2:0 */
	GRA_VIDEO_YUV420P16 = 2, /* 16 bits (UNORM16) */
	GRA_VIDEO_YUV444P = 3,
	GRA_VIDEO_YUV444P16 = 4,
	GRA_VIDEO_P010 = 5,      /* Y + interleaved CbCr, 16-bit words (UNORM16, as the reference stores them), 4:2:0 */
	GRA_VIDEO_P016 = 6
} gra_video_format;
typedef struct gra_video_options
{
	uint32_t format;      /* gra_video_format */
	uint32_t width, height; /* encode size; 0 = the backbuffer's */
	int32_t hdr10;        /* output colour space HDR10 (ST 2084, BT.2020) instead of sRGB (BT.709) */
	uint32_t ring_frames; /* unread frames held; 0 = 8 */
} gra_video_options;
/* One packed frame: planes back to back, rows tightly packed. */
typedef struct gra_video_layout
{
	uint32_t num_planes;
	uint32_t bytes_per_sample;   /* 1 or 2 */
	uint32_t width[3], height[3]; /* in samples; an interleaved CbCr plane counts pairs */
	uint32_t pitch[3];            /* bytes */
	uint64_t offset[3];
	uint64_t frame_bytes;
} gra_video_layout;
int gra_video_begin(gra_app *app, const gra_video_options *options);
int gra_video_frame_layout(gra_app *app, gra_video_layout *layout);
/* The oldest unread recorded frame, in order: waits for that frame's copy only.  0: copied (frame_number = the frame's index since
 * gra_video_begin, from 0); 1: no frame pending; negative: error. */
int gra_video_read_frame(gra_app *app, void *dst_host, uint64_t size_bytes, int64_t *frame_number);
int gra_video_end(gra_app *app);

/* ---- frame playback (VideoDecoder's upload + dispatch_conversion, ffmpeg_decode.cpp, without demuxer and decoder) ------------------
 * The other direction: packed YCbCr frames in the layout recording produces (`format` at width x height, gra_video_play_layout) are
 * uploaded and converted to RGB by gr_video_yuv_to_rgb on a stream of the player's own; the images come back in order through a
 * ring of pinned host buffers.  No device sync on this path.  Not available with row bands (strip_count > 1). */
typedef struct gra_video_play_options
{
	uint32_t format;        /* gra_video_format of the frames handed over */
	uint32_t width, height; /* of the frames and of the RGB images */
	gr_video_yuv_info info; /* what a decoder knows about the stream; recorded frames are full range, centre-sited, 8 or 16 bits */
	uint32_t output_format; /* GR_FORMAT_R8G8B8A8_UNORM / _SRGB; with info.pq: A2B10G10R10_UNORM_PACK32 or R16G16B16A16_SFLOAT */
	uint32_t ring_frames;   /* unread images held; 0 = 8 */
} gra_video_play_options;
int gra_video_play_begin(gra_app *app, const gra_video_play_options *options);
int gra_video_play_layout(gra_app *app, gra_video_layout *layout);
/* One frame of exactly gra_video_play_layout's frame_bytes: copied before the call returns, then uploaded and converted
 * asynchronously.  Fails when `ring_frames` images are unread: images are never overwritten or dropped. */
int gra_video_play_frame(gra_app *app, const void *frame, uint64_t size_bytes);
/* The oldest unread image (width x height texels of output_format, tightly packed), in order: waits for that frame's conversion and
 * copy only.  0: copied (frame_number = the frame's index since gra_video_play_begin, from 0); 1: none pending; negative: error. */
int gra_video_play_read_rgb(gra_app *app, void *dst_host, uint64_t size_bytes, int64_t *frame_number);
/* Frames still in flight are drained (the player's stream only), then everything is released. */
int gra_video_play_end(gra_app *app);

#ifdef __cplusplus
}
#endif
#endif
