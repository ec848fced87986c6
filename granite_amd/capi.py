"""ctypes binding of the gfx950 executor's C ABI (include/granite_hip.h).

This is the Python-side twin of what a Granite maintainer binds from C++: plain pointers and sizes,
no torch types.  The library is built in-tree by ``__graft_entry__.build()`` / ``granite_amd/csrc/Makefile`` and must be
present: there is no CPU fallback, every entry point raises if the HIP library is missing or a call fails.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GRANITE_LIB_DIR: an A/B build of the same sources (make OUT=../lib_xyz EXTRA_<unit>=...), for measurements only
LIB_PATH = os.path.join(_HERE, os.environ.get("GRANITE_LIB_DIR", "lib"), "libgranite_hip.so")

# gr_format (VkFormat numeric values)
FORMAT_R8_UNORM = 9
FORMAT_R8G8_UNORM = 16
FORMAT_R8G8B8A8_UNORM = 37
FORMAT_R8G8B8A8_SRGB = 43
FORMAT_B8G8R8A8_UNORM = 44
FORMAT_B8G8R8A8_SRGB = 50
FORMAT_A2B10G10R10_UNORM_PACK32 = 64
FORMAT_R16_UNORM = 70
FORMAT_R16_SFLOAT = 76
FORMAT_R16G16_UNORM = 77
FORMAT_R16G16_SFLOAT = 83
FORMAT_R16G16B16A16_SFLOAT = 97
FORMAT_R32_SFLOAT = 100
FORMAT_R32G32_SFLOAT = 103
FORMAT_B10G11R11_UFLOAT_PACK32 = 122
FORMAT_D16_UNORM = 124
FORMAT_D32_SFLOAT = 126
# block-compressed inputs of gr_texture_decode (VkFormat numbers; 140 / 142, the SNORM forms, are not handled)
FORMAT_BC1_RGB_UNORM_BLOCK = 131
FORMAT_BC1_RGB_SRGB_BLOCK = 132
FORMAT_BC1_RGBA_UNORM_BLOCK = 133
FORMAT_BC1_RGBA_SRGB_BLOCK = 134
FORMAT_BC2_UNORM_BLOCK = 135
FORMAT_BC2_SRGB_BLOCK = 136
FORMAT_BC3_UNORM_BLOCK = 137
FORMAT_BC3_SRGB_BLOCK = 138
FORMAT_BC4_UNORM_BLOCK = 139
FORMAT_BC5_UNORM_BLOCK = 141
FORMAT_BC6H_UFLOAT_BLOCK = 143
FORMAT_BC6H_SFLOAT_BLOCK = 144
FORMAT_BC7_UNORM_BLOCK = 145
FORMAT_BC7_SRGB_BLOCK = 146
BLOCK_FORMATS = (131, 132, 133, 134, 135, 136, 137, 138, 139, 141, 143, 144, 145, 146)  # BC1-BC7: 4 x 4 texels a block
# ASTC LDR, 2-D footprints, 16 bytes a block (the SFLOAT forms are not handled)
FORMAT_ASTC_4x4_UNORM_BLOCK = 157
FORMAT_ASTC_4x4_SRGB_BLOCK = 158
FORMAT_ASTC_5x4_UNORM_BLOCK = 159
FORMAT_ASTC_5x4_SRGB_BLOCK = 160
FORMAT_ASTC_5x5_UNORM_BLOCK = 161
FORMAT_ASTC_5x5_SRGB_BLOCK = 162
FORMAT_ASTC_6x5_UNORM_BLOCK = 163
FORMAT_ASTC_6x5_SRGB_BLOCK = 164
FORMAT_ASTC_6x6_UNORM_BLOCK = 165
FORMAT_ASTC_6x6_SRGB_BLOCK = 166
FORMAT_ASTC_8x5_UNORM_BLOCK = 167
FORMAT_ASTC_8x5_SRGB_BLOCK = 168
FORMAT_ASTC_8x6_UNORM_BLOCK = 169
FORMAT_ASTC_8x6_SRGB_BLOCK = 170
FORMAT_ASTC_8x8_UNORM_BLOCK = 171
FORMAT_ASTC_8x8_SRGB_BLOCK = 172
FORMAT_ASTC_10x5_UNORM_BLOCK = 173
FORMAT_ASTC_10x5_SRGB_BLOCK = 174
FORMAT_ASTC_10x6_UNORM_BLOCK = 175
FORMAT_ASTC_10x6_SRGB_BLOCK = 176
FORMAT_ASTC_10x8_UNORM_BLOCK = 177
FORMAT_ASTC_10x8_SRGB_BLOCK = 178
FORMAT_ASTC_10x10_UNORM_BLOCK = 179
FORMAT_ASTC_10x10_SRGB_BLOCK = 180
FORMAT_ASTC_12x10_UNORM_BLOCK = 181
FORMAT_ASTC_12x10_SRGB_BLOCK = 182
FORMAT_ASTC_12x12_UNORM_BLOCK = 183
FORMAT_ASTC_12x12_SRGB_BLOCK = 184
ASTC_FOOTPRINTS = ((4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (8, 5), (8, 6), (8, 8), (10, 5), (10, 6), (10, 8), (10, 10), (12, 10), (12, 12))
ASTC_FORMATS = {157 + i: ASTC_FOOTPRINTS[i // 2] for i in range(28)}  # format -> (block width, block height)

FORMAT_BPP = {
    FORMAT_R8_UNORM: 1,
    FORMAT_R8G8_UNORM: 2,
    FORMAT_R8G8B8A8_UNORM: 4,
    FORMAT_R8G8B8A8_SRGB: 4,
    FORMAT_B8G8R8A8_UNORM: 4,
    FORMAT_B8G8R8A8_SRGB: 4,
    FORMAT_R16_UNORM: 2,
    FORMAT_R16G16_UNORM: 4,
    FORMAT_A2B10G10R10_UNORM_PACK32: 4,
    FORMAT_R16_SFLOAT: 2,
    FORMAT_R16G16_SFLOAT: 4,
    FORMAT_R16G16B16A16_SFLOAT: 8,
    FORMAT_R32_SFLOAT: 4,
    FORMAT_R32G32_SFLOAT: 8,
    FORMAT_B10G11R11_UFLOAT_PACK32: 4,
    FORMAT_D16_UNORM: 2,
    FORMAT_D32_SFLOAT: 4,
}

# gr_video_scale: VkColorSpaceKHR values, scaler.comp CONTROL bits and transfer functions
COLOR_SPACE_SRGB_NONLINEAR = 0
COLOR_SPACE_EXTENDED_SRGB_LINEAR = 1000104002
COLOR_SPACE_HDR10_ST2084 = 1000104008
VIDEO_CONTROL_SKIP_RESCALE_BIT = 1
VIDEO_CONTROL_DOWNSCALING_BIT = 2
VIDEO_CONTROL_SAMPLED_DOWNSCALING_BIT = 4
VIDEO_CONTROL_CLAMP_COORD_BIT = 8
VIDEO_CONTROL_CHROMA_SUBSAMPLE_BIT = 16
VIDEO_CONTROL_PRIMARY_CONVERSION_BIT = 32
VIDEO_CONTROL_DITHER_BIT = 64
VIDEO_TRANSFER_IDENTITY = 0
VIDEO_TRANSFER_SRGB = 1
VIDEO_TRANSFER_PQ = 2
# gr_video_yuv_to_rgb: gr_video_yuv_info.matrix and .chroma_location
VIDEO_MATRIX_UNSPECIFIED, VIDEO_MATRIX_BT601_525, VIDEO_MATRIX_BT601_625, VIDEO_MATRIX_BT709, VIDEO_MATRIX_BT2020, VIDEO_MATRIX_SMPTE240M = range(6)
VIDEO_CHROMA_CENTER, VIDEO_CHROMA_LEFT, VIDEO_CHROMA_TOPLEFT, VIDEO_CHROMA_TOP, VIDEO_CHROMA_BOTTOMLEFT, VIDEO_CHROMA_BOTTOM = range(6)

LIGHTING_DIRECTIONAL_BIT = 1
LIGHTING_CLUSTERED_BIT = 2
LIGHTING_AMBIENT_FALLBACK_BIT = 4
LIGHTING_AMBIENT_OCCLUSION_BIT = 8
LIGHTING_SHARE_REGISTERS_BIT = 16  # scheduling hint only (include/granite_hip.h)

MAX_LIGHTS_BINDLESS = 4096
CULL_SETUP_BYTES_PER_LIGHT = 512
TRANSFORMED_SPOT_BYTES_PER_LIGHT = 96
TRANSFORMS_OFFSET_LIGHTS = 0
TRANSFORMS_OFFSET_SHADOW = 196608
TRANSFORMS_OFFSET_MODEL = 458752
TRANSFORMS_OFFSET_TYPE_MASK = 655360
TRANSFORMS_OFFSET_DECALS = 655872
TRANSFORMS_SIZE = 852480


class Cube(C.Structure):
    """gr_cube: an R16G16B16A16_SFLOAT cube mip chain in GTX payload layout (device pointer, texels a side, levels)."""
    _fields_ = [("ptr", C.c_void_p), ("size", C.c_uint32), ("levels", C.c_uint32)]


class Image(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("pitch_bytes", C.c_uint32),
                ("format", C.c_uint32)]


# gr_fft_mode, gr_fft_data_type, gr_fft_resource_type, gr_fft_pass_kind, gr_fft_buffer_id
FFT_FORWARD_C2C, FFT_INVERSE_C2C, FFT_R2C, FFT_C2R = 0, 1, 2, 3
FFT_FP32, FFT_FP16 = 0, 1
FFT_RESOURCE_TEXTURE, FFT_RESOURCE_BUFFER = 0, 1
FFT_PASS_C2C, FFT_PASS_R2C_RESOLVE, FFT_PASS_C2R_RESOLVE = 0, 1, 2
FFT_BUFFER_SRC, FFT_BUFFER_DST, FFT_BUFFER_SCRATCH_A, FFT_BUFFER_SCRATCH_B = 0, 1, 2, 3


class FftOptions(C.Structure):
    """gr_fft_options."""
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32), ("dimensions", C.c_uint32), ("mode", C.c_uint32),
                ("data_type", C.c_uint32), ("input_resource", C.c_uint32), ("output_resource", C.c_uint32)]


class FftResource(C.Structure):
    """gr_fft_resource: a buffer (ptr, size_bytes, strides in elements) or an image with its output offset."""
    _fields_ = [("type", C.c_uint32), ("ptr", C.c_void_p), ("size_bytes", C.c_uint64), ("row_stride", C.c_uint32), ("layer_stride", C.c_uint32),
                ("image", Image), ("output_offset", C.c_int32 * 2)]


class FftPass(C.Structure):
    """gr_fft_pass: one entry of gr_fft_describe."""
    _fields_ = [("kind", C.c_uint32), ("dimension", C.c_uint32), ("points", C.c_uint32), ("p", C.c_uint32), ("columns", C.c_uint32),
                ("workgroup_size", C.c_uint32), ("grid_size", C.c_uint32), ("lds_bytes", C.c_uint32), ("reads", C.c_uint32), ("writes", C.c_uint32)]


class PushVideo(C.Structure):
    _fields_ = [("resolution", C.c_int32 * 2), ("scaling_to_input", C.c_float * 2), ("inv_input_resolution", C.c_float * 2),
                ("dither_strength", C.c_float)]


assert C.sizeof(PushVideo) == 28


class VideoPlan(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("eotf", C.c_uint32), ("oetf", C.c_uint32), ("num_planes", C.c_uint32), ("push", PushVideo),
                ("gamma_space_transform", C.c_float * 12), ("primary_transform", C.c_float * 9)]


class PushYuvToRgb(C.Structure):
    _fields_ = [("yuv_to_rgb", C.c_float * 16), ("primary_conversion", C.c_float * 16), ("resolution", C.c_uint32 * 2),
                ("inv_resolution", C.c_float * 2), ("chroma_siting", C.c_float * 2), ("chroma_clamp", C.c_float * 2),
                ("unorm_rescale", C.c_float)]


assert C.sizeof(PushYuvToRgb) == 164


class VideoYuvInfo(C.Structure):
    _fields_ = [("bit_depth", C.c_uint32), ("msb_aligned", C.c_uint32), ("full_range", C.c_uint32), ("matrix", C.c_uint32),
                ("chroma_location", C.c_uint32), ("pq", C.c_uint32), ("nv21", C.c_uint32)]


class VideoYuvPlan(C.Structure):
    _fields_ = [("push", PushYuvToRgb), ("spec_pq", C.c_uint32), ("spec_num_planes", C.c_uint32), ("spec_nv21", C.c_uint32),
                ("matrix", C.c_uint32)]


# gr_ocean_generate_fft variants
OCEAN_VARIANT_HEIGHT, OCEAN_VARIANT_GRADIENT_NORMAL, OCEAN_VARIANT_GRADIENT_DISPLACEMENT = 0, 1, 2
OCEAN_NUM_FREQ_BANDS = 8


class PushOceanGenerate(C.Structure):
    """gr_push_ocean_generate: generate_fft.comp's Registers."""
    _fields_ = [("mod_factor", C.c_float * 2), ("N", C.c_uint32 * 2), ("freq_to_band_mod", C.c_float), ("time", C.c_float), ("period", C.c_float)]


class PushOceanBake(C.Structure):
    """gr_push_ocean_bake: bake_maps.comp's Registers."""
    _fields_ = [("inv_size", C.c_float * 4), ("scale", C.c_float * 4)]


class PushOceanMipmap(C.Structure):
    """gr_push_ocean_mipmap: mipmap.comp's Registers."""
    _fields_ = [("result_mod", C.c_float * 4), ("inv_resolution", C.c_float * 2), ("count", C.c_uint32 * 2), ("lod", C.c_float)]


class PushOceanUpdateLod(C.Structure):
    """gr_push_ocean_update_lod: update_lod.comp's Registers (std140, 64 bytes)."""
    _fields_ = [("shifted_camera_pos", C.c_float * 3), ("max_lod", C.c_float), ("image_offset", C.c_int32 * 2), ("num_threads", C.c_int32 * 2),
                ("grid_base", C.c_float * 2), ("grid_size", C.c_float * 2), ("lod_bias", C.c_float), ("padding", C.c_uint32 * 3)]


class PushOceanCull(C.Structure):
    """gr_push_ocean_cull: cull_blocks.comp's Registers (std140, 96 bytes)."""
    _fields_ = [("world_offset", C.c_float * 3), ("padding0", C.c_uint32), ("image_offset", C.c_int32 * 2), ("num_threads", C.c_uint32 * 2),
                ("inv_num_threads", C.c_float * 2), ("grid_base", C.c_float * 2), ("grid_size", C.c_float * 2), ("grid_resolution", C.c_float * 2),
                ("heightmap_range", C.c_float * 2), ("guard_band", C.c_float), ("lod_stride", C.c_uint32), ("max_lod", C.c_float),
                ("handle_edge_lods", C.c_int32), ("padding1", C.c_uint32 * 2)]


class OceanPatch(C.Structure):
    """gr_ocean_patch: PatchData of ocean.inc."""
    _fields_ = [("offsets", C.c_float * 2), ("inner_lod", C.c_float), ("padding", C.c_float), ("lods", C.c_float * 4)]


class OceanIndirectDraw(C.Structure):
    """gr_ocean_indirect_draw: IndirectDraw of ocean.inc."""
    _fields_ = [("index_count", C.c_uint32), ("instance_count", C.c_uint32), ("first_index", C.c_uint32), ("vertex_offset", C.c_int32),
                ("first_instance", C.c_uint32), ("padding0", C.c_uint32), ("padding1", C.c_uint32), ("padding2", C.c_uint32)]


class OceanBuffer(C.Structure):
    """gr_ocean_buffer: a storage buffer, device pointer and size."""
    _fields_ = [("ptr", C.c_void_p), ("size_bytes", C.c_uint64)]


OCEAN_MAX_LOD_INDIRECT = 8


# gr_meshlet_decode: decode flags, mesh styles, and the argument blocks
MESHLET_DECODE_UNROLLED_MESH, MESHLET_DECODE_INDEX_16 = 1, 2
MESHLET_STYLE_WIREFRAME, MESHLET_STYLE_TEXTURED, MESHLET_STYLE_SKINNED = 0, 1, 2


class PushMeshletDecode(C.Structure):
    """gr_push_meshlet_decode: the Registers block of decode/meshlet_decode.comp."""
    _fields_ = [("primitive_offset", C.c_uint32), ("vertex_offset", C.c_uint32), ("meshlet_count", C.c_uint32), ("wg_offset", C.c_uint32)]


class MeshletDecodeArgs(C.Structure):
    """gr_meshlet_decode_args: device pointers, capacities in elements."""
    _fields_ = [("streams", C.c_void_p), ("payload", C.c_void_p), ("payload_words", C.c_uint32), ("stream_count", C.c_uint32), ("offsets", C.c_void_p),
                ("indices", C.c_void_p), ("index_capacity", C.c_uint64), ("positions", C.c_void_p), ("position_capacity", C.c_uint64),
                ("attributes", C.c_void_p), ("attribute_capacity", C.c_uint64), ("skin", C.c_void_p), ("skin_capacity", C.c_uint64),
                ("target_style", C.c_uint32), ("flags", C.c_uint32)]


# gr_meshlet_cull: flags and the records of meshlet_cull.comp
MESHLET_CULL_ORTHO, MESHLET_CULL_SKINNED, MESHLET_CULL_FORCE_VISIBLE = 1, 2, 4


class PushMeshletCull(C.Structure):
    """gr_push_meshlet_cull: the Registers block of meshlet_cull.comp."""
    _fields_ = [("offset", C.c_uint32), ("count", C.c_uint32), ("mdi_count_offset", C.c_uint32), ("draw_indirect_offset", C.c_uint32)]


class MeshletTask(C.Structure):
    """gr_meshlet_task: MeshAssetDrawTaskInfo."""
    _fields_ = [("aabb_instance", C.c_uint32), ("occluder_state_offset", C.c_uint32), ("node_instance", C.c_uint32), ("mesh_index_count", C.c_uint32),
                ("material_flags", C.c_uint32)]


class MeshletAABB(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("pad0", C.c_float), ("hi", C.c_float * 3), ("pad1", C.c_float)]


class MeshletBound(C.Structure):
    """gr_meshlet_bound: Meshlet::Bound."""
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("cone_axis_cutoff", C.c_float * 4)]


class MatAffine(C.Structure):
    """gr_mat_affine: three rows of a 3 x 4 matrix."""
    _fields_ = [("rows", (C.c_float * 4) * 3)]


class MeshletDraw(C.Structure):
    """gr_meshlet_draw: RuntimeHeaderDecodedMDI."""
    _fields_ = [("index_count", C.c_uint32), ("first_index", C.c_uint32), ("vertex_offset", C.c_int32)]


class MeshletFrustum(C.Structure):
    """gr_meshlet_frustum: the std140 Frustum block of inc/meshlet_ubos.h, 224 bytes."""
    _fields_ = [("viewport", C.c_float * 4), ("planes", (C.c_float * 4) * 6), ("view", C.c_float * 16), ("viewport_scale_bias", C.c_float * 4),
                ("hiz_resolution", C.c_int32 * 2), ("winding", C.c_float), ("hiz_min_lod", C.c_int32), ("hiz_max_lod", C.c_int32), ("pad", C.c_uint32 * 3)]


class MeshletCullArgs(C.Structure):
    """gr_meshlet_cull_args: device pointers, counts in elements."""
    _fields_ = [("tasks", C.c_void_p), ("task_count", C.c_uint32), ("aabb_count", C.c_uint32), ("aabbs", C.c_void_p), ("transforms", C.c_void_p),
                ("bounds", C.c_void_p), ("transform_count", C.c_uint32), ("bound_count", C.c_uint32), ("draws", C.c_void_p), ("draw_count", C.c_uint32),
                ("occluder_count", C.c_uint32), ("occluders", C.c_void_p), ("output", C.c_void_p), ("output_dwords", C.c_uint64), ("chain", C.c_void_p),
                ("chain_width", C.c_uint32), ("chain_height", C.c_uint32), ("chain_levels", C.c_uint32), ("phase", C.c_uint32), ("flags", C.c_uint32),
                ("camera_position", C.c_float * 3), ("frustum", MeshletFrustum)]


# gr_cacao_*: FFX_CACAO_Quality values taken, limits, and the VkFormat values of two intermediates no Image argument takes
CACAO_QUALITY_HIGH, CACAO_QUALITY_HIGHEST = 3, 4
CACAO_MAX_BLUR_PASSES = 8
CACAO_MAX_EXTENT = 16384
CACAO_FORMAT_R8G8B8A8_SNORM, CACAO_FORMAT_R32_UINT = 38, 98
CACAO_INTERMEDIATE_COUNT = 7


class CacaoSettings(C.Structure):
    """gr_cacao_settings: FFX_CACAO_Settings."""
    _fields_ = [("radius", C.c_float), ("shadow_multiplier", C.c_float), ("shadow_power", C.c_float), ("shadow_clamp", C.c_float),
                ("horizon_angle_threshold", C.c_float), ("fade_out_from", C.c_float), ("fade_out_to", C.c_float), ("quality_level", C.c_uint32),
                ("adaptive_quality_limit", C.c_float), ("blur_pass_count", C.c_uint32), ("sharpness", C.c_float),
                ("temporal_supersampling_angle_offset", C.c_float), ("temporal_supersampling_radius_offset", C.c_float),
                ("detail_shadow_strength", C.c_float), ("generate_normals", C.c_uint32), ("bilateral_sigma_squared", C.c_float),
                ("bilateral_similarity_distance_sigma", C.c_float)]


class CacaoConstants(C.Structure):
    """gr_cacao_constants: FFX_CACAO_Constants, the shaders' constant buffer."""
    _f2 = C.c_float * 2
    _fields_ = [("DepthUnpackConsts", _f2), ("CameraTanHalfFOV", _f2), ("NDCToViewMul", _f2), ("NDCToViewAdd", _f2), ("DepthBufferUVToViewMul", _f2),
                ("DepthBufferUVToViewAdd", _f2), ("EffectRadius", C.c_float), ("EffectShadowStrength", C.c_float), ("EffectShadowPow", C.c_float),
                ("EffectShadowClamp", C.c_float), ("EffectFadeOutMul", C.c_float), ("EffectFadeOutAdd", C.c_float),
                ("EffectHorizonAngleThreshold", C.c_float), ("EffectSamplingRadiusNearLimitRec", C.c_float), ("DepthPrecisionOffsetMod", C.c_float),
                ("NegRecEffectRadius", C.c_float), ("LoadCounterAvgDiv", C.c_float), ("AdaptiveSampleCountLimit", C.c_float), ("InvSharpness", C.c_float),
                ("PassIndex", C.c_int32), ("BilateralSigmaSquared", C.c_float), ("BilateralSimilarityDistanceSigma", C.c_float),
                ("PatternRotScaleMatrices", (C.c_float * 4) * 5), ("NormalsUnpackMul", C.c_float), ("NormalsUnpackAdd", C.c_float),
                ("DetailAOStrength", C.c_float), ("Dummy0", C.c_float), ("SSAOBufferDimensions", _f2), ("SSAOBufferInverseDimensions", _f2),
                ("DepthBufferDimensions", _f2), ("DepthBufferInverseDimensions", _f2), ("DepthBufferOffset", C.c_int32 * 2),
                ("PerPassFullResUVOffset", _f2), ("InputOutputBufferDimensions", _f2), ("InputOutputBufferInverseDimensions", _f2),
                ("ImportanceMapDimensions", _f2), ("ImportanceMapInverseDimensions", _f2), ("DeinterleavedDepthBufferDimensions", _f2),
                ("DeinterleavedDepthBufferInverseDimensions", _f2), ("DeinterleavedDepthBufferOffset", _f2),
                ("DeinterleavedDepthBufferNormalisedOffset", _f2), ("NormalsWorldToViewspaceMatrix", (C.c_float * 4) * 4)]


class CacaoBufferSizes(C.Structure):
    """gr_cacao_buffer_sizes: FFX_CACAO_BufferSizeInfo."""
    _fields_ = [(name, C.c_uint32) for name in (
        "inputOutputBufferWidth", "inputOutputBufferHeight", "ssaoBufferWidth", "ssaoBufferHeight", "depthBufferXOffset", "depthBufferYOffset",
        "depthBufferWidth", "depthBufferHeight", "deinterleavedDepthBufferXOffset", "deinterleavedDepthBufferYOffset",
        "deinterleavedDepthBufferWidth", "deinterleavedDepthBufferHeight", "importanceMapWidth", "importanceMapHeight",
        "downsampledSsaoBufferWidth", "downsampledSsaoBufferHeight")]


class CacaoIntermediate(C.Structure):
    """gr_cacao_intermediate: one intermediate of the workspace."""
    _fields_ = [("name", C.c_char * 32), ("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("layers", C.c_uint32),
                ("mips", C.c_uint32), ("mip_offset", C.c_uint64 * 4), ("bytes", C.c_uint64)]


class TimingEntry(C.Structure):
    _fields_ = [("name", C.c_char_p), ("count", C.c_uint64), ("total_ms", C.c_double)]


class PushBloomThreshold(C.Structure):
    _fields_ = [("threads", C.c_uint32 * 2), ("inv_output_size", C.c_float * 2)]


class PushBloomDownsample(C.Structure):
    _fields_ = [("threads", C.c_uint32 * 2), ("inv_output_size", C.c_float * 2), ("inv_input_size", C.c_float * 2),
                ("lerp", C.c_float)]


class PushBloomUpsample(C.Structure):
    _fields_ = [("threads", C.c_uint32 * 2), ("inv_output_size", C.c_float * 2), ("inv_input_size", C.c_float * 2)]


class PushLuminance(C.Structure):
    _fields_ = [("size", C.c_uint32 * 2), ("lerp", C.c_float), ("min_loglum", C.c_float), ("max_loglum", C.c_float)]


class BloomPyramidArgs(C.Structure):
    _fields_ = [("hdr", Image), ("threshold", Image), ("d0", Image), ("d1", Image), ("d2", Image), ("d3", Image), ("history", Image),
                ("u2", Image), ("u1", Image), ("u0", Image), ("lum", C.c_void_p), ("push_threshold", PushBloomThreshold),
                ("push_d0", PushBloomDownsample), ("push_d1", PushBloomDownsample), ("push_d2", PushBloomDownsample), ("push_d3", PushBloomDownsample),
                ("push_u2", PushBloomUpsample), ("push_u1", PushBloomUpsample), ("push_u0", PushBloomUpsample), ("push_luminance", PushLuminance)]


# The push blocks of the bloom chain, filled as host/post/hdr.cpp fills them; `out` / `src` / `d3`: anything with a width and a height
# (a DeviceImage, an Image descriptor).
def threshold_push(out) -> PushBloomThreshold:
    return PushBloomThreshold((out.width, out.height), (1.0 / out.width, 1.0 / out.height))


def downsample_push(out, src, lerp: float = 0.0) -> PushBloomDownsample:
    return PushBloomDownsample((out.width, out.height), (1.0 / out.width, 1.0 / out.height), (1.0 / src.width, 1.0 / src.height), lerp)


def upsample_push(out, src) -> PushBloomUpsample:
    return PushBloomUpsample((out.width, out.height), (1.0 / out.width, 1.0 / out.height), (1.0 / src.width, 1.0 / src.height))


def luminance_push(d3, lerp: float, min_loglum: float = -3.0, max_loglum: float = 2.0) -> PushLuminance:
    return PushLuminance((d3.width // 2, d3.height // 2), lerp, min_loglum, max_loglum)


def pyramid_args(hdr: Image, levels: dict, history: Image, feedback_lerp: float, lum_ptr=None, lum_lerp: float = 0.0) -> BloomPyramidArgs:
    """gr_bloom_pyramid's argument block from the Image descriptors of the frame (levels: threshold, d0..d3, u2..u0 by name)."""
    l, a = levels, BloomPyramidArgs()
    a.hdr, a.history, a.lum = hdr, history, lum_ptr
    for name in ("threshold", "d0", "d1", "d2", "d3", "u2", "u1", "u0"):
        setattr(a, name, l[name])
    a.push_threshold = threshold_push(l["threshold"])
    a.push_d0, a.push_d1 = downsample_push(l["d0"], l["threshold"]), downsample_push(l["d1"], l["d0"])
    a.push_d2, a.push_d3 = downsample_push(l["d2"], l["d1"], feedback_lerp), downsample_push(l["d3"], l["d2"], feedback_lerp)
    a.push_u2, a.push_u1, a.push_u0 = upsample_push(l["u2"], l["d3"]), upsample_push(l["u1"], l["u2"]), upsample_push(l["u0"], l["u1"])
    if lum_ptr is not None:
        a.push_luminance = luminance_push(l["d3"], lum_lerp)
    return a


class PushTonemap(C.Structure):
    _fields_ = [("dynamic_exposure", C.c_float)]


class ClusterParams(C.Structure):
    _fields_ = [("transform", C.c_float * 16), ("clip_scale", C.c_float * 4), ("camera_base", C.c_float * 3),
                ("pad0", C.c_float), ("camera_front", C.c_float * 3), ("pad1", C.c_float), ("xy_scale", C.c_float * 2),
                ("resolution_xy", C.c_int32 * 2), ("inv_resolution_xy", C.c_float * 2), ("num_lights", C.c_int32),
                ("num_lights_32", C.c_int32), ("num_decals", C.c_int32), ("num_decals_32", C.c_int32),
                ("decals_texture_offset", C.c_int32), ("z_max_index", C.c_int32), ("z_scale", C.c_float),
                ("pad2", C.c_float * 3)]


assert C.sizeof(ClusterParams) == 176


class PushSpotTransform(C.Structure):
    _fields_ = [("vp", C.c_float * 16), ("camera_pos", C.c_float * 3), ("num_lights", C.c_uint32),
                ("camera_front", C.c_float * 3), ("z_near", C.c_float), ("z_far", C.c_float)]


assert C.sizeof(PushSpotTransform) == 100


class DecalTexture(C.Structure):
    """gr_decal_texture: an RGBA8 mip chain in device memory, levels tightly packed one after another."""
    _fields_ = [("levels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("num_levels", C.c_uint32), ("format", C.c_uint32)]


class DecalApplyArgs(C.Structure):
    """gr_decal_apply_args."""
    _fields_ = [("albedo", Image), ("depth", Image), ("inv_view_projection", C.c_float * 16), ("cluster", ClusterParams), ("transforms", C.c_void_p),
                ("bitmask_decal", C.c_void_p), ("range_decal", C.c_void_p), ("textures", C.c_void_p), ("num_textures", C.c_uint32), ("pad0", C.c_uint32)]


assert C.sizeof(DecalTexture) == 24 and C.sizeof(DecalApplyArgs) == 328
MAX_DECALS_BINDLESS = 4096


class SkyArgs(C.Structure):
    """gr_sky_args: the cube is absent when its ptr, size and levels are all 0."""
    _fields_ = [("emissive", Image), ("depth", Image), ("inv_local_view_projection", C.c_float * 16), ("color", C.c_float * 3), ("camera_height", C.c_float),
                ("sun_direction", C.c_float * 3), ("pad0", C.c_float), ("cube", Cube)]


class SkyCubeParams(C.Structure):
    """gr_sky_cube_params: volumetric_light_setup_sky.comp's UBO, less inv_resolution (1 / size, formed by the launcher)."""
    _fields_ = [("sun_color", C.c_float * 3), ("camera_y", C.c_float), ("sun_direction", C.c_float * 3), ("pad0", C.c_float)]


assert C.sizeof(SkyArgs) == 160 and C.sizeof(SkyCubeParams) == 32


class PushClusterSetup(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("num_lights", C.c_uint32)]


class PushZRange(C.Structure):
    _fields_ = [("num_volumes", C.c_uint32), ("num_volumes_128", C.c_uint32), ("num_ranges", C.c_uint32)]


class ClusterFrontArgs(C.Structure):
    """gr_cluster_front_args (include/granite_hip.h): uploads + spot_transform + setup + z_range as one launch."""
    _fields_ = [("transforms", C.c_void_p), ("src_lights", C.c_void_p), ("src_models", C.c_void_p), ("src_type_mask", C.c_void_p),
                ("transformed_spots", C.c_void_p), ("cull_setup", C.c_void_p), ("params", C.c_void_p), ("spot_push", C.c_void_p),
                ("setup_push", C.c_void_p), ("src_ranges", C.c_void_p), ("light_ranges", C.c_void_p), ("range_out", C.c_void_p),
                ("z_push", C.c_void_p)]


class PushDirectional(C.Structure):
    _fields_ = [("inv_view_proj_col2", C.c_float * 4), ("color", C.c_float * 3), ("environment_intensity", C.c_float),
                ("camera_pos", C.c_float * 3), ("environment_mipscale", C.c_float), ("direction", C.c_float * 3),
                ("cascade_log_bias", C.c_float), ("camera_front", C.c_float * 3), ("pad0", C.c_float),
                ("inv_resolution", C.c_float * 2), ("pad1", C.c_float * 2)]


class PushClustering(C.Structure):
    _fields_ = [("inv_view_proj_col2", C.c_float * 4), ("camera_pos", C.c_float * 3), ("pad0", C.c_float),
                ("inv_resolution", C.c_float * 2), ("pad1", C.c_float * 2)]


class LightingArgs(C.Structure):
    _fields_ = [("albedo", Image), ("normal", Image), ("pbr", Image), ("depth", Image), ("emissive", Image),
                ("hdr", Image),
                ("inv_view_projection", C.c_float * 16), ("directional", PushDirectional), ("clustering", PushClustering),
                ("cluster", ClusterParams), ("transforms", C.c_void_p), ("bitmask", C.c_void_p), ("range", C.c_void_p),
                ("flags", C.c_uint32), ("rows", C.c_uint32 * 2), ("ambient_occlusion", Image),
                ("fog_color", C.c_float * 3), ("fog_falloff", C.c_float)]


SHADOW_PCF, SHADOW_PCF_WIDE, SHADOW_VSM = 1, 2, 3
SHADOW_NUM_CASCADES = 4


class DirectionalLightArgs(C.Structure):
    """gr_directional_light_args: the shadowed directional quad; layers 1 (transforms[0] alone) or 4 (SHADOW_CASCADES)."""
    _fields_ = [("albedo", Image), ("normal", Image), ("pbr", Image), ("depth", Image), ("emissive", Image), ("hdr", Image),
                ("inv_view_projection", C.c_float * 16), ("directional", PushDirectional), ("flags", C.c_uint32), ("mode", C.c_uint32),
                ("layers", C.c_uint32), ("pad0", C.c_uint32), ("ambient_occlusion", Image), ("shadow_maps", Image * SHADOW_NUM_CASCADES),
                ("transforms", (C.c_float * 16) * SHADOW_NUM_CASCADES)]


assert C.sizeof(DirectionalLightArgs) == 696


class Rows(C.Structure):
    """gr_rows: render area of one launch, output rows [first, first + count).  Passed by pointer: None (NULL) = the whole image,
    count == 0 = NO rows (the launcher returns GR_OK without launching: an empty band must not touch the image).  The one embedded
    use, LightingArgs.rows, keeps {0, 0} = whole target, as a zero-initialised argument struct has it (include/granite_hip.h)."""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32)]


class UploadRange(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("src_pinned", C.c_void_p), ("bytes", C.c_size_t)]


class PushFxaa(C.Structure):
    _fields_ = [("inv_resolution", C.c_float * 2)]


class PushSmaa(C.Structure):
    _fields_ = [("rt_metrics", C.c_float * 4)]


class PushTaa(C.Structure):
    _fields_ = [("reproj", C.c_float * 16), ("rt_metrics", C.c_float * 4)]


assert C.sizeof(PushTaa) == 80


class HizArgs(C.Structure):
    _fields_ = [("depth", Image), ("chain", C.c_void_p), ("chain_width", C.c_uint32), ("chain_height", C.c_uint32),
                ("chain_levels", C.c_uint32), ("output_downsample", C.c_uint32), ("z_transform", C.c_float * 4),
                ("counter", C.c_void_p)]


class SsrArgs(C.Structure):
    _fields_ = [("depth_chain", C.c_void_p), ("chain_width", C.c_uint32), ("chain_height", C.c_uint32), ("chain_levels", C.c_uint32),
                ("pbr", Image), ("normal", Image), ("light", Image), ("dither_lut", C.c_void_p), ("frame", C.c_uint32),
                ("view_projection", C.c_float * 16), ("inv_view_projection", C.c_float * 16), ("camera_position", C.c_float * 3),
                ("output", Image), ("ray_length", Image), ("ray_confidence", Image), ("ray_list", C.c_void_p), ("ray_counter", C.c_void_p),
                ("scratch", C.c_void_p)]


class SsrApplyArgs(C.Structure):
    _fields_ = [("hdr", Image), ("reflected", Image), ("albedo", Image), ("normal", Image), ("pbr", Image), ("depth", Image),
                ("brdf_lut", Image), ("inv_view_projection", C.c_float * 16), ("camera_position", C.c_float * 3)]


class SpdArgs(C.Structure):
    _fields_ = [("input", Image), ("chain", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("mips", C.c_uint32),
                ("components", C.c_uint32), ("reduction_mode", C.c_uint32), ("filter_mods", C.c_void_p)]


SPD_REDUCTION_COLOR, SPD_REDUCTION_DEPTH = 0, 1


class PushPq10(C.Structure):
    _fields_ = [("primary_conversion", C.c_float * 16), ("hdr_pre_exposure", C.c_float), ("ui_pre_exposure", C.c_float),
                ("max_light_level", C.c_float), ("inv_max_light_level", C.c_float)]


class GraniteHipError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """dlopen the in-tree libgranite_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GraniteHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp = C.c_void_p
    sigs = {
        "gr_abi_version": (C.c_int, []),
        "gr_create": (vp, [C.c_int]),
        "gr_destroy": (None, [vp]),
        "gr_last_error": (C.c_char_p, [vp]),
        "gr_sync": (C.c_int, [vp, vp]),
        "gr_alloc": (C.c_int, [vp, C.c_size_t, P(vp)]),
        "gr_free": (C.c_int, [vp, vp]),
        "gr_upload": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
        "gr_download": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
        "gr_copy": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
        "gr_fill_zero": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "gr_timing_enable": (C.c_int, [vp, C.c_int]),
        "gr_timing_set_filter": (C.c_int, [vp, C.c_char_p]),
        "gr_timing_set_sampling": (C.c_int, [vp, C.c_uint32]),
        "gr_timing_max_ms": (C.c_int, [vp, C.c_char_p, vp]),
        "gr_timing_span_begin": (C.c_int, [vp, vp, C.c_char_p, vp]),
        "gr_timing_span_end": (C.c_int, [vp, vp, vp]),
        "gr_bandwidth_probe": (C.c_int, [vp, C.c_size_t, C.c_int, P(C.c_double), P(C.c_double)]),
        "gr_timing_reset": (C.c_int, [vp]),
        "gr_timing_query": (C.c_int, [vp, P(TimingEntry), C.c_int]),
        "gr_bloom_threshold": (C.c_int, [vp, vp, P(Image), P(Image), vp, P(PushBloomThreshold)]),
        "gr_bloom_downsample": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(PushBloomDownsample)]),
        "gr_bloom_upsample": (C.c_int, [vp, vp, P(Image), P(Image), P(PushBloomUpsample)]),
        "gr_luminance": (C.c_int, [vp, vp, P(Image), vp, P(PushLuminance)]),
        "gr_ssr_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
        "gr_ssr_trace": (C.c_int, [vp, vp, P(SsrArgs)]),
        "gr_ssr_apply": (C.c_int, [vp, vp, P(SsrApplyArgs)]),
        "gr_bloom_tail_supported": (C.c_int, [P(Image), P(Image), P(Image), P(Image), P(Image), P(PushBloomDownsample), P(PushBloomDownsample),
                                              P(PushBloomUpsample), P(PushBloomUpsample)]),
        "gr_bloom_down_tail": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(Image), P(PushBloomDownsample), P(PushBloomDownsample)]),
        "gr_bloom_down_mid_supported": (C.c_int, [P(Image), P(Image), P(Image), P(PushBloomDownsample), P(PushBloomDownsample)]),
        "gr_bloom_down_mid": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(PushBloomDownsample), P(PushBloomDownsample), P(Rows)]),
        "gr_bloom_down_head_supported": (C.c_int, [P(Image), P(Image), P(Image), P(Image), P(PushBloomThreshold), P(PushBloomDownsample), P(PushBloomDownsample)]),
        "gr_bloom_down_head": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(Image), vp, P(PushBloomThreshold), P(PushBloomDownsample), P(PushBloomDownsample)]),
        "gr_bloom_pyramid_supported": (C.c_int, [P(BloomPyramidArgs)]),
        "gr_bloom_pyramid": (C.c_int, [vp, vp, P(BloomPyramidArgs)]),
        "gr_debug_pyramid_giveups": (C.c_int, [vp, P(C.c_uint32)]),
        "gr_bloom_up_all_supported": (C.c_int, [P(Image), P(Image), P(Image), P(Image), P(PushBloomUpsample), P(PushBloomUpsample), P(PushBloomUpsample)]),
        "gr_bloom_up_all": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(Image), vp, P(PushBloomUpsample), P(PushBloomUpsample), P(PushBloomUpsample),
                                      P(PushLuminance), C.c_uint32]),
        "gr_bloom_up_tail": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), vp, P(PushBloomUpsample), P(PushBloomUpsample), P(PushLuminance)]),
        "gr_tonemap": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), vp, P(PushTonemap)]),
        "gr_bloom_threshold_rows": (C.c_int, [vp, vp, P(Image), P(Image), vp, P(PushBloomThreshold), P(Rows)]),
        "gr_bloom_downsample_rows": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(PushBloomDownsample), P(Rows)]),
        "gr_bloom_upsample_rows": (C.c_int, [vp, vp, P(Image), P(Image), P(PushBloomUpsample), P(Rows)]),
        "gr_tonemap_rows": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), vp, P(PushTonemap), P(Rows)]),
        "gr_upload_batch": (C.c_int, [vp, vp, P(UploadRange), C.c_uint32]),
        "gr_alloc_host": (C.c_int, [vp, C.c_size_t, P(vp)]),
        "gr_free_host": (C.c_int, [vp, vp]),
        "gr_cluster_spot_transform": (C.c_int, [vp, vp, vp, vp, P(PushSpotTransform)]),
        "gr_cluster_setup": (C.c_int, [vp, vp, vp, vp, vp, P(ClusterParams), P(PushClusterSetup)]),
        "gr_cluster_binning": (C.c_int, [vp, vp, vp, vp, vp, P(ClusterParams)]),
        "gr_cluster_z_range": (C.c_int, [vp, vp, vp, vp, P(PushZRange)]),
        "gr_cluster_front": (C.c_int, [vp, vp, P(ClusterFrontArgs)]),
        "gr_alloc_host": (C.c_int, [vp, C.c_size_t, P(vp)]),
        "gr_free_host": (C.c_int, [vp, vp]),
        "gr_lighting": (C.c_int, [vp, vp, P(LightingArgs)]),
        "gr_smaa_set_luts": (C.c_int, [vp, vp, vp]),
        "gr_fxaa": (C.c_int, [vp, vp, P(Image), P(Image), P(PushFxaa)]),
        "gr_blit": (C.c_int, [vp, vp, P(Image), P(Image), C.c_int]),
        "gr_smaa_edge_detection": (C.c_int, [vp, vp, P(Image), P(Image), P(PushSmaa), C.c_int]),
        "gr_smaa_blend_weight": (C.c_int, [vp, vp, P(Image), P(Image), P(PushSmaa), C.c_int]),
        "gr_smaa_neighbor_blend": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(PushSmaa)]),
        "gr_taa_resolve": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(Image), P(Image), P(Image), P(PushTaa), C.c_int]),
        "gr_hiz": (C.c_int, [vp, vp, P(HizArgs)]),
        "gr_fill_byte": (C.c_int, [vp, vp, vp, C.c_int, C.c_size_t]),
        "gr_fill_u32": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_size_t]),
        "gr_get_device_info": (C.c_int, [vp, C.c_char_p, C.c_size_t, vp]),
        "gr_spd_downsample": (C.c_int, [vp, vp, P(SpdArgs)]),
        "gr_debug_mix": (C.c_int, [vp, vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32]),
        "gr_pack_b10g11r11": (C.c_int, [vp, vp, vp, vp, C.c_uint32]),
        "gr_pq10_encode": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(PushPq10)]),
        "gr_fsr_upscale": (C.c_int, [vp, vp, P(Image), P(Image), C.c_int]),
        "gr_video_scale": (C.c_int, [vp, vp, P(Image), P(Image), C.c_uint32, C.c_uint32, C.c_uint32]),
        "gr_video_scale_plan": (C.c_int, [P(Image), P(Image), C.c_uint32, C.c_uint32, C.c_uint32, P(VideoPlan)]),
        "gr_video_scaler_weights": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint16)]),
        "gr_video_yuv_to_rgb": (C.c_int, [vp, vp, P(Image), C.c_uint32, P(Image), P(VideoYuvInfo)]),
        "gr_video_yuv_plan": (C.c_int, [P(Image), C.c_uint32, P(Image), P(VideoYuvInfo), P(VideoYuvPlan)]),
        "gr_texture_decoded_format": (C.c_uint32, [C.c_uint32]),
        "gr_texture_block_bytes": (C.c_uint32, [C.c_uint32]),
        "gr_texture_block_dim": (C.c_int, [C.c_uint32, P(C.c_uint32), P(C.c_uint32)]),
        "gr_texture_block_info": (C.c_int, [C.c_uint32, P(C.c_uint32), P(C.c_uint32)]),
        "gr_texture_decode": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint32, P(Image)]),
        "gr_texture_encode_supported": (C.c_int, [C.c_uint32, C.c_uint32]),
        "gr_texture_encode": (C.c_int, [vp, vp, C.c_uint32, P(Image), vp, C.c_uint32]),
        "gr_texture_generate_mipmap": (C.c_int, [vp, vp, P(Image), P(Image)]),
        "gr_cube_chain_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32]),
        "gr_cube_chain_offset": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32]),
        "gr_env_equirect_to_cube": (C.c_int, [vp, vp, P(Image), vp, C.c_uint32, C.c_uint32]),
        "gr_env_specular": (C.c_int, [vp, vp, P(Cube), vp, C.c_uint32, C.c_uint32]),
        "gr_env_diffuse": (C.c_int, [vp, vp, P(Cube), vp, C.c_uint32]),
        "gr_fft_describe": (C.c_int, [P(FftOptions), P(FftPass), C.c_uint32]),
        "gr_fft_plan_create": (C.c_int, [vp, P(FftOptions), P(vp)]),
        "gr_fft_plan_destroy": (None, [vp, vp]),
        "gr_fft_plan_iterations": (C.c_uint32, [vp]),
        "gr_fft_execute": (C.c_int, [vp, vp, vp, P(FftResource), P(FftResource)]),
        "gr_fft_execute_iteration": (C.c_int, [vp, vp, vp, P(FftResource), P(FftResource), C.c_uint32]),
        "gr_ocean_generate_fft": (C.c_int, [vp, vp, vp, vp, P(PushOceanGenerate), C.c_uint32, P(C.c_float)]),
        "gr_ocean_bake_maps": (C.c_int, [vp, vp, P(Image), P(Image), P(Image), P(Image), P(PushOceanBake)]),
        "gr_ocean_mipmap": (C.c_int, [vp, vp, P(Image), P(Image), P(PushOceanMipmap)]),
        "gr_ocean_update_lod": (C.c_int, [vp, vp, P(Image), P(PushOceanUpdateLod)]),
        "gr_ocean_init_counter_buffer": (C.c_int, [vp, vp, P(OceanBuffer), P(C.c_uint32)]),
        "gr_ocean_cull_blocks": (C.c_int, [vp, vp, P(Image), C.c_uint32, P(OceanBuffer), P(OceanBuffer), P(PushOceanCull), P(C.c_float)]),
        "gr_meshlet_decode": (C.c_int, [vp, vp, P(MeshletDecodeArgs), P(PushMeshletDecode)]),
        "gr_meshlet_cull": (C.c_int, [vp, vp, P(MeshletCullArgs), P(PushMeshletCull)]),
        "gr_cluster_binning_decal": (C.c_int, [vp, vp, vp, vp, P(ClusterParams)]),
        "gr_decal_apply": (C.c_int, [vp, vp, P(DecalApplyArgs)]),
        "gr_sky_apply": (C.c_int, [vp, vp, P(SkyArgs)]),
        "gr_sky_cube": (C.c_int, [vp, vp, vp, C.c_uint32, P(SkyCubeParams)]),
        "gr_directional_light": (C.c_int, [vp, vp, P(DirectionalLightArgs)]),
        "gr_vsm_moments": (C.c_int, [vp, vp, P(Image), P(Image)]),
        "gr_vsm_blur": (C.c_int, [vp, vp, P(Image), P(Image), C.c_int]),
        "gr_cacao_reference_settings": (None, [P(CacaoSettings)]),
        "gr_cacao_update_buffer_sizes": (C.c_int, [C.c_uint32, C.c_uint32, P(CacaoBufferSizes)]),
        "gr_cacao_update_constants": (C.c_int, [vp, P(CacaoConstants), P(CacaoSettings), P(CacaoBufferSizes), P(C.c_float), P(C.c_float)]),
        "gr_cacao_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
        "gr_cacao_workspace_describe": (C.c_int, [C.c_uint32, C.c_uint32, P(CacaoIntermediate), C.c_uint32]),
        "gr_cacao_prepare_depths": (C.c_int, [vp, vp, P(Image), vp, P(CacaoConstants)]),
        "gr_cacao_prepare_normals": (C.c_int, [vp, vp, P(Image), vp, P(CacaoConstants)]),
        "gr_cacao_generate_base": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, P(CacaoConstants)]),
        "gr_cacao_importance_generate": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, P(CacaoConstants)]),
        "gr_cacao_importance_postprocess_a": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, P(CacaoConstants)]),
        "gr_cacao_importance_postprocess_b": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, P(CacaoConstants)]),
        "gr_cacao_generate": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, P(CacaoConstants), C.c_uint32]),
        "gr_cacao_blur": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, P(CacaoConstants), C.c_uint32]),
        "gr_cacao_apply": (C.c_int, [vp, vp, vp, P(Image), P(CacaoConstants), C.c_uint32]),
        "gr_fsr_sharpen": (C.c_int, [vp, vp, P(Image), P(Image), C.c_float]),
        "gr_mip_chain_offset": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "gr_mip_chain_size": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "gr_abi_version", "gr_create", "gr_destroy", "gr_last_error", "gr_sync", "gr_alloc", "gr_free", "gr_upload",
    "gr_download", "gr_copy", "gr_fill_zero", "gr_upload_batch", "gr_alloc_host", "gr_free_host", "gr_timing_enable", "gr_timing_set_filter", "gr_timing_reset", "gr_timing_query",
    "gr_bloom_threshold", "gr_bloom_downsample", "gr_bloom_upsample", "gr_luminance", "gr_tonemap",
    "gr_bloom_threshold_rows", "gr_bloom_downsample_rows", "gr_bloom_upsample_rows", "gr_tonemap_rows",
    "gr_cluster_spot_transform", "gr_cluster_setup", "gr_cluster_binning", "gr_cluster_z_range", "gr_cluster_front", "gr_lighting",
    "gr_smaa_set_luts", "gr_fxaa", "gr_blit", "gr_smaa_edge_detection", "gr_smaa_blend_weight", "gr_smaa_neighbor_blend", "gr_taa_resolve",
    "gr_hiz", "gr_mip_chain_offset", "gr_mip_chain_size", "gr_fsr_upscale", "gr_fsr_sharpen", "gr_fill_byte", "gr_fill_u32", "gr_pq10_encode", "gr_get_device_info", "gr_spd_downsample", "gr_debug_mix", "gr_pack_b10g11r11",
    "gr_video_scale", "gr_video_scale_plan", "gr_video_scaler_weights", "gr_video_yuv_to_rgb", "gr_video_yuv_plan",
    "gr_texture_decoded_format", "gr_texture_block_bytes", "gr_texture_block_dim", "gr_texture_block_info", "gr_texture_decode",
    "gr_texture_encode_supported", "gr_texture_encode", "gr_texture_generate_mipmap",
    "gr_cube_chain_bytes", "gr_cube_chain_offset", "gr_env_equirect_to_cube", "gr_env_specular", "gr_env_diffuse",
    "gr_fft_describe", "gr_fft_plan_create", "gr_fft_plan_destroy", "gr_fft_plan_iterations", "gr_fft_execute", "gr_fft_execute_iteration",
    "gr_ocean_generate_fft", "gr_ocean_bake_maps", "gr_ocean_mipmap", "gr_ocean_update_lod", "gr_ocean_init_counter_buffer", "gr_ocean_cull_blocks",
    "gr_meshlet_decode", "gr_meshlet_cull", "gr_cluster_binning_decal", "gr_decal_apply", "gr_sky_apply", "gr_sky_cube",
    "gr_directional_light", "gr_vsm_moments", "gr_vsm_blur",
    "gr_cacao_reference_settings", "gr_cacao_update_buffer_sizes", "gr_cacao_update_constants", "gr_cacao_workspace_bytes", "gr_cacao_workspace_describe",
    "gr_cacao_prepare_depths", "gr_cacao_prepare_normals", "gr_cacao_generate_base", "gr_cacao_importance_generate",
    "gr_cacao_importance_postprocess_a", "gr_cacao_importance_postprocess_b", "gr_cacao_generate", "gr_cacao_blur", "gr_cacao_apply",
]


def cacao_reference_settings() -> CacaoSettings:
    """The FFX_CACAO_Settings setup_ffx_cacao installs (renderer/post/ssao.cpp:73-91)."""
    s = CacaoSettings()
    load_library().gr_cacao_reference_settings(C.byref(s))
    return s


def cacao_constants(width: int, height: int, projection, view, settings: Optional[CacaoSettings] = None, ctx: Optional["Context"] = None):
    """The four per-pass constant blocks (a ctypes array of CacaoConstants) for a width x height frame; projection and view are 16 floats
    each, column-major (RenderParameters::projection and ::view).  Raises on settings the kernels do not take."""
    lib = load_library()
    settings = settings or cacao_reference_settings()
    sizes = CacaoBufferSizes()
    constants = (CacaoConstants * 4)()
    proj = (C.c_float * 16)(*[float(v) for v in np.asarray(projection, np.float32).reshape(16)])
    to_view = (C.c_float * 16)(*[float(v) for v in np.asarray(view, np.float32).reshape(16)])
    code = lib.gr_cacao_update_buffer_sizes(width, height, C.byref(sizes))
    if code == 0:
        code = lib.gr_cacao_update_constants(ctx.handle if ctx else None, constants, C.byref(settings), C.byref(sizes), proj, to_view)
    if code != 0:
        message = lib.gr_last_error(ctx.handle).decode() if ctx else "width, height or settings the SSAO kernels do not take"
        raise GraniteHipError(f"gr_cacao_update_constants failed ({code}): {message}")
    return constants


def cacao_workspace_describe(width: int, height: int) -> Optional[list]:
    """[{name, format, width, height, layers, mips, mip_offset, bytes}] of the workspace, or None for a size that is refused."""
    out = (CacaoIntermediate * CACAO_INTERMEDIATE_COUNT)()
    if load_library().gr_cacao_workspace_describe(width, height, out, CACAO_INTERMEDIATE_COUNT) != 0:
        return None
    return [{"name": d.name.decode(), "format": d.format, "width": d.width, "height": d.height, "layers": d.layers, "mips": d.mips,
             "mip_offset": list(d.mip_offset)[:d.mips], "bytes": d.bytes} for d in out]


def fft_options(nx, ny=1, nz=1, dimensions=1, mode=FFT_FORWARD_C2C, data_type=FFT_FP32, input_resource=FFT_RESOURCE_BUFFER,
                output_resource=FFT_RESOURCE_BUFFER) -> FftOptions:
    return FftOptions(int(nx), int(ny), int(nz), int(dimensions), int(mode), int(data_type), int(input_resource), int(output_resource))


def fft_describe(options: FftOptions):
    """gr_fft_describe (host-only): the pass list of a plan as FftPass entries, or None where gr_fft_plan_create refuses the options."""
    lib = load_library()
    passes = (FftPass * 16)()
    n = lib.gr_fft_describe(C.byref(options), passes, 16)
    return None if n < 0 else [passes[i] for i in range(n)]


def fft_buffer_resource(ptr, size_bytes, row_stride, layer_stride) -> FftResource:
    r = FftResource()
    r.type, r.ptr, r.size_bytes, r.row_stride, r.layer_stride = FFT_RESOURCE_BUFFER, ptr, int(size_bytes), int(row_stride), int(layer_stride)
    return r


def fft_image_resource(image: Image, output_offset=(0, 0)) -> FftResource:
    r = FftResource()
    r.type, r.image = FFT_RESOURCE_TEXTURE, image
    r.output_offset[:] = [int(output_offset[0]), int(output_offset[1])]
    return r


def _video_images(input_size, input_format, planes):
    """gr_image descriptors (null pointers) for the host-only plan: input_size (w, h), planes [(w, h, format), ...]."""
    src = Image(None, int(input_size[0]), int(input_size[1]), int(input_size[0]) * FORMAT_BPP[input_format], int(input_format))
    arr = (Image * max(1, len(planes)))()
    for i, (w, h, fmt) in enumerate(planes):
        arr[i] = Image(None, int(w), int(h), int(w) * FORMAT_BPP[fmt], int(fmt))
    return src, arr


def video_scale_plan(input_size, input_format, planes, input_color_space, output_color_space) -> Optional[dict]:
    """What gr_video_scale would launch (VideoScaler::rescale's decisions), computed on the host; None when it refuses."""
    lib = load_library()
    src, arr = _video_images(input_size, input_format, planes)
    plan = VideoPlan()
    if lib.gr_video_scale_plan(C.byref(src), arr, len(planes), int(input_color_space), int(output_color_space), C.byref(plan)) < 0:
        return None
    return {"flags": plan.flags, "eotf": plan.eotf, "oetf": plan.oetf, "num_planes": plan.num_planes,
            "resolution": tuple(plan.push.resolution), "scaling_to_input": tuple(plan.push.scaling_to_input),
            "inv_input_resolution": tuple(plan.push.inv_input_resolution), "dither_strength": plan.push.dither_strength,
            "gamma_space_transform": np.array(plan.gamma_space_transform[:], dtype=np.float32).reshape(3, 4),
            "primary_transform": np.array(plan.primary_transform[:], dtype=np.float32).reshape(3, 3).T}


def video_scaler_weights(input_width: int, input_height: int, output_width: int, output_height: int) -> np.ndarray:
    """The fp16 weight table of VideoScaler::update_weights as uint16 bits, shape (2, 256, 8): horizontal, vertical."""
    lib = load_library()
    out = np.zeros((2, 256, 8), dtype=np.uint16)
    rc = lib.gr_video_scaler_weights(input_width, input_height, output_width, output_height, out.ctypes.data_as(C.POINTER(C.c_uint16)))
    if rc < 0:
        raise GraniteHipError(f"gr_video_scaler_weights({input_width}, {input_height}, {output_width}, {output_height}) failed")
    return out


def video_yuv_info(bit_depth=8, msb_aligned=0, full_range=0, matrix=VIDEO_MATRIX_BT709, chroma_location=VIDEO_CHROMA_CENTER, pq=0,
                   nv21=0) -> VideoYuvInfo:
    return VideoYuvInfo(int(bit_depth), int(msb_aligned), int(full_range), int(matrix), int(chroma_location), int(pq), int(nv21))


def video_yuv_plan(planes, out, info: VideoYuvInfo) -> Optional[dict]:
    """What gr_video_yuv_to_rgb would launch (init_yuv_to_rgb's UBO and dispatch_conversion's specialization constants), computed on
    the host; None when it refuses.  planes [(w, h, format), ...], out (w, h, format); matrices as (4, 4) indexed [col][row]."""
    lib = load_library()
    _, arr = _video_images((1, 1), FORMAT_R8G8B8A8_UNORM, planes)
    dst = Image(None, int(out[0]), int(out[1]), int(out[0]) * FORMAT_BPP[out[2]], int(out[2]))
    plan = VideoYuvPlan()
    if lib.gr_video_yuv_plan(arr, len(planes), C.byref(dst), C.byref(info), C.byref(plan)) < 0:
        return None
    f = lambda v: np.array(v[:], dtype=np.float32)
    return {"yuv_to_rgb": f(plan.push.yuv_to_rgb).reshape(4, 4), "primary_conversion": f(plan.push.primary_conversion).reshape(4, 4),
            "resolution": tuple(plan.push.resolution), "inv_resolution": tuple(f(plan.push.inv_resolution)),
            "chroma_siting": tuple(f(plan.push.chroma_siting)), "chroma_clamp": tuple(f(plan.push.chroma_clamp)),
            "unorm_rescale": np.float32(plan.push.unorm_rescale), "spec_pq": plan.spec_pq, "spec_num_planes": plan.spec_num_planes,
            "spec_nv21": plan.spec_nv21, "matrix": plan.matrix}


class DeviceBuffer:
    """A zero-initialised HBM allocation owned through gr_alloc/gr_free."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        ctx.check(ctx.lib.gr_alloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, array: np.ndarray, offset: int = 0) -> "DeviceBuffer":
        a = np.ascontiguousarray(array)
        assert offset + a.nbytes <= self.nbytes, (offset, a.nbytes, self.nbytes)
        self.ctx.check(self.ctx.lib.gr_upload(self.ctx.handle, None, self.ptr + offset, a.ctypes.data, a.nbytes))
        self.ctx.sync()
        return self

    def download(self, dtype=np.uint8, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(n, dtype=dt)
        self.ctx.check(self.ctx.lib.gr_download(self.ctx.handle, None, out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.gr_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceImage:
    """A linear row-major attachment in HBM (tight pitch) + its gr_image descriptor."""

    def __init__(self, ctx: "Context", width: int, height: int, fmt: int, ptr: Optional[int] = None):
        self.ctx = ctx
        self.width, self.height, self.format = int(width), int(height), int(fmt)
        self.bpp = FORMAT_BPP[fmt]
        self.pitch = self.width * self.bpp
        self.buffer = None
        if ptr is None:
            self.buffer = DeviceBuffer(ctx, self.pitch * self.height)
            ptr = self.buffer.ptr
        self.ptr = ptr
        self.desc = Image(ptr, self.width, self.height, self.pitch, self.format)

    def upload(self, array: np.ndarray) -> "DeviceImage":
        a = np.ascontiguousarray(array)
        assert a.nbytes == self.pitch * self.height, (a.shape, a.dtype, self.width, self.height, self.bpp)
        self.ctx.check(self.ctx.lib.gr_upload(self.ctx.handle, None, self.ptr, a.ctypes.data, a.nbytes))
        self.ctx.sync()
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.pitch * self.height, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.gr_download(self.ctx.handle, None, out.ctypes.data, self.ptr, out.nbytes))
        if self.format == FORMAT_R16G16B16A16_SFLOAT:
            return out.view(np.uint16).reshape(self.height, self.width, 4)
        if self.format in (FORMAT_R8G8B8A8_SRGB, FORMAT_R8G8B8A8_UNORM, FORMAT_B8G8R8A8_UNORM, FORMAT_B8G8R8A8_SRGB):
            return out.reshape(self.height, self.width, 4)
        if self.format == FORMAT_R8_UNORM:
            return out.reshape(self.height, self.width)
        if self.format == FORMAT_R16_UNORM:
            return out.view(np.uint16).reshape(self.height, self.width)
        if self.format == FORMAT_R16G16_UNORM:
            return out.view(np.uint16).reshape(self.height, self.width, 2)
        if self.format == FORMAT_R8G8_UNORM:
            return out.reshape(self.height, self.width, 2)
        if self.format in (FORMAT_D32_SFLOAT, FORMAT_R32_SFLOAT):
            return out.view(np.float32).reshape(self.height, self.width)
        if self.format in (FORMAT_A2B10G10R10_UNORM_PACK32, FORMAT_B10G11R11_UFLOAT_PACK32):
            return out.view(np.uint32).reshape(self.height, self.width)
        if self.format == FORMAT_R16G16_SFLOAT:
            return out.view(np.uint16).reshape(self.height, self.width, 2)
        if self.format == FORMAT_R16_SFLOAT:
            return out.view(np.uint16).reshape(self.height, self.width)
        return out.reshape(self.height, self.pitch)


class Context:
    """gr_ctx wrapper. `stream` arguments are raw hipStream_t handles (ints) or None for the default stream."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.handle = self.lib.gr_create(device)
        if not self.handle:
            raise GraniteHipError(f"gr_create({device}) failed: no usable HIP device")

    def check(self, code: int):
        if code < 0:
            raise GraniteHipError(f"[{code}] {self.lib.gr_last_error(self.handle).decode()}")
        return code

    def sync(self, stream=None):
        self.check(self.lib.gr_sync(self.handle, stream))

    def close(self):
        if self.handle:
            self.lib.gr_destroy(self.handle)
            self.handle = None

    # ---- timing -----------------------------------------------------------------------------------------------
    def timing_enable(self, enable: bool):
        self.check(self.lib.gr_timing_enable(self.handle, int(enable)))

    def timing_max_ms(self, name: str) -> float:
        """Longest single bracket recorded under `name` since the last reset."""
        out = C.c_double(0.0)
        self.check(self.lib.gr_timing_max_ms(self.handle, name.encode(), C.byref(out)))
        return float(out.value)

    def timing_reset(self):
        self.check(self.lib.gr_timing_reset(self.handle))

    def timing_query(self):
        arr = (TimingEntry * 64)()
        n = self.check(self.lib.gr_timing_query(self.handle, arr, 64))
        return {arr[i].name.decode(): (int(arr[i].count), float(arr[i].total_ms)) for i in range(n)}

    # ---- post chain -------------------------------------------------------------------------------------------
    @staticmethod
    def _rows(rows):
        return None if rows is None else C.byref(Rows(int(rows[0]), int(rows[1])))

    def bloom_threshold(self, hdr: DeviceImage, out: DeviceImage, lum_ptr=None, stream=None, rows=None):
        self.check(self.lib.gr_bloom_threshold_rows(self.handle, stream, hdr.desc, out.desc, lum_ptr, threshold_push(out), self._rows(rows)))

    def bloom_downsample(self, src: DeviceImage, out: DeviceImage, history: Optional[DeviceImage] = None, lerp: float = 0.0,
                         stream=None, rows=None):
        self.check(self.lib.gr_bloom_downsample_rows(self.handle, stream, src.desc, out.desc,
                                                     history.desc if history is not None else None, downsample_push(out, src, lerp), self._rows(rows)))

    def bloom_upsample(self, src: DeviceImage, out: DeviceImage, stream=None, rows=None):
        self.check(self.lib.gr_bloom_upsample_rows(self.handle, stream, src.desc, out.desc, upsample_push(out, src), self._rows(rows)))

    def bloom_tail(self, d1: DeviceImage, d2: DeviceImage, d3: DeviceImage, history: DeviceImage, u2: DeviceImage, u1: DeviceImage,
                   feedback_lerp: float, lum_ptr=None, lum_lerp: float = 0.0, stream=None) -> bool:
        """downsample-2, downsample-3 (+ feedback), luminance, upsample-2, upsample-1 as the two fused launches; False (nothing
        launched) when the pyramid does not qualify."""
        p_d2, p_d3 = downsample_push(d2, d1, feedback_lerp), downsample_push(d3, d2, feedback_lerp)
        p_u2, p_u1 = upsample_push(u2, d3), upsample_push(u1, u2)
        if not self.lib.gr_bloom_tail_supported(d1.desc, d2.desc, d3.desc, u2.desc, u1.desc, p_d2, p_d3, p_u2, p_u1):
            return False
        self.check(self.lib.gr_bloom_down_tail(self.handle, stream, d1.desc, d2.desc, d3.desc, history.desc, p_d2, p_d3))
        p_lum = luminance_push(d3, lum_lerp) if lum_ptr is not None else None
        self.check(self.lib.gr_bloom_up_tail(self.handle, stream, d3.desc, u2.desc, u1.desc, lum_ptr, p_u2, p_u1, p_lum))
        return True

    def bloom_down_mid(self, threshold: DeviceImage, d0: DeviceImage, d1: DeviceImage, stream=None, rows=None) -> bool:
        """downsample-0 and downsample-1 as one launch (rows restricts downsample-1); False (nothing launched) when the levels do not qualify."""
        p_d0, p_d1 = downsample_push(d0, threshold), downsample_push(d1, d0)
        if not self.lib.gr_bloom_down_mid_supported(threshold.desc, d0.desc, d1.desc, p_d0, p_d1):
            return False
        self.check(self.lib.gr_bloom_down_mid(self.handle, stream, threshold.desc, d0.desc, d1.desc, p_d0, p_d1, self._rows(rows)))
        return True

    def bloom_up_all(self, d3: DeviceImage, u2: DeviceImage, u1: DeviceImage, u0: DeviceImage, lum_ptr=None, lum_lerp: float = 0.0, stream=None,
                     busy_frame: bool = False) -> bool:
        """luminance, upsample-2, upsample-1 and upsample-0 as one launch; False (nothing launched) when the frame does not qualify."""
        p_u2, p_u1, p_u0 = upsample_push(u2, d3), upsample_push(u1, u2), upsample_push(u0, u1)
        if not self.lib.gr_bloom_up_all_supported(d3.desc, u2.desc, u1.desc, u0.desc, p_u2, p_u1, p_u0):
            return False
        p_lum = luminance_push(d3, lum_lerp) if lum_ptr is not None else None
        self.check(self.lib.gr_bloom_up_all(self.handle, stream, d3.desc, u2.desc, u1.desc, u0.desc, lum_ptr, p_u2, p_u1, p_u0, p_lum, 1 if busy_frame else 0))
        return True

    def bloom_pyramid(self, hdr: DeviceImage, levels: dict, history: DeviceImage, feedback_lerp: float, lum_ptr=None, lum_lerp: float = 0.0, stream=None,
                      any_size: bool = False) -> bool:
        """The whole bloom pass as ONE launch (levels: threshold, d0..d3, u2..u0 by name); False (nothing launched) when the frame does not qualify.
        any_size: launch without asking gr_bloom_pyramid_supported (which offers the launch up to 640 x 384 frames; the launcher checks the rest itself)."""
        a = pyramid_args(hdr.desc, {name: image.desc for name, image in levels.items()}, history.desc, feedback_lerp, lum_ptr, lum_lerp)
        if not any_size and not self.lib.gr_bloom_pyramid_supported(a):
            return False
        self.check(self.lib.gr_bloom_pyramid(self.handle, stream, a))
        return True

    def pyramid_giveups(self) -> int:
        n = C.c_uint32(0)
        self.check(self.lib.gr_debug_pyramid_giveups(self.handle, C.byref(n)))
        return int(n.value)

    def bloom_down_head(self, hdr: DeviceImage, threshold: DeviceImage, d0: DeviceImage, d1: DeviceImage, lum_ptr=None, stream=None) -> bool:
        """threshold, downsample-0 and downsample-1 as one launch; False (nothing launched) when the frame does not qualify."""
        p_t, p_d0, p_d1 = threshold_push(threshold), downsample_push(d0, threshold), downsample_push(d1, d0)
        if not self.lib.gr_bloom_down_head_supported(hdr.desc, threshold.desc, d0.desc, d1.desc, p_t, p_d0, p_d1):
            return False
        self.check(self.lib.gr_bloom_down_head(self.handle, stream, hdr.desc, threshold.desc, d0.desc, d1.desc, lum_ptr, p_t, p_d0, p_d1))
        return True

    def luminance(self, d3: DeviceImage, lum_ptr, lerp: float, min_loglum: float = -3.0, max_loglum: float = 2.0, stream=None):
        self.check(self.lib.gr_luminance(self.handle, stream, d3.desc, lum_ptr, luminance_push(d3, lerp, min_loglum, max_loglum)))

    def tonemap(self, hdr: DeviceImage, bloom: DeviceImage, out: DeviceImage, lum_ptr=None, dynamic_exposure: float = 1.0,
                stream=None, rows=None):
        push = PushTonemap(dynamic_exposure)
        self.check(self.lib.gr_tonemap_rows(self.handle, stream, hdr.desc, bloom.desc, out.desc, lum_ptr, push, self._rows(rows)))


    # ---- anti-aliasing --------------------------------------------------------------------------------------------
    def fxaa(self, src: DeviceImage, out: DeviceImage, stream=None):
        push = PushFxaa((1.0 / src.width, 1.0 / src.height))
        self.check(self.lib.gr_fxaa(self.handle, stream, src.desc, out.desc, push))

    def smaa_set_luts(self, area: np.ndarray, search: np.ndarray):
        a, s = np.ascontiguousarray(area, np.uint8), np.ascontiguousarray(search, np.uint8)
        assert a.size == 160 * 560 * 2 and s.size == 64 * 16
        self.check(self.lib.gr_smaa_set_luts(self.handle, a.ctypes.data, s.ctypes.data))

    @staticmethod
    def _smaa_push(img: DeviceImage) -> PushSmaa:
        return PushSmaa((1.0 / img.width, 1.0 / img.height, float(img.width), float(img.height)))

    def smaa_edge_detection(self, color: DeviceImage, edges: DeviceImage, quality: int, stream=None):
        self.check(self.lib.gr_smaa_edge_detection(self.handle, stream, color.desc, edges.desc, self._smaa_push(color), quality))

    def smaa_blend_weight(self, edges: DeviceImage, weights: DeviceImage, quality: int, stream=None):
        self.check(self.lib.gr_smaa_blend_weight(self.handle, stream, edges.desc, weights.desc, self._smaa_push(edges), quality))

    def smaa_neighbor_blend(self, color: DeviceImage, weights: DeviceImage, out: DeviceImage, stream=None):
        self.check(self.lib.gr_smaa_neighbor_blend(self.handle, stream, color.desc, weights.desc, out.desc, self._smaa_push(color)))

    def taa_resolve(self, current: DeviceImage, depth: DeviceImage, mv: DeviceImage, history, out_color: DeviceImage,
                    out_history: DeviceImage, reproj16, quality: int, stream=None):
        push = PushTaa()
        push.reproj[:] = [float(v) for v in reproj16]
        push.rt_metrics[:] = (1.0 / current.width, 1.0 / current.height, float(current.width), float(current.height))
        self.check(self.lib.gr_taa_resolve(self.handle, stream, current.desc, depth.desc, mv.desc,
                                           history.desc if history is not None else None, out_color.desc, out_history.desc, push,
                                           quality))

    def texture_decode(self, block_format: int, blocks, block_row_pitch: int, out, stream=None):
        """gr_texture_decode: one level of one layer of BC1-BC7 or ASTC LDR blocks (device pointer; ceil(w / bw) blocks a row, bw x bh
        texels a block as texture_block_info gives them) into `out` (DeviceImage or Image) of the decoded format."""
        desc = out.desc if isinstance(out, DeviceImage) else out
        self.check(self.lib.gr_texture_decode(self.handle, stream, int(block_format), blocks, int(block_row_pitch), C.byref(desc)))

    def texture_encode(self, block_format: int, image, blocks, block_row_pitch: int, stream=None):
        """gr_texture_encode: one level of one layer of R8 / RG8 / RGBA8 texels (`image`: DeviceImage or Image) to BC4 / BC5 blocks at the
        device pointer `blocks`, ceil(w / 4) blocks a row, rows `block_row_pitch` bytes apart."""
        desc = image.desc if isinstance(image, DeviceImage) else image
        self.check(self.lib.gr_texture_encode(self.handle, stream, int(block_format), C.byref(desc), blocks, int(block_row_pitch)))

    def texture_generate_mipmap(self, src, dst, stream=None):
        """gr_texture_generate_mipmap: `dst` (max(src >> 1, 1) texels an axis, same UNORM8 format) from `src`; DeviceImage or Image each."""
        s, d = (i.desc if isinstance(i, DeviceImage) else i for i in (src, dst))
        self.check(self.lib.gr_texture_generate_mipmap(self.handle, stream, C.byref(s), C.byref(d)))

    @staticmethod
    def texture_block_info(block_format: int):
        """(block width, block height, bytes per block, decoded format) of a format gr_texture_decode takes; ValueError otherwise."""
        lib = load_library()
        w, h, nbytes, decoded = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        if lib.gr_texture_block_dim(int(block_format), C.byref(w), C.byref(h)) < 0 or \
                lib.gr_texture_block_info(int(block_format), C.byref(nbytes), C.byref(decoded)) < 0:
            raise ValueError(f"format {block_format} is not a block format gr_texture_decode takes")
        return w.value, h.value, nbytes.value, decoded.value

    # ---- environment baking: cubes are DeviceBuffers holding an RGBA16F chain in GTX payload layout (gr_cube_chain_bytes) ----------
    def env_equirect_to_cube(self, equirect: DeviceImage, cube: DeviceBuffer, size: int, levels: int, stream=None):
        """gr_env_equirect_to_cube: lat-long RGBA16F image -> cube level 0, then `levels - 1` linear-blit mips."""
        assert cube.nbytes >= self.lib.gr_cube_chain_bytes(size, levels) or not (0 < size <= 16384), (cube.nbytes, size, levels)
        self.check(self.lib.gr_env_equirect_to_cube(self.handle, stream, equirect.desc, cube.ptr, int(size), int(levels)))

    def env_specular(self, src: DeviceBuffer, src_size: int, src_levels: int, out: DeviceBuffer, out_size: int, out_levels: int, stream=None):
        """gr_env_specular: the GGX-prefiltered reflection chain of a cube, all faces and levels in one launch."""
        assert src.nbytes >= self.lib.gr_cube_chain_bytes(src_size, src_levels) and out.nbytes >= self.lib.gr_cube_chain_bytes(out_size, out_levels)
        self.check(self.lib.gr_env_specular(self.handle, stream, C.byref(Cube(src.ptr, src_size, src_levels)), out.ptr, int(out_size), int(out_levels)))

    def env_diffuse(self, src: DeviceBuffer, src_size: int, src_levels: int, out: DeviceBuffer, out_size: int, stream=None):
        """gr_env_diffuse: the irradiance cube (one level) of a cube."""
        assert src.nbytes >= self.lib.gr_cube_chain_bytes(src_size, src_levels) and out.nbytes >= self.lib.gr_cube_chain_bytes(out_size, 1)
        self.check(self.lib.gr_env_diffuse(self.handle, stream, C.byref(Cube(src.ptr, src_size, src_levels)), out.ptr, int(out_size)))

    # ---- the sky pass ------------------------------------------------------------------------------------------------------------------
    def sky_apply(self, emissive: DeviceImage, depth: DeviceImage, inv_local_view_projection, color, camera_height: float, sun_direction,
                  cube: Optional[DeviceBuffer] = None, cube_size: int = 0, cube_levels: int = 0, stream=None):
        """gr_sky_apply: the far pixels (depth == 0) of `emissive` get the atmosphere, or, with a cube, texture(cube, direction).rgb * color."""
        args = SkyArgs()
        args.emissive, args.depth = emissive.desc, depth.desc
        args.inv_local_view_projection[:] = [float(v) for v in np.asarray(inv_local_view_projection, np.float32).reshape(16)]
        args.color[:] = [float(v) for v in color]
        args.camera_height = float(camera_height)
        args.sun_direction[:] = [float(v) for v in sun_direction]
        if cube is not None:
            assert cube.nbytes >= self.lib.gr_cube_chain_bytes(cube_size, cube_levels) or not (0 < cube_size <= 16384), (cube.nbytes, cube_size, cube_levels)
            args.cube = Cube(cube.ptr, int(cube_size), int(cube_levels))
        self.check(self.lib.gr_sky_apply(self.handle, stream, C.byref(args)))

    def sky_cube(self, out: DeviceBuffer, size: int, sun_color, camera_y: float, sun_direction, stream=None):
        """gr_sky_cube: six faces of `size` RGBA16F texels of atmosphere (32 / 16 steps, alpha 1), level 0 of a gr_env_* chain."""
        assert out.nbytes >= self.lib.gr_cube_chain_bytes(size, 1) or not (0 < size <= 16384), (out.nbytes, size)
        params = SkyCubeParams((C.c_float * 3)(*[float(v) for v in sun_color]), float(camera_y), (C.c_float * 3)(*[float(v) for v in sun_direction]), 0.0)
        self.check(self.lib.gr_sky_cube(self.handle, stream, out.ptr, int(size), C.byref(params)))

    # ---- directional-light shadows ---------------------------------------------------------------------------------------------------
    def directional_light(self, args: DirectionalLightArgs, stream=None):
        """gr_directional_light: hdr = rne16(emissive + the shadowed directional light [+ the ambient fallback]) where depth != 0."""
        self.check(self.lib.gr_directional_light(self.handle, stream, C.byref(args)))

    def vsm_moments(self, depth, moments, stream=None):
        """gr_vsm_moments: (z, z * z) of a D16_UNORM or D32_SFLOAT map into an R32G32_SFLOAT image of its size."""
        self.check(self.lib.gr_vsm_moments(self.handle, stream, depth.desc, moments.desc))

    def vsm_blur(self, src, out, up: bool, stream=None):
        """gr_vsm_blur: the nine-tap down (taps at +-1.75 texels of src) or up (+-0.875) blur of one layer of moments."""
        self.check(self.lib.gr_vsm_blur(self.handle, stream, src.desc, out.desc, int(bool(up))))

    # ---- FFT: a plan owns its scratch and twiddles and may be in flight on one stream at a time ---------------------------------
    def fft_plan(self, options: FftOptions):
        """gr_fft_plan_create: an opaque plan handle (free it with fft_plan_destroy)."""
        plan = C.c_void_p()
        self.check(self.lib.gr_fft_plan_create(self.handle, C.byref(options), C.byref(plan)))
        return plan

    def fft_plan_destroy(self, plan):
        self.lib.gr_fft_plan_destroy(self.handle, plan)

    def fft_execute(self, plan, dst: FftResource, src: FftResource, stream=None, iteration: Optional[int] = None):
        """gr_fft_execute, or gr_fft_execute_iteration for one pass of the plan."""
        if iteration is None:
            self.check(self.lib.gr_fft_execute(self.handle, stream, plan, C.byref(dst), C.byref(src)))
        else:
            self.check(self.lib.gr_fft_execute_iteration(self.handle, stream, plan, C.byref(dst), C.byref(src), int(iteration)))

    # ---- ocean: the FFT update's own dispatches -----------------------------------------------------------------------------------
    def ocean_generate_fft(self, distribution, out, push: PushOceanGenerate, variant: int, freq_bands=None, stream=None):
        """gr_ocean_generate_fft: distribution (N.x * N.y float2) -> out (N.x * N.y packed half2); both device pointers.  freq_bands: eight
        amplitudes (FREQ_BAND_MODULATION) or None."""
        bands = None if freq_bands is None else (C.c_float * OCEAN_NUM_FREQ_BANDS)(*[float(v) for v in freq_bands])
        self.check(self.lib.gr_ocean_generate_fft(self.handle, stream, distribution, out, C.byref(push), int(variant), bands))

    def ocean_bake_maps(self, height: DeviceImage, displacement: DeviceImage, grad_jacobian: DeviceImage, height_displacement: Optional[DeviceImage],
                        push: PushOceanBake, stream=None):
        """gr_ocean_bake_maps: R16F height + RG16F displacement -> RGBA16F gradient / Jacobian and (unless None) height / displacement."""
        hd = None if height_displacement is None else height_displacement.desc
        self.check(self.lib.gr_ocean_bake_maps(self.handle, stream, height.desc, displacement.desc, grad_jacobian.desc, hd, C.byref(push)))

    def ocean_mipmap(self, src: DeviceImage, out: DeviceImage, push: PushOceanMipmap, stream=None):
        """gr_ocean_mipmap: one LinearWrap tap per texel of `out` (push.count texels) from `src`, times push.result_mod."""
        self.check(self.lib.gr_ocean_mipmap(self.handle, stream, src.desc, out.desc, C.byref(push)))

    # ---- ocean: the LOD update's dispatches ------------------------------------------------------------------------------------------
    def ocean_update_lod(self, lod_image: DeviceImage, push: PushOceanUpdateLod, stream=None):
        """gr_ocean_update_lod: the R16F LOD map of a num_threads x num_threads grid."""
        self.check(self.lib.gr_ocean_update_lod(self.handle, stream, lod_image.desc, C.byref(push)))

    def ocean_init_counter_buffer(self, counters: "DeviceBuffer", counts16, stream=None):
        """gr_ocean_init_counter_buffer: eight indirect draws, index_count from the first eight of the sixteen counts."""
        counts = (C.c_uint32 * 16)(*[int(v) for v in counts16])
        self.check(self.lib.gr_ocean_init_counter_buffer(self.handle, stream, C.byref(OceanBuffer(counters.ptr, counters.nbytes)), counts))

    def ocean_cull_blocks(self, lod_image: DeviceImage, wrap: int, patches: "DeviceBuffer", counters: "DeviceBuffer", push: PushOceanCull, frustum, stream=None):
        """gr_ocean_cull_blocks: one patch per block in view, appended to its LOD's bucket.  frustum: 24 floats, six planes."""
        planes = (C.c_float * 24)(*[float(v) for v in frustum])
        self.check(self.lib.gr_ocean_cull_blocks(self.handle, stream, lod_image.desc, int(wrap), C.byref(OceanBuffer(patches.ptr, patches.nbytes)),
                                                 C.byref(OceanBuffer(counters.ptr, counters.nbytes)), C.byref(push), planes))

    # ---- mesh decode --------------------------------------------------------------------------------------------------------------------
    def meshlet_decode(self, args: MeshletDecodeArgs, primitive_offset: int, vertex_offset: int, meshlet_count: int, wg_offset: int = 0, stream=None):
        """gr_meshlet_decode: one launch that expands MESHLET4 streams into index, position, attribute and skin buffers."""
        push = PushMeshletDecode(int(primitive_offset), int(vertex_offset), int(meshlet_count), int(wg_offset))
        self.check(self.lib.gr_meshlet_decode(self.handle, stream, C.byref(args), C.byref(push)))

    def meshlet_cull(self, args: MeshletCullArgs, offset: int, count: int, mdi_count_offset: int, draw_indirect_offset: int, stream=None):
        """gr_meshlet_cull: one launch that culls `count` tasks from `offset` on and appends the surviving chunks' draw records."""
        push = PushMeshletCull(int(offset), int(count), int(mdi_count_offset), int(draw_indirect_offset))
        self.check(self.lib.gr_meshlet_cull(self.handle, stream, C.byref(args), C.byref(push)))

    # ---- SSAO: FidelityFX CACAO --------------------------------------------------------------------------------------------------------
    def cacao_workspace(self, width: int, height: int) -> DeviceBuffer:
        """A workspace for a width x height frame (gr_alloc returns 256-byte aligned memory)."""
        nbytes = self.lib.gr_cacao_workspace_bytes(width, height)
        if nbytes == 0:
            raise GraniteHipError(f"gr_cacao_workspace_bytes: {width} x {height} is not a size the SSAO pass takes")
        return DeviceBuffer(self, nbytes)

    def cacao(self, depth: DeviceImage, normal: DeviceImage, out: DeviceImage, workspace, constants, quality: int = CACAO_QUALITY_HIGHEST,
              blur_passes: int = 2, stream=None):
        """The sequence of FFX_CACAO_GraniteDraw on one stream: depth D32_SFLOAT and normal A2B10G10R10 -> out R8_UNORM.  workspace: a
        DeviceBuffer or a 256-byte aligned device pointer of gr_cacao_workspace_bytes; constants: cacao_constants(...)."""
        lib, h = self.lib, self.handle
        ws = workspace.ptr if isinstance(workspace, DeviceBuffer) else workspace
        w, hgt = depth.width, depth.height
        self.check(lib.gr_cacao_prepare_depths(h, stream, depth.desc, ws, constants))
        self.check(lib.gr_cacao_prepare_normals(h, stream, normal.desc, ws, constants))
        if quality == CACAO_QUALITY_HIGHEST:
            self.check(lib.gr_cacao_generate_base(h, stream, ws, w, hgt, constants))
            self.check(lib.gr_cacao_importance_generate(h, stream, ws, w, hgt, constants))
            self.check(lib.gr_cacao_importance_postprocess_a(h, stream, ws, w, hgt, constants))
            self.check(lib.gr_cacao_importance_postprocess_b(h, stream, ws, w, hgt, constants))
        self.check(lib.gr_cacao_generate(h, stream, ws, w, hgt, constants, quality))
        if blur_passes:
            self.check(lib.gr_cacao_blur(h, stream, ws, w, hgt, constants, blur_passes))
        self.check(lib.gr_cacao_apply(h, stream, ws, out.desc, constants, 1 if blur_passes else 0))

    def blit(self, src: DeviceImage, out: DeviceImage, linear: bool, stream=None):
        self.check(self.lib.gr_blit(self.handle, stream, src.desc, out.desc, int(linear)))

    def fsr_upscale(self, src: DeviceImage, out: DeviceImage, fp16: bool = True, stream=None):
        self.check(self.lib.gr_fsr_upscale(self.handle, stream, src.desc, out.desc, int(fp16)))

    def fsr_sharpen(self, src: DeviceImage, out: DeviceImage, sharpness: float, stream=None):
        self.check(self.lib.gr_fsr_sharpen(self.handle, stream, src.desc, out.desc, C.c_float(sharpness)))

    def pq10_encode(self, hdr: DeviceImage, ui: DeviceImage, out: DeviceImage, conversion9, hdr_pre_exposure=500.0, ui_pre_exposure=400.0,
                    max_light_level=1000.0, stream=None):
        push = PushPq10()
        m = [float(v) for v in conversion9]
        for col in range(3):
            for row in range(3):
                push.primary_conversion[4 * col + row] = m[3 * col + row]
        push.primary_conversion[15] = 1.0
        push.hdr_pre_exposure, push.ui_pre_exposure = hdr_pre_exposure, ui_pre_exposure
        push.max_light_level, push.inv_max_light_level = max_light_level, float(np.float32(1.0) / np.float32(max_light_level))
        self.check(self.lib.gr_pq10_encode(self.handle, stream, hdr.desc, ui.desc, out.desc, push))

    def video_scale(self, src: DeviceImage, planes, input_color_space: int = COLOR_SPACE_SRGB_NONLINEAR,
                    output_color_space: int = COLOR_SPACE_SRGB_NONLINEAR, stream=None):
        """gr_video_scale: `src` converted (and rescaled to planes[0]'s size) into 1-3 output planes (DeviceImage or Image)."""
        arr = (Image * len(planes))(*[p.desc if isinstance(p, DeviceImage) else p for p in planes])
        self.check(self.lib.gr_video_scale(self.handle, stream, src.desc, arr, len(planes), int(input_color_space), int(output_color_space)))

    def video_yuv_to_rgb(self, planes, out, info: VideoYuvInfo, stream=None):
        """gr_video_yuv_to_rgb: 1-3 YCbCr planes (DeviceImage or Image) converted into `out`."""
        arr = (Image * len(planes))(*[p.desc if isinstance(p, DeviceImage) else p for p in planes])
        dst = out.desc if isinstance(out, DeviceImage) else out
        self.check(self.lib.gr_video_yuv_to_rgb(self.handle, stream, arr, len(planes), C.byref(dst), C.byref(info)))

    def hiz(self, depth: DeviceImage, z_transform, output_downsample: bool = False, chain: Optional[DeviceBuffer] = None,
            counter: Optional[DeviceBuffer] = None, stream=None):
        """Depth hierarchy of `depth` sized as setup_depth_hierarchy_pass sizes it (spd.cpp:207-218).  Returns
        (chain buffer, counter buffer, layout dict); chain / counter can be passed back in to reuse them."""
        ds = int(output_downsample)
        levels = max(1, max(depth.width, depth.height).bit_length() - 1 - ds)
        cw, ch = ((depth.width + 63) & ~63) >> ds, ((depth.height + 63) & ~63) >> ds
        if chain is None:
            chain = DeviceBuffer(self, self.lib.gr_mip_chain_size(cw, ch, 4, levels))
        if counter is None:
            counter = DeviceBuffer(self, 4)
        args = HizArgs()
        args.depth = depth.desc
        args.chain, args.chain_width, args.chain_height, args.chain_levels = chain.ptr, cw, ch, levels
        args.output_downsample = ds
        args.z_transform[:] = [float(v) for v in z_transform]
        args.counter = counter.ptr
        self.check(self.lib.gr_hiz(self.handle, stream, args))
        return chain, counter, {"chain_w": cw, "chain_h": ch, "levels": levels}

    def ssr_trace(self, chain: DeviceBuffer, layout: dict, pbr: DeviceImage, normal: DeviceImage, light: DeviceImage, dither: DeviceBuffer,
                  frame: int, view_projection, inv_view_projection, camera_position, stream=None, images: Optional[dict] = None) -> dict:
        """classify + build_indirect + trace_primary.  Returns the output / ray-length / confidence images and the ray buffers.
        images: the caller's own "output" (RGBA16F), "ray_length" (R16F) and "confidence" (R8) images, any of them; else fresh tight ones."""
        w, h = light.width, light.height
        images = images or {}
        out = {"output": images.get("output") or DeviceImage(self, w, h, FORMAT_R16G16B16A16_SFLOAT),
               "ray_length": images.get("ray_length") or DeviceImage(self, w, h, FORMAT_R16_SFLOAT),
               "confidence": images.get("confidence") or DeviceImage(self, w, h, FORMAT_R8_UNORM), "ray_list": DeviceBuffer(self, w * h * 4),
               "ray_counter": DeviceBuffer(self, 4096), "scratch": DeviceBuffer(self, self.lib.gr_ssr_scratch_bytes(w, h))}
        a = SsrArgs()
        a.depth_chain, a.chain_width, a.chain_height, a.chain_levels = chain.ptr, layout["chain_w"], layout["chain_h"], layout["levels"]
        a.pbr, a.normal, a.light = pbr.desc, normal.desc, light.desc
        a.dither_lut, a.frame = dither.ptr, frame
        a.view_projection[:] = [float(v) for v in view_projection]
        a.inv_view_projection[:] = [float(v) for v in inv_view_projection]
        a.camera_position[:] = [float(v) for v in camera_position]
        a.output, a.ray_length, a.ray_confidence = out["output"].desc, out["ray_length"].desc, out["confidence"].desc
        a.ray_list, a.ray_counter, a.scratch = out["ray_list"].ptr, out["ray_counter"].ptr, out["scratch"].ptr
        self.check(self.lib.gr_ssr_trace(self.handle, stream, a))
        return out

    def ssr_apply(self, hdr: DeviceImage, reflected: DeviceImage, albedo: DeviceImage, normal: DeviceImage, pbr: DeviceImage, depth: DeviceImage,
                  brdf_lut: DeviceImage, inv_view_projection, camera_position, stream=None):
        a = SsrApplyArgs()
        a.hdr, a.reflected, a.albedo, a.normal, a.pbr, a.depth, a.brdf_lut = (i.desc for i in (hdr, reflected, albedo, normal, pbr, depth, brdf_lut))
        a.inv_view_projection[:] = [float(v) for v in inv_view_projection]
        a.camera_position[:] = [float(v) for v in camera_position]
        self.check(self.lib.gr_ssr_apply(self.handle, stream, a))

    def spd_downsample(self, source: DeviceImage, width: int, height: int, mips: int, components: int = 4, depth_mode: bool = False,
                       filter_mods=None, chain: Optional[DeviceBuffer] = None, stream=None) -> DeviceBuffer:
        """emit_single_pass_downsample: fills an RGBA16F chain whose level 0 is width x height from `source`."""
        if chain is None:
            chain = DeviceBuffer(self, self.lib.gr_mip_chain_size(width, height, 8, mips))
        args = SpdArgs()
        args.input = source.desc
        args.chain, args.width, args.height, args.mips, args.components = chain.ptr, width, height, mips, components
        args.reduction_mode = SPD_REDUCTION_DEPTH if depth_mode else SPD_REDUCTION_COLOR
        fm = None if filter_mods is None else np.ascontiguousarray(filter_mods, np.float32).reshape(mips, 4)
        args.filter_mods = None if fm is None else fm.ctypes.data
        self.check(self.lib.gr_spd_downsample(self.handle, stream, args))
        return chain

    def read_mip_chain(self, chain: DeviceBuffer, layout: dict):
        raw = chain.download(np.float32)
        out = []
        for l in range(layout["levels"]):
            w, h = max(layout["chain_w"] >> l, 1), max(layout["chain_h"] >> l, 1)
            o = self.lib.gr_mip_chain_offset(layout["chain_w"], layout["chain_h"], 4, l) // 4
            out.append(raw[o:o + w * h].reshape(h, w))
        return out
