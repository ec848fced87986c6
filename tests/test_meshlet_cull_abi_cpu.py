"""CPU: the culling ABI.  The ctypes structures have the sizes and offsets of the reference's blocks (meshlet_cull.comp's Registers,
inc/meshlet_render_types.h, inc/meshlet_ubos.h in std140), include/granite_hip.h asserts the same and declares the entry point, the
library exports it and capi lists it, gr_meshlet_cull_args is the same in C and in ctypes, and tests/meshlet_cull_ref.py -- the
restatement GPU tests use beyond the stored cases -- equals the executed shader on every stored case in every set."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meshlet_cull_cases as mc
import meshlet_cull_ref as ref
from granite_amd import capi
from host_program import ROOT, c_layout

HEADER = open(os.path.join(ROOT, "include", "granite_hip.h")).read()


def test_structures_have_the_shader_blocks_layout():
    assert C.sizeof(capi.PushMeshletCull) == 16
    assert [getattr(capi.PushMeshletCull, f).offset for f in ("offset", "count", "mdi_count_offset", "draw_indirect_offset")] == [0, 4, 8, 12]
    assert C.sizeof(capi.MeshletTask) == 20
    assert [getattr(capi.MeshletTask, f).offset for f in ("aabb_instance", "occluder_state_offset", "node_instance", "mesh_index_count", "material_flags")] == [0, 4, 8, 12, 16]
    assert C.sizeof(capi.MeshletAABB) == 32 and capi.MeshletAABB.hi.offset == 16
    assert C.sizeof(capi.MeshletBound) == 32 and capi.MeshletBound.radius.offset == 12 and capi.MeshletBound.cone_axis_cutoff.offset == 16
    assert C.sizeof(capi.MatAffine) == 48
    assert C.sizeof(capi.MeshletDraw) == 12 and capi.MeshletDraw.vertex_offset.offset == 8
    assert C.sizeof(capi.MeshletFrustum) == 224
    offsets = {"viewport": 0, "planes": 16, "view": 112, "viewport_scale_bias": 176, "hiz_resolution": 192, "winding": 200, "hiz_min_lod": 204, "hiz_max_lod": 208}
    assert {f: getattr(capi.MeshletFrustum, f).offset for f in offsets} == offsets
    assert (capi.MESHLET_CULL_ORTHO, capi.MESHLET_CULL_SKINNED, capi.MESHLET_CULL_FORCE_VISIBLE) == (ref.ORTHO, ref.SKINNED, ref.FORCE_VISIBLE) == (1, 2, 4)


def test_the_header_asserts_the_same_and_cites_the_reference():
    for line in ("GR_ASSERT_SIZE(gr_push_meshlet_cull, 16);", "GR_ASSERT_SIZE(gr_meshlet_task, 20);", "GR_ASSERT_SIZE(gr_meshlet_aabb, 32);", "GR_ASSERT_SIZE(gr_meshlet_bound, 32);",
                 "GR_ASSERT_SIZE(gr_mat_affine, 48);", "GR_ASSERT_SIZE(gr_meshlet_draw, 12);", "GR_ASSERT_SIZE(gr_meshlet_frustum, 224);"):
        assert line in HEADER, line
    for field, offset in (("viewport", 0), ("planes", 16), ("view", 112), ("viewport_scale_bias", 176), ("hiz_resolution", 192), ("winding", 200), ("hiz_min_lod", 204),
                          ("hiz_max_lod", 208)):
        assert f"GR_ASSERT_OFFSET(gr_meshlet_frustum, {field}, {offset});" in HEADER
    for cite in ("meshlet_cull.comp:23-29", "inc/meshlet_render_types.h:15-22", "inc/meshlet_ubos.h:4-14", "vulkan/mesh/meshlet.hpp:79-84", "vulkan/mesh/meshlet.hpp:72-77"):
        assert cite in HEADER, cite
    assert re.search(r"int gr_meshlet_cull\(gr_ctx \*ctx, gr_stream stream, const gr_meshlet_cull_args \*args, const gr_push_meshlet_cull \*push\);", HEADER)
    for flag, value in (("ORTHO", 1), ("SKINNED", 2), ("FORCE_VISIBLE", 4)):
        assert re.search(rf"#define GR_MESHLET_CULL_{flag} {value}u", HEADER)


def test_the_library_exports_the_entry_point():
    assert "gr_meshlet_cull" in capi.EXPORTED_SYMBOLS
    lib = capi.load_library()
    assert lib.gr_meshlet_cull.argtypes is not None and lib.gr_meshlet_cull.restype is C.c_int
    assert hasattr(capi.Context, "meshlet_cull")


def test_the_argument_block_is_the_same_in_c_and_in_ctypes(tmp_path):
    fields = [name for name, _ in capi.MeshletCullArgs._fields_]
    assert c_layout(tmp_path, "gr_meshlet_cull_args", fields) == [C.sizeof(capi.MeshletCullArgs)] + [getattr(capi.MeshletCullArgs, f).offset for f in fields]


def test_the_host_records_are_the_kernels():
    """meshlet_cull.hpp states its records again (it is also built without the C header): same sizes, and the C header's names in the host layer"""
    core = open(os.path.join(ROOT, "granite_amd", "csrc", "meshlet_cull.hpp")).read()
    assert "sizeof(Task) == 20 && sizeof(AABB) == 32 && sizeof(Bound) == 32 && sizeof(Affine) == 48 && sizeof(Draw) == 12 && sizeof(Frustum) == 224" in core
    host = open(os.path.join(ROOT, "granite_amd", "csrc", "host", "mesh", "meshlet_cull.cpp")).read()
    assert "sizeof(gr_meshlet_bound) == sizeof(Meshlet::Bound) && sizeof(gr_meshlet_draw) == sizeof(Meshlet::RuntimeHeaderDecodedMDI)" in host


GOLDEN = mc.load_golden()


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_the_restatement_equals_the_executed_shader(name):
    for phase, flags in mc.sets():
        scene = mc.golden_scene(GOLDEN, name, bool(flags & ref.ORTHO))
        want_output, want_occluders = mc.golden_result(GOLDEN, name, phase, flags)
        output, occluders, _ = mc.run_reference(scene, phase, flags)
        assert np.array_equal(output, want_output) and np.array_equal(occluders, want_occluders), (name, phase, flags)


def test_the_stored_cases_are_the_case_builders():
    """the archive holds what tests/meshlet_cull_cases.py builds today: a changed builder needs a regenerated golden"""
    chains = mc.chains()
    for name in mc.CASE_NAMES:
        for ortho in (False, True):
            built, stored = mc.build_case(name, ortho, chains), mc.golden_scene(GOLDEN, name, ortho)
            for a in mc.SCENE_ARRAYS + ("chain",):
                assert np.array_equal(built[a], stored[a]), (name, ortho, a)


def test_the_case_list_covers_what_it_names():
    assert {f"tasks_{n}" for n in (1, 31, 32, 33, 63, 64, 65, 130)} | {"none_tasks_0", "offset_nonzero", "two_lists"} <= set(mc.CASE_NAMES)
    assert len(mc.sets()) == 16
    scene = mc.golden_scene(GOLDEN, "two_lists", False)
    assert len(mc.dispatches_lists(scene["dispatches"])) == 2 and len({int(d[3]) for d in scene["dispatches"]}) == 2
    assert int(mc.golden_scene(GOLDEN, "offset_nonzero", False)["dispatches"][0][0]) > 0
    chunks = {(int(t[3]) & 31) + 1 for t in mc.golden_scene(GOLDEN, "tasks_33", False)["tasks"]}
    assert {1, 31, 32} <= chunks
    assert os.path.getsize(mc.GOLDEN_PATH) < 512 * 1024
