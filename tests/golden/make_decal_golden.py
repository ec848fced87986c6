"""Records tests/golden/decal_shader_v1.npz: the reference's lights/clusterer_bindless_binning_decal.comp and apply_volumetric_decals of
lights/volumetric_decal.h, executed on the CPU, on the cases of tests/decal_cases.py.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  Same recipe as make_meshlet_cull_golden.py: the
shaders are re-spelled with oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory, compiled against
oracle/ref_build/glsl_cpu.hpp with the runner next to this file (-ffp-contract=off), run, and the directory is removed: only inputs and
outputs are kept.  The archive is written with fixed time stamps, so that a second run gives the same bytes.

    python tests/golden/make_decal_golden.py [output.npz]

The binning shader runs in both of its forms, SUBGROUPS=0 (one 32-thread workgroup per cell and chunk) and SUBGROUPS=1 with 64 lanes
(8 x 8 cell tile); ballot and shuffle are the runner's.  The two forms must agree on every case; the 64-lane result is stored.  (They do not
agree everywhere: for a decal wholly right of or below the screen, at a resolution whose reciprocal is not exact, the last cell's
u + stride rounds above 1.0 where its tile's does not.  The cases keep their decals' centres on screen.)

volumetric_decal.h cannot be compiled as the reference ships it, and the temporary copy is touched in three places, none of which holds
arithmetic:
  - lights/linear_geometry_sampler.h names the binding BINDING_GLOBAL_GEOMETRY_SAMPLER, which inc/global_bindings.h no longer defines
    (it has ..._SAMPLER_WRAP and ..._SAMPLER_CLAMP); glsl2cpp.py drops layout() qualifiers, and the dead name with them;
  - `world_to_texture[0 .. 2]` indexes a mat_affine, which inc/affine.h has since made a struct of `vec4 rows[3]`: spelled
    `world_to_texture.rows[0 .. 2]`;
  - `texture2D TexDecals[];`, an unsized descriptor array, is spelled as a pointer, as glsl2cpp.py spells unsized buffer members.
The apply runs at subgroup size 1, one invocation per pixel with depth != 0.  texture() is the runner's, with the model stated in
granite_amd/csrc/decal_core.hpp, fed the uv of the aligned 2 x 2 quad.  The stored result is the float colour before the 8-bit store and
whether a decal was fetched for the pixel.

The decal z ranges are the reference's clusterer_bindless_z_range.comp as oracle/ref_build runs it (oracle/_ref/libref_shaders.so, built by
__graft_entry__.build()) over the cases' slice intervals.

The host functions are pinned by the reference's own math library: decal_host_runner.cpp, compiled at generation time against the reference's
math/simd.hpp, math/aabb.hpp and math/muglm (with muglm.cpp and aabb.cpp from where they lie, -msse4.1 as oracle/ref_build builds
libref_muglm.so), evaluates per decal of every apply case the sort key dot(front, transform_aabb(unit box).get_center()), decal_z_range's
lo / hi through SIMD::mul(vec4, mat_affine, vec4), the mvp through SIMD::mul(mat4, mat4, mat4) and mat_affine(inverse(world.to_mat4())).
All four are stored (`<case>/host/...`) and decal_ref.py -- which the host layer is held to bit for bit by tests/test_decal_app_cpu.py -- must equal
them bit for bit.  (host/math.cpp's general inverse() works in double; the decal path restates muglm's fp32 one.)

Asserts that tests/decal_ref.py equals all of this exactly -- masks and ranges word for word, the colour bit for bit -- and that every
branch the cases are there for is taken at least once."""
import ctypes as C
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle", "ref_build")]
import decal_cases as dc  # noqa: E402
import decal_ref as ref  # noqa: E402
import shader_runner as sr  # noqa: E402

LIGHTS = os.path.join(sr.SHADERS, "lights")


def patch_decal_header(text):
    assert "BINDING_GLOBAL_GEOMETRY_SAMPLER)" not in text
    for old, new, count in ((".world_to_texture[", ".world_to_texture.rows[", 3), ("texture2D TexDecals[];", "texture2D *TexDecals;", 1)):
        assert text.count(old) == count, old
        text = text.replace(old, new)
    return text


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), ["lights/clusterer_bindless_binning_decal.comp", "lights/volumetric_decal.h"],
               patch={"lights/volumetric_decal.h": patch_decal_header})
    objs = sr.compile_runner(tmp, os.path.join(HERE, "decal_runner.cpp"), [("decal_runner", [])], extra=["-pthread", "-fno-strict-aliasing"])
    return sr.link(os.path.join(tmp, "libdecal_runner.so"), objs, extra=["-pthread"])


def build_host(tmp):
    objs = sr.reference_math_objects(tmp, [("decal_host_runner", os.path.join(HERE, "decal_host_runner.cpp"), []), ("muglm", sr.MUGLM, []),
                                           ("aabb", os.path.join(sr.MATH, "aabb.cpp"), [])], extra=["-I" + os.path.join(sr.MATH, "muglm")])
    return sr.link(os.path.join(tmp, "libdecal_host_runner.so"), objs)


def run_host(host, case, cam):
    """the reference's math library on every decal of a case -> sort keys (n), world_to_texture (n, 12), z lo / hi (n, 2), mvps (n, 16)"""
    rp = cam.render_params()
    vp, pos, front = (np.ascontiguousarray(rp[a:b], np.float32) for a, b in ((32, 48), (96, 99), (99, 102)))
    n = len(case["world_rows"])
    keys, w2t, z, mvps = np.zeros(n, np.float32), np.zeros((n, 12), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 16), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for i in range(n):
        rows = np.ascontiguousarray(case["world_rows"][i], np.float32)
        host.ref_decal_host(p(rows), p(vp), p(pos), p(front), p(keys[i:i + 1]), p(w2t[i]), p(z[i]), p(mvps[i]))
    return keys, w2t, z, mvps


class DecalTex(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("num_levels", C.c_uint32), ("format", C.c_uint32)]


class ApplyRun(C.Structure):
    _fields_ = [("prm", C.c_void_p), ("inv_view_projection", C.c_void_p), ("decal_rows", C.c_void_p), ("bitmask", C.c_void_p), ("range", C.c_void_p),
                ("albedo", C.c_void_p), ("depth", C.c_void_p), ("textures", C.c_void_p), ("srgb_decode", C.c_void_p), ("colour", C.c_void_p), ("touched", C.c_void_p),
                ("width", C.c_uint32), ("height", C.c_uint32), ("num_textures", C.c_uint32)]


def run_binning(lib, case, subgroup_size):
    prm = np.frombuffer(case["prm"].tobytes(), np.uint8).copy()
    rx, ry = (int(v) for v in case["prm"]["resolution_xy"])
    mvps = np.ascontiguousarray(case["mvps"], np.float32).reshape(-1)
    mvps = mvps if len(mvps) else np.zeros(16, np.float32)
    out = np.zeros(rx * ry * int(case["prm"]["num_decals_32"]), np.uint32)
    lib.ref_decal_binning(prm.ctypes.data_as(C.c_void_p), mvps.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), subgroup_size)
    return out


def run_z_range(shaders, intervals, num_ranges):
    v = np.ascontiguousarray(intervals, np.uint32)
    out = np.zeros((num_ranges, 2), np.uint32)
    shaders.ref_cluster_z_range(v.ctypes.data_as(C.c_void_p), len(v), num_ranges, out.ctypes.data_as(C.c_void_p))
    return out


def run_apply(lib, case, bitmask, ranges):
    w, h = case["width"], case["height"]
    keep = {"prm": np.frombuffer(case["prm"].tobytes(), np.uint8).copy(), "inv": np.ascontiguousarray(case["inv_view_projection"], np.float32),
            "rows": np.ascontiguousarray(case["decal_rows"], np.float32), "bitmask": np.ascontiguousarray(bitmask, np.uint32),
            "range": np.ascontiguousarray(ranges, np.uint32), "albedo": np.ascontiguousarray(case["albedo"], np.uint32),
            "depth": np.ascontiguousarray(case["depth"], np.float32), "table": ref.srgb_decode_table(),
            "texels": [np.ascontiguousarray(t["texels"], np.uint32) for t in case["textures"]]}
    textures = (DecalTex * max(len(case["textures"]), 1))()
    for i, t in enumerate(case["textures"]):
        textures[i] = DecalTex(keep["texels"][i].ctypes.data, t["width"], t["height"], t["num_levels"], t["format"])
    colour, touched = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.uint8)
    p = lambda a: a.ctypes.data
    run = ApplyRun(p(keep["prm"]), p(keep["inv"]), p(keep["rows"]), p(keep["bitmask"]), p(keep["range"]), p(keep["albedo"]), p(keep["depth"]),
                   C.addressof(textures), p(keep["table"]), p(colour), p(touched), w, h, len(case["textures"]))
    lib.ref_decal_apply(C.byref(run))
    return colour, touched.astype(bool)


def write_npz(path, record):
    """np.savez_compressed with fixed time stamps: the same record gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(record):
            raw = io.BytesIO()
            np.lib.format.write_array(raw, np.asanyarray(record[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, raw.getvalue())


# what a case is there for: each counter is non-zero in that case (decal_ref.apply's info)
APPLY_COVERAGE = {
    "two_overlap": ["second_blend", "lod_above_zero", "lod_clamped_top"],
    "three_overlap_odd": ["third_blend", "lod_above_zero"],
    "far_plane": ["far_plane_in_footprint", "axis_without_partner"],
    "depth_step": ["masked_by_range", "lod_above_zero"],
    "beyond_slices": ["beyond_last_slice", "masked_by_range"],
    "texture_offset_3": ["blends"],
    "texture_outside": ["texture_outside_table", "blends"],
    "many": ["third_blend", "axis_without_partner"],
}
LEFT_OUT_CAP = 0.005  # of a case's decal-covered pixels (tests/test_decal_ref_cpu.py asserts it again)


def generate(path):
    for shader in ("clusterer_bindless_binning_decal.comp", "volumetric_decal.h"):
        if not os.path.isfile(os.path.join(LIGHTS, shader)):
            raise FileNotFoundError(os.path.join(LIGHTS, shader))
    shaders = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_shaders.so"))
    record = {}
    with sr.scratch("decal_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        host = C.CDLL(build_host(tmp))
        seen = {"full_screen": 0, "behind": 0, "empty_cells": 0, "two_chunks": 0, "three_chunks": 0, "no_decals": 0, "border_cells_out": 0, "sub_cell": 0}
        texture_blends = {}
        for name in dc.BINNING_CASES:
            case = dc.binning_case(name)
            plain, lanes64 = run_binning(lib, case, 0), run_binning(lib, case, 64)
            assert np.array_equal(plain, lanes64), f"{name}: the shader's two forms differ on {(plain != lanes64).sum()} words"
            mine = ref.binning(case["prm"], case["mvps"])
            ranges = run_z_range(shaders, case["intervals"], dc.RES_Z)
            print(f"{name:22s} {len(lanes64):5d} words, decal_ref differs on {(mine != lanes64).sum()}; {dc.RES_Z} ranges, decal_ref differs on {(ref.z_ranges(case['intervals'], dc.RES_Z) != ranges).sum()}")
            assert np.array_equal(mine, lanes64) and np.array_equal(ref.z_ranges(case["intervals"], dc.RES_Z), ranges), name
            n, n32 = int(case["prm"]["num_decals"]), int(case["prm"]["num_decals_32"])
            bb = ref.screen_bbs(case["mvps"]) if n else np.zeros((0, 4), np.float32)
            seen["full_screen"] += int((bb == np.float32([-1, -1, 1, 1])).all(axis=1).sum())
            seen["behind"] += int((bb == np.float32(-10)).all(axis=1).sum())
            seen["empty_cells"] += int((lanes64 == 0).sum())
            seen["two_chunks"] += n32 == 2
            seen["three_chunks"] += n32 == 3
            seen["no_decals"] += n == 0
            if name == "cell_border/8x8":  # decal 0 spans [-0.5, 0.5]: cells 2 .. 5 of 8 each way and no other, although cells 1 and 6 touch its edge
                want = np.zeros((8, 8), bool)
                want[2:6, 2:6] = True
                assert np.array_equal((lanes64.reshape(8, 8) & 1) != 0, want), name
                seen["border_cells_out"] += 1
            if name.startswith("sub_cell/"):  # smaller than a cell: each decal reaches one cell, or the up to four that meet where it lies
                rx = int(case["prm"]["resolution_xy"][0])
                for decal in range(n):
                    cells = np.nonzero((lanes64 >> decal) & 1)[0]
                    assert 1 <= len(cells) <= 4 and np.ptp(cells % rx) <= 1 and np.ptp(cells // rx) <= 1, (name, decal, cells)
                    seen["sub_cell"] += 1
            record.update({f"{name}/{k}": v for k, v in dc.pack_case(case).items()})
            record[f"{name}/bitmask"], record[f"{name}/range"] = lanes64, ranges
        for k, v in seen.items():
            assert v > 0, f"no binning case hit {k}"
        print("binning coverage: " + ", ".join(f"{k} {v}" for k, v in seen.items()))
        for name in dc.APPLY_CASES:
            case = dc.apply_case(name)
            plain, lanes64 = run_binning(lib, case, 0), run_binning(lib, case, 64)
            ranges = run_z_range(shaders, case["intervals"], dc.RES_Z)
            assert np.array_equal(plain, lanes64) and np.array_equal(lanes64, case["bitmask_decal"]) and np.array_equal(ranges, case["range_decal"]), name
            colour, touched = run_apply(lib, case, lanes64, ranges)
            mine = ref.apply(case)
            differ = int((colour.view(np.uint32) != mine["colour"].view(np.uint32)).sum()) + int((touched != mine["touched"]).sum())
            covered = int(touched.sum())
            margin = 64.0 * mine["uvw_error"]
            left_out = int((mine["edge_distance"] < margin).sum())
            print(f"{name:18s} {case['width']}x{case['height']}, {int(case['prm']['num_decals'])} decals: {covered} pixels covered, decal_ref differs on {differ} values; "
                  f"margin {margin:.3g}, {left_out} pixels within it; " + ", ".join(f"{k} {v}" for k, v in mine["info"].items() if v))
            assert differ == 0, name
            assert covered > 0 and left_out <= LEFT_OUT_CAP * covered, (name, left_out, covered)
            untouched = ~touched
            assert np.array_equal(colour[untouched].view(np.uint32), ref.srgb_decode_table()[(case["albedo"][untouched][:, None] >> np.uint32([0, 8, 16])) & 255].view(np.uint32))
            for key, count in mine["info"]["texture_blends"].items():
                texture_blends[key] = texture_blends.get(key, 0) + count
            # the host functions, by the reference's own math library
            cam = dc.synth.Camera(case["width"], case["height"])
            rp = cam.render_params()
            keys, w2t_muglm, z, host_mvps = run_host(host, case, cam)
            rows = case["world_rows"]
            assert np.array_equal(ref.host_sort_keys(rows, rp[99:102]).view(np.uint32), keys.view(np.uint32)), f"{name}: sort keys"
            assert np.array_equal(np.float32([ref.decal_z_range(r, rp[96:99], rp[99:102]) for r in rows]).view(np.uint32), z.view(np.uint32)), f"{name}: decal_z_range"
            assert np.array_equal(np.stack([ref.host_mvp(rp[32:48], r) for r in rows]).view(np.uint32), host_mvps.view(np.uint32)), f"{name}: mvps"
            w2t = np.stack([ref.host_world_to_texture(r) for r in rows])
            assert np.array_equal(w2t.view(np.uint32), w2t_muglm.view(np.uint32)), f"{name}: world_to_texture"
            print(f"{name:18s} host: {len(rows)} sort keys, z ranges, mvps and world_to_texture rows equal the reference's math library")
            record[f"{name}/host/world_rows"], record[f"{name}/host/sort_keys"], record[f"{name}/host/z_range"] = rows, keys, z
            record[f"{name}/host/mvps"], record[f"{name}/host/world_to_texture"] = host_mvps, w2t_muglm
            for cause in APPLY_COVERAGE[name]:
                assert mine["info"][cause] > 0, f"{name}: nothing hit {cause}"
            record.update({f"{name}/{k}": v for k, v in dc.pack_case(case).items()})
            record[f"{name}/bitmask"], record[f"{name}/range"] = lanes64, ranges
            record[f"{name}/colour"], record[f"{name}/touched"] = colour, touched
        for t in dc.texture_set():  # 16x4 full chain and 8x8 one level in both formats, 1x1
            key = (t["width"], t["height"], t["num_levels"], t["format"])
            assert texture_blends.get(key, 0) > 0, f"no decal blends texture {key}"
        print("texture coverage: " + ", ".join(f"{k[0]}x{k[1]} levels {k[2]} format {k[3]}: {v} blends" for k, v in sorted(texture_blends.items())))
    write_npz(path, record)
    stored = np.load(path)
    for name in dc.APPLY_CASES:  # what a test will read is what was recorded
        case, back = dc.apply_case(name), dc.golden_case(stored, name)
        assert all(np.array_equal(case[k], back[k]) for k in ("mvps", "intervals", "decal_rows", "albedo", "depth", "inv_view_projection", "bitmask_decal", "range_decal")), name
        assert case["prm"].tobytes() == back["prm"].tobytes() and len(case["textures"]) == len(back["textures"])
        assert all(np.array_equal(a["texels"], b["texels"]) and all(a[f] == b[f] for f in dc.TEXTURE_FIELDS) for a, b in zip(case["textures"], back["textures"])), name
    print(f"{path}: {os.path.getsize(path)} bytes, {len(dc.BINNING_CASES)} binning cases, {len(dc.APPLY_CASES)} apply cases")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "decal_shader_v1.npz"))
