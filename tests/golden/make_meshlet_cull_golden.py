"""Records tests/golden/meshlet_cull_shader_v1.npz: the reference's meshlet_cull.comp (with inc/meshlet_render.h), executed on the CPU, on
the scenes of tests/meshlet_cull_cases.py.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  Same recipe as make_meshlet_golden.py: the
shader is re-spelled with oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory, compiled against
oracle/ref_build/glsl_cpu.hpp with the runner next to this file (-ffp-contract=off), once per specialisation set -- phase 0 / 1 / 2 x ORTHO
x SKINNED, and FORCE_VISIBLE for phase 2: 16 sets -- run, and the directory is removed: only inputs and outputs are kept.

    python tests/golden/make_meshlet_cull_golden.py [output.npz]

One fix-up is made on the temporary copy: main() declares `AABB aabb = aabb.data[...]`, a local that in GLSL starts to exist after its
initialiser and in C++ before it, where it would hide the buffer it reads; the local is renamed.

A case runs every set whose ORTHO flag matches the projection its scene was built for, so each case is stored for both projections.
Every dispatch of a case runs on the same output and occluder buffers, one after the other.  Outputs start filled with the poison byte
0xcd, count words zero; an output buffer is stored as its count words and, per record in buffer order, {list, chunk, task}, after asserting
that the scene's draws, these and the poison give the buffer back dword for dword (meshlet_cull_cases.expand_output).  The archive is written with fixed time stamps, so that a second run gives the same bytes.

Prints, per case, on how many records and occluder words tests/meshlet_cull_ref.py differs from the shader (the order of tasks in the
output is the shader's groups in order, which the restatement follows, so the buffers are compared as they are), asserts that this is
zero, and asserts the coverage the case list is there for: every reject cause rejects and every accept path accepts at least once, and
no case other than `all` and `none_*` has an empty or a full list in any set (a case of a single task, tasks_1, can only have a full list
under SKINNED, and is exempt there)."""
import ctypes as C
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import meshlet_cull_cases as mc  # noqa: E402
import meshlet_cull_ref as ref  # noqa: E402
import shader_runner as sr  # noqa: E402

SHADER = os.path.join(sr.SHADERS, "meshlet_cull.comp")


def fn_name(phase, flags):
    return f"ref_meshlet_cull_{mc.set_name(phase, flags)}"


def rename_the_shadowed_aabb(text):
    for old, new in (("AABB aabb = aabb.data[", "AABB task_aabb = aabb.data["), ("frustum_cull(aabb.lo, aabb.hi)", "frustum_cull(task_aabb.lo, task_aabb.hi)")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    return text


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), [SHADER], patch=rename_the_shadowed_aabb)
    variants = []
    for phase, f in mc.sets():
        name = fn_name(phase, f)
        spec = [f"-DCULL_FN={name}", f"-DMESHLET_RENDER_PHASE={phase}", f"-DSPEC_ORTHO={'true' if f & ref.ORTHO else 'false'}",
                f"-DSPEC_SKINNED={'true' if f & ref.SKINNED else 'false'}", f"-DSPEC_FORCE_VISIBLE={'true' if f & ref.FORCE_VISIBLE else 'false'}"]
        variants.append((name, spec))
    assert len(variants) == 16
    objs = sr.compile_runner(tmp, os.path.join(HERE, "meshlet_cull_runner.cpp"), variants, extra=["-pthread", "-fno-strict-aliasing"], jobs=4)
    return sr.link(os.path.join(tmp, "libmeshlet_cull_runner.so"), objs, extra=["-pthread"])


class CullRun(C.Structure):
    _fields_ = [("tasks", C.c_void_p), ("aabbs", C.c_void_p), ("transforms", C.c_void_p), ("bounds", C.c_void_p), ("draws", C.c_void_p), ("occluders", C.c_void_p),
                ("output", C.c_void_p), ("chain", C.c_void_p), ("chain_width", C.c_int32), ("chain_height", C.c_int32), ("chain_levels", C.c_int32),
                ("push", C.c_uint32 * 4), ("camera", C.c_float * 3), ("frustum", C.c_uint32 * 56)]


def run_shader(lib, scene, phase, flags):
    keep = {k: np.ascontiguousarray(scene[k]) for k in ("tasks", "aabbs", "transforms", "bounds", "draws", "chain")}
    occluders, output = np.array(scene["occluders"], np.uint32), np.array(scene["output"], np.uint32)
    fn = getattr(lib, fn_name(phase, flags))
    fn.restype = C.c_uint32
    for push in scene["dispatches"]:
        run = CullRun(*[a.ctypes.data for a in (keep["tasks"], keep["aabbs"], keep["transforms"], keep["bounds"], keep["draws"], occluders, output, keep["chain"])],
                      scene["chain_width"], scene["chain_height"], scene["chain_levels"], (C.c_uint32 * 4)(*[int(v) for v in push]),
                      (C.c_float * 3)(*[float(v) for v in scene["camera"]]), (C.c_uint32 * 56)(*[int(v) for v in scene["frustum"]]))
        outside = fn(C.byref(run))
        assert outside == 0, f"{outside} texel fetches outside their level"
    return output, occluders


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


REJECTS = [f"aabb_plane_{i}_reject" for i in range(6)] + [f"chunk_plane_{i}_reject" for i in range(6)] + [
    "aabb_hiz_reject", "chunk_hiz_reject", "chunk_cone_reject", "chunk_bit_clear", "task_word_zero", "task_word_cleared", "chunk_drawn_in_phase_1"]
ACCEPTS = ["aabb_accept", "chunk_accept", "aabb_hiz_accept", "chunk_hiz_accept", "aabb_near_accept", "chunk_near_accept", "chunk_cone_accept", "chunk_no_cone",
           "delta_0", "delta_1", "delta_2", "delta_3", "delta_many", "lod_at_min", "lod_at_max", "lod_between", "span_left", "span_right", "span_top", "span_bottom",
           "taps_1", "taps_2x", "taps_2y", "taps_4"]
DIRECTED_COVERAGE = {  # what a directed case is there for: each of these is non-zero in that case alone
    "aabb_planes": [f"aabb_plane_{i}_reject" for i in range(6)] + ["aabb_accept"],
    "sphere_planes": [f"chunk_plane_{i}_reject" for i in range(6)] + ["chunk_accept"],
    "cone": ["chunk_cone_reject", "chunk_cone_accept", "chunk_no_cone"],
    "transforms": ["chunk_plane_0_reject", "chunk_accept"],
    "near_straddle": ["chunk_near_accept", "chunk_hiz_accept"],
    "occlusion": ["aabb_hiz_reject", "aabb_hiz_accept", "chunk_hiz_reject", "chunk_hiz_accept"],
    "pixel_spans": ["delta_0", "delta_1", "delta_2", "delta_3", "delta_many", "taps_1", "taps_2x", "taps_2y", "taps_4"],
    "pixel_spans_a": ["delta_0", "delta_1", "delta_2", "delta_3", "delta_many"],
    "lod_clamp": ["lod_at_min", "lod_at_max", "lod_between"],
    "span_sides": ["span_left", "span_right", "span_top", "span_bottom"],
    "phase_words": ["task_word_zero", "task_word_cleared", "chunk_bit_clear", "chunk_drawn_in_phase_1"],
}


def generate(path):
    if not os.path.isfile(SHADER):
        raise FileNotFoundError(SHADER)
    record = {}
    chain_table = mc.chains()
    for key, (flat, w, h, levels) in chain_table.items():
        record[f"chain/{key}"] = flat
        record[f"chain/{key}/shape"] = np.array([w, h, levels], np.int32)
    total = ref.Info()
    with sr.scratch("meshlet_cull_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        for name in mc.CASE_NAMES:
            differ, compared = 0, 0
            mine = ref.Info()
            for ortho in (0, 1):
                scene = mc.build_case(name, ortho, chain_table)
                assert np.all(scene["output"][mc.COUNT_WORDS:] == ref.POISON_WORD) and not scene["output"][:mc.COUNT_WORDS].any()
                for a, value in mc.pack_scene(scene).items():
                    if ortho == 0 or not np.array_equal(record[f"{name}/o0/{a}"], value):
                        record[f"{name}/o{ortho}/{a}"] = value
                chunks = sum((int(t[3]) & 31) + 1 for d in scene["dispatches"] for t in scene["tasks"][int(d[0]):int(d[0]) + int(d[1])])
                for phase, flags in mc.sets():
                    if bool(flags & ref.ORTHO) != bool(ortho):
                        continue
                    output, occluders = run_shader(lib, scene, phase, flags)
                    want_output, want_occluders, info = mc.run_reference(scene, phase, flags)
                    differ += int((output != want_output).sum()) + int((occluders != want_occluders).sum())
                    compared += len(output) + len(occluders)
                    mc.assert_same(scene, output, occluders, want_output, want_occluders, f"{name} {mc.set_name(phase, flags)}")
                    for k, v in info.items():
                        mine[k] += v
                        total[k] += v
                    drawn = sum(int(output[m]) for m in mc.dispatches_lists(scene["dispatches"]))
                    assert drawn == info["draws"]
                    if not (name == "all" or name.startswith("none_") or (name == "tasks_1" and flags & ref.SKINNED)):
                        for m in mc.dispatches_lists(scene["dispatches"]):
                            in_list = sum((int(t[3]) & 31) + 1 for d in scene["dispatches"] if int(d[2]) == m for t in scene["tasks"][int(d[0]):int(d[0]) + int(d[1])])
                            assert 0 < int(output[m]) < in_list, (name, phase, flags, m, int(output[m]), in_list)
                    key = f"{name}/{mc.set_name(phase, flags)}"
                    counts, rows = mc.compact_output(scene, output)
                    assert np.array_equal(mc.expand_output(scene, counts, rows), output), f"{key}: the buffer is more than its records and the poison"
                    record[key] = mc.pack_result(scene, output, occluders)
            for cause in DIRECTED_COVERAGE.get(name, []):
                assert mine[cause] > 0, f"{name}: nothing hit {cause}"
            print(f"{name:16s} {len(scene['tasks']):3d} tasks {chunks:5d} chunks  {compared:7d} dwords compared, meshlet_cull_ref differs on {differ}")
            assert differ == 0, name
        for cause in REJECTS + ACCEPTS:
            assert total[cause] > 0, f"nothing hit {cause}"
        print("coverage: " + ", ".join(f"{k} {total[k]}" for k in REJECTS + ACCEPTS))
    write_npz(path, record)
    stored = np.load(path)
    for name in mc.CASE_NAMES:  # what a test will read is what was recorded
        for ortho in (0, 1):
            scene, back = mc.build_case(name, ortho, chain_table), mc.golden_scene(stored, name, ortho)
            assert all(np.array_equal(scene[a], back[a]) for a in mc.SCENE_ARRAYS + ("chain",)), name
    print(f"{path}: {os.path.getsize(path)} bytes, {len(mc.CASE_NAMES)} cases x 16 sets")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "meshlet_cull_shader_v1.npz"))
