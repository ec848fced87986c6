"""Records tests/golden/meshlet_decode_shader_v1.npz: the reference's decode/meshlet_decode.comp, executed on the CPU, on the synthetic
MESHLET4 files of tests/meshlet_cases.py.

Needs the reference's sources (REF, as oracle/ref_build/Makefile: default /root/reference).  Same recipe as make_astc_decode_golden.py and
make_ocean_lod_golden.py: the shader is re-spelled with oracle/ref_build/glsl2cpp.py and gen_swizzles.py into a temporary directory,
compiled against oracle/ref_build/glsl_cpu.hpp with the runner next to this file (-ffp-contract=off), once per specialisation set --
file style x target style the file provides x {unrolled, 16-bit, 8-bit} indices, 18 sets -- run, and the directory is removed: only the
input files and the decoded outputs are kept.

    python tests/golden/make_meshlet_golden.py [output.npz]

Every case runs every set of its file's style.  Outputs start filled with the guard byte 0xcd and have three elements of room after the
last one.  The Offsets array is decode_mesh's for the case's runtime style and the set's flags (tests/meshlet_ref.offsets).  The shader
reads word payload_size_words for the last window of a stream that ends at the last word: the runner's payload is the file's with one
zero word after it, which is what the exporter's padding word and robust buffer access give the shader.

What is stored per case: the file, the push offsets, the runtime style, the index buffer per width, and positions, attributes and skin
once -- asserted identical in every set that writes them, and untouched guard in every set that does not.

Prints, per class, how many elements tests/meshlet_ref.py decodes differently, and asserts that this is zero."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "ref_build")]
import meshlet_cases as mc  # noqa: E402
import meshlet_ref as mr  # noqa: E402
import shader_runner as sr  # noqa: E402

SHADER = os.path.join(sr.SHADERS, "decode", "meshlet_decode.comp")


def fn_name(style, target, flags):
    return f"ref_meshlet_s{style}_t{target}_i{mr.index_bytes(flags)}"


def build(tmp):
    sr.respell(os.path.join(tmp, "gen"), [SHADER])
    variants = []
    for style in (0, 1, 2):
        for target, f in mc.sets_of(style):
            name = fn_name(style, target, f)
            spec = [f"-DMESHLET_FN={name}", f"-DSPEC_NUM_U32_STREAMS={mc.STREAMS_OF_STYLE[style]}", f"-DSPEC_TARGET_MESH_STYLE={target}",
                    f"-DSPEC_UNROLLED_MESH={'true' if f & mr.UNROLLED_MESH else 'false'}", f"-DSPEC_INDEX16={'true' if f & mr.INDEX_16 else 'false'}"]
            variants.append((name, spec))
    assert len(variants) == 18
    objs = sr.compile_runner(tmp, os.path.join(HERE, "meshlet_decode_runner.cpp"), variants, jobs=4)
    return sr.link(os.path.join(tmp, "libmeshlet_decode_runner.so"), objs)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_shader(lib, mesh, offs, primitive_offset, vertex_offset, target, flags, caps):
    streams = np.ascontiguousarray(mesh["streams"])
    payload = np.concatenate([mesh["payload"], np.zeros(1, np.uint32)])
    push = np.array([primitive_offset, vertex_offset, mesh["meshlet_count"], 0], np.uint32)
    nb = mr.index_bytes(flags)
    out = {"indices": np.full(caps[0] * 3 * nb, mr.GUARD, np.uint8), "positions": np.full(caps[1] * 12, mr.GUARD, np.uint8),
           "attributes": np.full(caps[1] * 16, mr.GUARD, np.uint8), "skin": np.full(caps[1] * 8, mr.GUARD, np.uint8)}
    getattr(lib, fn_name(mesh["style"], target, flags))(ptr(streams), ptr(payload), ptr(np.ascontiguousarray(offs)), ptr(push), ptr(out["indices"]),
                                                         ptr(out["positions"]), ptr(out["attributes"]), ptr(out["skin"]), C.c_uint32((mesh["meshlet_count"] + 7) // 8))
    return out


def generate(path):
    if not os.path.isfile(SHADER):
        raise FileNotFoundError(SHADER)
    record = {}
    with sr.scratch("meshlet_golden_") as tmp:
        lib = C.CDLL(build(tmp))
        for name, (data, primitive_offset, vertex_offset, runtime_style) in sorted(mc.cases().items()):
            mesh = mr.parse(data)
            counts = mr.counts_of(mesh["streams"])
            caps = mc.capacities(counts, primitive_offset, vertex_offset)
            kept, differ, elements = {}, 0, 0
            for target, flags in mc.sets_of(mesh["style"]):
                offs = mr.offsets(counts, runtime_style, flags)
                got = run_shader(lib, mesh, offs, primitive_offset, vertex_offset, target, flags, caps)
                ref = mr.decode(mesh["streams"], mesh["payload"], offs, primitive_offset, vertex_offset, target, flags, caps)
                for key, stride in (("indices", 3 * mr.index_bytes(flags)), ("positions", 12), ("attributes", 16), ("skin", 8)):
                    differ += int((got[key].reshape(-1, stride) != ref[key].reshape(-1, stride)).any(-1).sum())
                    elements += len(got[key]) // stride
                    written = key in ("indices", "positions") or (key == "attributes" and target >= 1) or (key == "skin" and target >= 2)
                    if not written:
                        assert np.all(got[key] == mr.GUARD), (name, key)
                        continue
                    slot = f"indices{mr.index_bytes(flags)}" if key == "indices" else key
                    assert slot not in kept or np.array_equal(kept[slot], got[key]), (name, slot, target, flags)
                    kept[slot] = got[key]
            print(f"{name:18s} style {mesh['style']}  {mesh['meshlet_count']:2d} meshlets  {mesh['payload_words']:4d} words  {elements:6d} elements compared, meshlet_ref differs on {differ}")
            assert differ == 0, name
            record[f"{name}/file"] = np.frombuffer(data, np.uint8)
            record[f"{name}/push"] = np.array([primitive_offset, vertex_offset], np.uint32)
            record[f"{name}/runtime_style"] = np.array(runtime_style, np.uint32)
            for slot, value in kept.items():
                record[f"{name}/{slot}"] = value
    np.savez_compressed(path, **record)
    print(f"{path}: {os.path.getsize(path)} bytes, {sum(k.endswith('/file') for k in record)} cases")


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "meshlet_decode_shader_v1.npz"))
