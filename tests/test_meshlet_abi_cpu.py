"""CPU: the parts of the mesh-decode ABI that need no device.  Against the device-less HIP stand-in of tests/hip_stub: a valid
gr_meshlet_decode costs exactly one launch, zero meshlets (or a wg_offset past the last group) none, and everything the launcher refuses
is refused with its code and message before a launch.  Without any HIP call: the symbols are in the headers, the libraries and
EXPORTED_SYMBOLS, and every refusal of Granite::Meshlet::create_mesh_view is reached through gra_meshlet_describe with a file from
tests/meshlet_cases.py -- a truncated file at every section boundary among them, a missing padding word accepted."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import meshlet_cases as mc
import meshlet_ref as mr
from granite_amd import app as gapp
from granite_amd import capi, meshlet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")


def test_symbols_are_in_headers_libraries_and_lists():
    hip, app = (open(os.path.join(ROOT, "include", n)).read() for n in ("granite_hip.h", "granite_app.h"))
    assert "int gr_meshlet_decode(" in hip and "GR_ASSERT_SIZE(gr_push_meshlet_decode, 16)" in hip
    assert "int gra_meshlet_describe(" in app and "int gra_meshlet_decode(" in app
    assert "gr_meshlet_decode" in capi.EXPORTED_SYMBOLS and hasattr(capi.load_library(), "gr_meshlet_decode")
    for name in ("gra_meshlet_describe", "gra_meshlet_decode"):
        assert name in gapp.EXPORTED_SYMBOLS and hasattr(gapp.load_library(), name)
    assert C.sizeof(capi.PushMeshletDecode) == 16 and C.sizeof(capi.MeshletDecodeArgs) == 104
    assert (capi.MESHLET_DECODE_UNROLLED_MESH, capi.MESHLET_DECODE_INDEX_16) == (mr.UNROLLED_MESH, mr.INDEX_16)


WORKER = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from granite_amd import capi
stub = C.CDLL(%(stub)r); stub.hip_stub_count.restype = C.c_uint64; stub.hip_stub_count.argtypes = [C.c_char_p]
gr = capi.Context(0)
buf = {k: capi.DeviceBuffer(gr, 1 << 16) for k in ("streams", "payload", "offsets", "indices", "positions", "attributes", "skin")}
def call(stream_count=6, target=2, flags=0, count=9, wg_offset=0, words=100, **ptrs):
    a = capi.MeshletDecodeArgs()
    for k in buf:
        setattr(a, k, ptrs.get(k, buf[k].ptr))
    a.payload_words, a.stream_count, a.target_style, a.flags = words, stream_count, target, flags
    a.index_capacity = a.position_capacity = a.attribute_capacity = a.skin_capacity = 1000
    before = stub.hip_stub_count(b"launches")
    code = gr.lib.gr_meshlet_decode(gr.handle, None, C.byref(a), C.byref(capi.PushMeshletDecode(3, 5, count, wg_offset)))
    return [code, gr.lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]
out = {
    "ok_skinned": call(), "ok_u32": call(flags=1), "ok_u16": call(flags=2), "ok_u16_odd_base": call(flags=2, indices=buf["indices"].ptr + 1),
    "ok_u32_base_plus_1": call(flags=1, indices=buf["indices"].ptr + 1), "ok_target_below_file": call(stream_count=6, target=0),
    "ok_wireframe_no_attr": call(stream_count=2, target=0, attributes=None, skin=None), "ok_textured_no_skin": call(stream_count=4, target=1, skin=None),
    "ok_wg_offset": call(count=17, wg_offset=2), "ok_thousands": call(count=100000),
    "zero_meshlets": call(count=0), "zero_meshlets_null": call(count=0, streams=None, payload=None, indices=None),
    "wg_offset_past": call(count=17, wg_offset=3),
    "streams_3": call(stream_count=3, target=0), "streams_0": call(stream_count=0, target=0), "streams_8": call(stream_count=8),
    "style_3": call(target=3), "textured_of_2": call(stream_count=2, target=1), "skinned_of_4": call(stream_count=4, target=2),
    "flags_4": call(flags=4), "zero_words": call(words=0),
    "null_streams": call(streams=None), "null_payload": call(payload=None), "null_offsets": call(offsets=None), "null_indices": call(indices=None),
    "null_positions": call(positions=None), "null_attributes": call(attributes=None), "null_skin": call(skin=None),
    "null_attributes_textured": call(stream_count=4, target=1, attributes=None),
    "streams_misaligned": call(streams=buf["streams"].ptr + 4), "attributes_misaligned": call(attributes=buf["attributes"].ptr + 8),
    "skin_misaligned": call(skin=buf["skin"].ptr + 4), "positions_misaligned": call(positions=buf["positions"].ptr + 2),
}
null_args = gr.lib.gr_meshlet_decode(gr.handle, None, None, C.byref(capi.PushMeshletDecode(0, 0, 1, 0)))
out["null_args"] = [null_args, gr.lib.gr_last_error(gr.handle).decode(), 0]
print(json.dumps(out))
'''


def test_launches_and_refusals_need_no_device():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT, "stub": STUB}], env=dict(os.environ, LD_PRELOAD=STUB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for key in (k for k in out if k.startswith("ok_")):
        assert out[key] == [0, "", 1], (key, out[key])  # exactly one launch, whatever the meshlet count
    for key in ("zero_meshlets", "zero_meshlets_null", "wg_offset_past"):
        assert out[key] == [0, "", 0], (key, out[key])  # GR_OK without a launch
    refusals = {"streams_3": "stream_count 3 is not 2, 4 or 6", "streams_0": "stream_count 0", "streams_8": "stream_count 8", "style_3": "target_style 3",
                "textured_of_2": "needs 4 streams", "skinned_of_4": "needs 6 streams", "flags_4": "flags 0x4", "zero_words": "zero words",
                "null_streams": "args->streams", "null_payload": "args->payload", "null_offsets": "args->offsets", "null_indices": "args->indices",
                "null_positions": "args->positions", "null_attributes": "args->attributes", "null_skin": "args->skin",
                "null_attributes_textured": "args->attributes", "streams_misaligned": "alignment", "attributes_misaligned": "alignment",
                "skin_misaligned": "alignment", "positions_misaligned": "alignment", "null_args": "args"}
    assert set(refusals) | {k for k in out if k.startswith("ok_")} | {"zero_meshlets", "zero_meshlets_null", "wg_offset_past"} == set(out)
    for key, text in refusals.items():
        got = out[key]
        assert got[0] == -1 and "gr_meshlet_decode" in got[1] and text in got[1] and got[2] == 0, (key, got)


def describe(tmp_path, data):
    path = tmp_path / "mesh.msh4"
    path.write_bytes(data)
    return meshlet.describe(str(path))


def refused(tmp_path, data, text):
    with pytest.raises(meshlet.MeshletError) as e:
        describe(tmp_path, data)
    assert text in str(e.value), str(e.value)


def three_meshlets(**kw):
    rng = np.random.default_rng(5)
    return mc.build_file(2, [mc.random_meshlet(rng, 2, p, v) for p, v in ((5, 7), (32, 32), (1, 3))], **kw)


def test_describe_answers_without_a_device(tmp_path):
    data = three_meshlets()
    info = describe(tmp_path, data)
    mesh = mr.parse(data)
    assert (info.style, info.stream_count, info.meshlet_count, info.payload_size_words) == (2, 6, 3, mesh["payload_words"])
    assert (info.total_primitives, info.total_vertices, info.chunk_count) == (38, 42, 1)
    assert describe(tmp_path, mc.random_file(6, 0, [(1, 1)] * 17)).chunk_count == 3
    f = meshlet.read(str(tmp_path / "mesh.msh4"))
    assert f.meshlet_count == 17 and f.streams.shape == (17, 2, 4) and np.array_equal(f.counts, np.ones((17, 2)))
    empty = describe(tmp_path, mc.random_file(7, 1, []))
    assert (empty.meshlet_count, empty.chunk_count, empty.total_vertices) == (0, 0, 0)


def test_a_missing_padding_word_is_accepted_and_truncation_is_refused_at_every_section(tmp_path):
    padded, bare = three_meshlets(), three_meshlets(padding=False)
    assert len(padded) == len(bare) + 4
    assert describe(tmp_path, bare).total_vertices == describe(tmp_path, padded).total_vertices == 42
    mesh = mr.parse(bare)
    sections = [("too small", 8 + 16), ("meshlet bounds", 3 * 32), ("chunk bounds", 32), ("stream headers", 3 * 6 * 16), ("payload", mesh["payload_words"] * 4)]
    at = 0
    for text, size in sections:
        refused(tmp_path, bare[:at], text)             # the file ends where the section starts
        refused(tmp_path, bare[:at + size - 1], text)  # ... and one byte short of its end
        refused(tmp_path, bare[:at + size - 4], text)
        at += size
    assert at == len(bare)
    refused(tmp_path, b"MESHLET3" + bare[8:], "magic")


def test_every_refusal_names_its_meshlet_and_stream(tmp_path):
    words = mr.parse(three_meshlets())["payload_words"]
    for override, text in (({(1, 0, 0): 33}, "meshlet 1, stream 0: counts 33 and 32 are above 32"),
                           ({(2, 0, 1): 0xffffffff}, "meshlet 2, stream 0: counts"),
                           ({(0, 1, 2): 17 | (0xfff9 << 16)}, "meshlet 0, stream 1: 17 bits per component, above the stream's 16"),
                           ({(1, 3, 2): 255}, "meshlet 1, stream 3: 255 bits"),
                           ({(2, 2, 2): 9 | (3 << 16)}, "meshlet 2, stream 2: 9 bits per component, above the stream's 8"),
                           ({(0, 4, 2): 9}, "meshlet 0, stream 4: 9 bits"), ({(1, 5, 2): 16}, "meshlet 1, stream 5: 16 bits"),
                           ({(1, 0, 3): words - 1}, "meshlet 1, stream 0: words"), ({(2, 1, 3): words}, "meshlet 2, stream 1: words"),
                           ({(0, 5, 3): 0xffffffff}, "meshlet 0, stream 5: words 4294967295"), ({(1, 2, 3): words - 3}, "meshlet 1, stream 2: words")):
        refused(tmp_path, three_meshlets(header_overrides=override), text)
    bare = bytearray(three_meshlets(padding=False))
    for field, value, text in ((8, 3, "style 3"), (12, 4, "has 6 streams, not 4"), (20, 0, "zero words"), (20, words + 1, "ends inside the payload")):
        broken = bytearray(bare)
        broken[field:field + 4] = int(value).to_bytes(4, "little")
        refused(tmp_path, bytes(broken), text)
    # a stream that ends exactly at the payload's last word is no refusal, with or without the padding word
    assert describe(tmp_path, mc.tail_file(False)).meshlet_count == describe(tmp_path, mc.tail_file(True)).meshlet_count == 2
