"""TEST SUPPORT.  A writer of the MESHLET4 container and the case list of tests/golden/meshlet_decode_shader_v1.npz.

The reference tree holds no MESHLET4 file, and its exporter needs a library this project does not carry, so every input is synthetic:
streams are built field by field from chosen counts, bit widths, base values, aux fields and element values, and packed in the exporter's
bit order (scene-export/meshlet_export.cpp write_bits: element i, component c, bit b of a stream of C components of `bits` bits goes to
bit (i * C + c) * bits + b of the stream's words, least significant bit of a word first; a stream takes ceil(count * C * bits / 32)
words).

Classes (cases()):
  pos_bits_B      positions with B in 0, 1, 5, 8, 11, 12, 16 bits
  pos_bits_B      B in 13, 14, 15 on the three-component stream, where the exporter itself says the window breaks (it forces 16 bits):
                  the last component can start past bit 63 - B of the window and loses its high bits -- in the shader and in this
                  project alike, since it is the same arithmetic; the golden pins that
  uv_bits_B       B in 0 .. 16
  byte_bits_B     B in 0 .. 8 for normal/tangent, bone indices and bone weights at once
  wrap_16, wrap_8 base + delta past 0xffff and 0xff
  exp_E           exponents -20, -7, -1, 0, 3, 9 on positions and UV
  tangent_mode_A  aux 1, 2, 3 on the oct8 stream (and 0, which decodes as 1 does)
  counts_P_V      prim / vert counts 0, 1, 31, 32 in every pairing that matters
  tail_pad, tail_nopad   the last stream ends exactly at the payload's last word, its last element starting in that word, with the
                  exporter's zero padding word after it and without
  wireframe, textured    files of the two smaller styles
  offsets         non-zero push offsets, nine meshlets with unequal counts (two chunks)
Every case is decoded for every target style its file provides and for the three index widths."""
import os
import struct

import numpy as np

import meshlet_ref as mr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "meshlet_decode_shader_v1.npz")
COMPONENTS = {0: 3, 1: 3, 2: 4, 3: 2, 4: 4, 5: 4}
WIDTH = {1: 16, 2: 8, 3: 16, 4: 8, 5: 8}  # bits of a decoded component
STREAMS_OF_STYLE = {0: 2, 1: 4, 2: 6}
INDEX_FLAGS = (mr.UNROLLED_MESH, mr.INDEX_16, 0)


def pack(values, bits):
    """(n, C) unsigned values -> uint32 words, write_bits's order"""
    values = np.asarray(values, np.uint64)
    total = values.size * bits
    words = np.zeros((total + 31) // 32, np.uint32)
    if bits == 0:
        return words
    assert int(values.max(initial=0)) < (1 << bits)
    flat = values.reshape(-1)
    stream_bits = ((flat[:, None] >> np.arange(bits, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    stream_bits = np.concatenate([stream_bits, np.zeros(len(words) * 32 - total, np.uint8)])
    return np.packbits(stream_bits, bitorder="little").view(np.uint32).copy()


def stream(kind, bits, values, base=None, aux=0):
    """One attribute stream: values (n, C) deltas below 2^bits, base (C,) of the component width, aux the field at bits >> 16"""
    c = COMPONENTS[kind]
    base = np.zeros(c, np.int64) if base is None else np.asarray(base, np.int64)
    return dict(kind=kind, bits=bits, aux=aux, base=base, values=np.asarray(values, np.int64).reshape(-1, c))


def base_words(s):
    c, b = COMPONENTS[s["kind"]], s["base"]
    if WIDTH[s["kind"]] == 16:
        return [int(b[0]) | (int(b[1]) << 16), int(b[2]) if c == 3 else 0]
    return [int(b[0]) | (int(b[1]) << 8) | (int(b[2]) << 16) | (int(b[3]) << 24), 0]


def build_file(style, meshlets, padding=True, stream_count=None, header_overrides=None):
    """meshlets: list of dict(prims=(P, 3) values below 32, vert_count=V, streams=[stream(...) for kinds 1 ..]).
    header_overrides: {(meshlet, stream, field): value} applied to the written Stream records (field 0 .. 3), for refusals."""
    stream_count = STREAMS_OF_STYLE[style] if stream_count is None else stream_count
    payload, records = [], []
    at = 0
    for m in meshlets:
        prims = np.asarray(m["prims"], np.int64).reshape(-1, 3)
        words = pack(prims, 5)
        records.append([len(prims), m["vert_count"], 0, at])
        payload.append(words)
        at += len(words)
        assert len(m["streams"]) == stream_count - 1
        for s in m["streams"]:
            words = pack(s["values"], s["bits"])
            records.append(base_words(s) + [s["bits"] | ((s["aux"] & 0xffff) << 16), at])
            payload.append(words)
            at += len(words)
    records = np.array(records, np.uint32).reshape(len(meshlets), stream_count, 4)
    for (m, s, f), value in (header_overrides or {}).items():
        records[m, s, f] = value
    payload = np.concatenate(payload) if payload else np.zeros(0, np.uint32)
    if len(payload) == 0:
        payload = np.zeros(1, np.uint32)  # a file of empty meshlets: the format has no payload of zero words
    chunks = (len(meshlets) + 7) // 8
    bounds = np.arange((len(meshlets) + chunks) * 8, dtype=np.float32)
    out = mr.MAGIC + struct.pack("<4I", style, stream_count, len(meshlets), len(payload)) + bounds.tobytes() + records.tobytes() + payload.tobytes()
    return out + (b"\0\0\0\0" if padding else b"")


def random_meshlet(rng, style, prim_count, vert_count, pos_bits=11, uv_bits=9, byte_bits=5, exponent=-7, tangent_mode=3, wrap=False):
    def field(kind, bits, aux):
        c, width = COMPONENTS[kind], WIDTH[kind]
        values = rng.integers(0, 1 << bits, (vert_count, c)) if bits else np.zeros((vert_count, c), np.int64)
        top = (1 << width) - 1
        base = rng.integers(top - (1 << bits) // 2, top + 1, c) if wrap else rng.integers(0, top + 1 - ((1 << bits) - 1), c)
        return stream(kind, bits, values, np.clip(base, 0, top), aux)
    streams = [field(1, pos_bits, exponent)]
    if style >= 1:
        streams += [field(2, byte_bits, tangent_mode), field(3, uv_bits, exponent)]
    if style >= 2:
        streams += [field(4, byte_bits, 0), field(5, byte_bits, 0)]
    return dict(prims=rng.integers(0, 32, (prim_count, 3)), vert_count=vert_count, streams=streams)


def random_file(seed, style, counts, padding=True, **kw):
    rng = np.random.default_rng(seed)
    return build_file(style, [random_meshlet(rng, style, p, v, **kw) for p, v in counts], padding)


def tail_file(padding):
    """The last stream (bone weights, 8 bits x 4) of the last meshlet: 32 elements of 32 bits fill 32 words exactly, so the last
    element starts in the payload's last word and its window's second word is word payload_size_words."""
    rng = np.random.default_rng(77)
    meshlets = [random_meshlet(rng, 2, 17, 23), random_meshlet(rng, 2, 32, 32, byte_bits=8)]
    return build_file(2, meshlets, padding)


def cases():
    """name -> (file bytes, primitive_offset, vertex_offset, runtime_style)"""
    out = {}
    mixed = [(5, 7), (32, 32), (1, 3)]
    for b in (0, 1, 5, 8, 11, 12, 13, 14, 15, 16):
        out[f"pos_bits_{b}"] = (random_file(100 + b, 2, mixed, pos_bits=b), 0, 0, mr.MESHLET)
    for b in range(17):
        out[f"uv_bits_{b}"] = (random_file(200 + b, 1, [(3, 32), (9, 11)], uv_bits=b), 0, 0, mr.MESHLET)
    for b in range(9):
        out[f"byte_bits_{b}"] = (random_file(300 + b, 2, [(4, 32), (2, 13)], byte_bits=b), 0, 0, mr.MESHLET)
    out["wrap_16"] = (random_file(400, 1, mixed, pos_bits=12, uv_bits=12, wrap=True), 0, 0, mr.MESHLET)
    out["wrap_8"] = (random_file(401, 2, mixed, byte_bits=6, wrap=True), 0, 0, mr.MESHLET)
    for e in (-20, -7, -1, 0, 3, 9):
        out[f"exp_{e}"] = (random_file(500 + e, 1, [(7, 19)], exponent=e), 0, 0, mr.MESHLET)
    for a in (0, 1, 2, 3):
        out[f"tangent_mode_{a}"] = (random_file(600 + a, 1, [(6, 32), (3, 5)], tangent_mode=a, byte_bits=8), 0, 0, mr.MESHLET)
    for p, v in ((0, 0), (0, 1), (1, 1), (1, 0), (31, 31), (32, 32), (31, 32), (32, 1)):
        out[f"counts_{p}_{v}"] = (random_file(700 + 33 * p + v, 2, [(p, v), (2, 3)]), 0, 0, mr.MESHLET)
    out["tail_pad"] = (tail_file(True), 0, 0, mr.MESHLET)
    out["tail_nopad"] = (tail_file(False), 0, 0, mr.MESHLET)
    out["wireframe"] = (random_file(800, 0, mixed), 0, 0, mr.MDI)
    out["textured"] = (random_file(801, 1, mixed), 0, 0, mr.MDI)
    nine = [(5, 7), (1, 1), (32, 32), (0, 4), (9, 30), (31, 2), (12, 12), (3, 3), (8, 20)]
    out["offsets"] = (random_file(900, 2, nine), 11, 5, mr.MDI)
    return out


def sets_of(style):
    """(target_style, flags) for a file of `style`"""
    return [(t, f) for t in range(style + 1) for f in INDEX_FLAGS]


def capacities(counts, primitive_offset, vertex_offset, tail=3):
    return int(counts[:, 0].sum()) + primitive_offset + tail, int(counts[:, 1].sum()) + vertex_offset + tail


def golden():
    """name -> dict(file, push (2,), runtime_style, and per (target, flags) the four uint8 output buffers of mr.decode's layout)"""
    data = np.load(GOLDEN)
    out = {}
    for key in data.files:
        name, rest = key.split("/", 1)
        out.setdefault(name, {})[rest] = data[key]
    return out


def golden_outputs(case, target_style, flags, guard=mr.GUARD):
    """The recorded buffers of one set: streams the target style does not write are guard, as recorded once per case"""
    vertices = len(case["positions"]) // 12
    return {"indices": case[f"indices{mr.index_bytes(flags)}"], "positions": case["positions"],
            "attributes": case["attributes"] if target_style >= 1 else np.full(vertices * 16, guard, np.uint8),
            "skin": case["skin"] if target_style >= 2 else np.full(vertices * 8, guard, np.uint8)}
