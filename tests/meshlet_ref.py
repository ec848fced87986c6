"""TEST SUPPORT.  A numpy restatement of the MESHLET4 decode and of decode_mesh's host arithmetic, written from the format's description
(vulkan/mesh/meshlet.hpp, inc/meshlet_payload_decode.h, inc/meshlet_attribute_decode.h), not from granite_amd/csrc/meshlet_decode.hpp.

Container: magic "MESHLET4"; FormatHeader {style, stream_count, meshlet_count, payload_size_words}; meshlet_count Bounds of 32 bytes;
ceil(meshlet_count / 8) chunk Bounds; meshlet_count * stream_count Streams {base_value[2], bits, offset_in_words}; the payload words,
with or without one zero padding word after them.

Payload: element i of a stream of C components of `bits` bits starts at bit i * bits * C of the stream's words, and is read through the
64 bits of two consecutive words; component k is the window >> ((start & 31) + k * bits), truncated to 32 bits, then masked to `bits`
bits (0 bits: 0).  A word at or past payload_size_words reads as 0.  Components are base + delta, wrapped to 16 or 8 bits.

tests/golden/make_meshlet_golden.py holds this file to the executed shader, element for element."""
import struct

import numpy as np

MAGIC = b"MESHLET4"
CHUNK = 8
WIREFRAME, TEXTURED, SKINNED = 0, 1, 2
UNROLLED_MESH, INDEX_16 = 1, 2
MDI, MESHLET = 0, 1
GUARD = 0xCD


def index_bytes(flags):
    return 4 if flags & UNROLLED_MESH else (2 if flags & INDEX_16 else 1)


def parse(data):
    """bytes -> dict(style, stream_count, meshlet_count, payload_words, bounds, chunk_bounds, streams (M, S, 4) uint32, payload uint32)"""
    data = bytes(data)
    assert data[:8] == MAGIC
    style, stream_count, meshlet_count, payload_words = struct.unpack_from("<4I", data, 8)
    at = 24
    bounds = np.frombuffer(data, np.float32, meshlet_count * 8, at).reshape(-1, 8)
    at += meshlet_count * 32
    chunks = (meshlet_count + CHUNK - 1) // CHUNK
    chunk_bounds = np.frombuffer(data, np.float32, chunks * 8, at).reshape(-1, 8)
    at += chunks * 32
    streams = np.frombuffer(data, np.uint32, meshlet_count * stream_count * 4, at).reshape(meshlet_count, stream_count, 4)
    at += meshlet_count * stream_count * 16
    payload = np.frombuffer(data, np.uint32, payload_words, at)
    return dict(style=style, stream_count=stream_count, meshlet_count=meshlet_count, payload_words=payload_words, bounds=bounds,
                chunk_bounds=chunk_bounds, streams=streams, payload=payload)


def counts_of(streams):
    """(M, 2) {prim_count, vert_count}"""
    return streams[:, 0, :2].astype(np.int64)


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------------
def offsets(counts, runtime_style, flags):
    """decode_mesh's per-meshlet Offsets {primitive_output_offset, vertex_output_offset, index_offset}, (M, 3) uint32.
    index_offset: the Meshlet runtime never grows it; MDI grows it by vert_count; MDI that is not unrolled restarts it every 8 meshlets."""
    out = np.zeros((len(counts), 3), np.uint32)
    prim = vert = index = 0
    for i, (p, v) in enumerate(counts):
        if runtime_style == MDI and not flags & UNROLLED_MESH and i % CHUNK == 0:
            index = 0
        out[i] = (prim & 0xffffffff, vert & 0xffffffff, index & 0xffffffff)
        prim, vert = prim + int(p), vert + int(v)
        if runtime_style != MESHLET:
            index += int(v)
    return out


def indirect(counts, runtime_style, primitive_offset=0, vertex_offset=0):
    """upload_indirect_buffer.  Meshlet: (8 * chunks, 4) uint32 {primitive_offset, vertex_offset, primitive_count, vertex_count}, zero
    past the last meshlet.  MDI: (chunks, 3) uint32 {indexCount, firstIndex, vertexOffset}, one per chunk of 8."""
    chunks = (len(counts) + CHUNK - 1) // CHUNK
    prim, vert = primitive_offset, vertex_offset
    if runtime_style == MESHLET:
        out = np.zeros((chunks * CHUNK, 4), np.uint32)
        for i, (p, v) in enumerate(counts):
            out[i] = (prim & 0xffffffff, vert & 0xffffffff, p, v)
            prim, vert = prim + int(p), vert + int(v)
        return out
    out = np.zeros((chunks, 3), np.uint32)
    for c in range(chunks):
        part = counts[c * CHUNK:(c + 1) * CHUNK]
        out[c] = ((3 * int(part[:, 0].sum())) & 0xffffffff, (3 * prim) & 0xffffffff, vert & 0xffffffff)
        prim, vert = prim + int(part[:, 0].sum()), vert + int(part[:, 1].sum())
    return out


# ---- payload --------------------------------------------------------------------------------------------------------------------------
def _words(payload, index):
    index = index.astype(np.int64) & 0xffffffff
    inside = index < len(payload)
    return np.where(inside, payload[np.where(inside, index, 0)], 0).astype(np.uint64)


def extract(payload, offset_in_words, bits, components):
    """offset_in_words, bits: (M,) -> (M, 32, components) uint32, every lane decoded whether or not it is counted"""
    lane = np.arange(32, dtype=np.int64)[None, :]
    bits = bits.astype(np.int64)[:, None]
    first = lane * bits * components
    word = offset_in_words.astype(np.int64)[:, None] + first // 32
    window = _words(payload, word) | (_words(payload, word + 1) << np.uint64(32))
    out = np.zeros(first.shape + (components,), np.uint32)
    mask = np.where(bits >= 32, 0xffffffff, (1 << np.minimum(bits, 32)) - 1).astype(np.uint64)
    for k in range(components):
        shift = (first & 31) + k * bits
        v = np.where(shift < 64, window >> np.minimum(shift, 63).astype(np.uint64), 0) & np.uint64(0xffffffff)
        out[..., k] = (v & mask).astype(np.uint32)
    return out


def _bytes4(payload, s):
    value = extract(payload, s[:, 3], s[:, 2] & 0xff, 4).astype(np.int64)
    base = np.stack([(s[:, 0] >> (8 * i)) & 0xff for i in range(4)], -1).astype(np.int64)
    return value + base[:, None, :]


def _oct(fx, fy):
    one, zero = np.float32(1), np.float32(0)
    z = one - np.abs(fx) - np.abs(fy)
    t = np.maximum(-z, zero)
    x = fx + np.where(fx >= zero, -t, t)
    y = fy + np.where(fy >= zero, -t, t)
    length = np.sqrt(x * x + y * y + z * z)
    return x / length, y / length, z / length


def _quantize(v, scale, mask):
    scaled = (np.minimum(np.maximum(v, np.float32(-1)), np.float32(1)) * np.float32(scale)).astype(np.float64)
    rounded = np.where(scaled >= 0, np.floor(scaled + 0.5), np.ceil(scaled - 0.5)).astype(np.int64)  # round(): half away from zero
    return (rounded & mask).astype(np.uint32)


def pack_a2bgr10(x, y, z, w):
    return (_quantize(w, 1, 3) << 30) | (_quantize(z, 511, 1023) << 20) | (_quantize(y, 511, 1023) << 10) | _quantize(x, 511, 1023)


def unorm4x8_round_trip(byte):
    """packUnorm4x8(unpackUnorm4x8(.)) of one byte, in fp32"""
    f = np.float32(byte) / np.float32(255)
    return int(np.floor(np.float64(np.minimum(np.maximum(f, np.float32(0)), np.float32(1)) * np.float32(255)) + 0.5))


def decode_lanes(streams, payload, target_style):
    """Every lane of every meshlet: dict of prims (M, 32, 3) uint32 without index_offset, positions (M, 32, 3) float32,
    attributes (M, 32, 4) uint32 {normal, tangent, uv bits}, skin (M, 32, 2) uint32."""
    with np.errstate(all="ignore"):
        out = {"prims": extract(payload, streams[:, 0, 3], np.full(len(streams), 5), 3)}
        s = streams[:, 1]
        exponent = (s[:, 2].astype(np.int32) >> 16)[:, None, None]
        base = np.stack([s[:, 0] & 0xffff, s[:, 0] >> 16, s[:, 1] & 0xffff], -1).astype(np.int64)
        value = ((extract(payload, s[:, 3], s[:, 2] & 0xff, 3).astype(np.int64) + base[:, None, :]) & 0xffff).astype(np.uint16).view(np.int16)
        out["positions"] = np.ldexp(value.astype(np.float32), exponent).astype(np.float32)
        if target_style >= TEXTURED:
            s = streams[:, 2]
            nt = _bytes4(payload, s)
            aux = (s[:, 2] >> 16)[:, None]
            t_sign = np.where(aux == 3, nt[..., 3] & 1, aux == 2).astype(bool)
            nt[..., 3] = np.where(aux == 3, nt[..., 3] & ~1, nt[..., 3])
            f = (nt & 0xff).astype(np.uint8).view(np.int8).astype(np.float32) / np.float32(127)
            n, t = _oct(f[..., 0], f[..., 1]), _oct(f[..., 2], f[..., 3])
            zero = np.zeros_like(n[0])
            attr = np.zeros(nt.shape[:2] + (4,), np.uint32)
            attr[..., 0] = pack_a2bgr10(*n, zero)
            attr[..., 1] = pack_a2bgr10(*t, np.where(t_sign, np.float32(-1), np.float32(1)))
            s = streams[:, 3]
            exponent = (s[:, 2].astype(np.int32) >> 16)[:, None, None]
            base = np.stack([s[:, 0] & 0xffff, s[:, 0] >> 16], -1).astype(np.int64)
            value = ((extract(payload, s[:, 3], s[:, 2] & 0xff, 2).astype(np.int64) + base[:, None, :]) & 0xffff).astype(np.uint16).view(np.int16)
            uv = (np.float32(0.5) * np.ldexp(value.astype(np.float32), exponent).astype(np.float32) + np.float32(0.5)).astype(np.float32)
            attr[..., 2:] = uv.view(np.uint32)
            out["attributes"] = attr
        if target_style >= SKINNED:
            skin = np.zeros(streams.shape[:1] + (32, 2), np.uint32)
            for k, stream in enumerate((4, 5)):  # weights: unpackUnorm4x8 then packUnorm4x8, the identity on a byte (unorm4x8_round_trip)
                v = _bytes4(payload, streams[:, stream]) & 0xff
                skin[..., k] = (v[..., 0] | (v[..., 1] << 8) | (v[..., 2] << 16) | (v[..., 3] << 24)).astype(np.uint32)
            out["skin"] = skin
    return out


def decode(streams, payload, offs, primitive_offset, vertex_offset, target_style, flags, capacities, guard=GUARD):
    """What one decode leaves in buffers that were filled with `guard`.  capacities: (primitives, vertices).  Returns uint8 arrays
    indices (3 * index_bytes per primitive), positions (12 per vertex), attributes (16), skin (8): streams the style does not write stay
    guard.  Elements past a capacity and counts above 32 are dropped, as the kernel drops them."""
    lanes = decode_lanes(streams, payload, target_style)
    nb = index_bytes(flags)
    dtype = {4: np.uint32, 2: np.uint16, 1: np.uint8}[nb]
    prim_cap, vert_cap = capacities
    out = {"indices": np.full(prim_cap * 3 * nb, guard, np.uint8), "positions": np.full(vert_cap * 12, guard, np.uint8),
           "attributes": np.full(vert_cap * 16, guard, np.uint8), "skin": np.full(vert_cap * 8, guard, np.uint8)}
    idx = out["indices"].view(dtype).reshape(-1, 3)
    pos, attr, skin = out["positions"].view(np.uint32).reshape(-1, 3), out["attributes"].view(np.uint32).reshape(-1, 4), out["skin"].view(np.uint32).reshape(-1, 2)
    counts = np.minimum(counts_of(streams), 32)
    for m in range(len(streams)):
        p, v = counts[m]
        at = (int(offs[m, 0]) + primitive_offset + np.arange(p)) & 0xffffffff
        keep = at < prim_cap
        idx[at[keep]] = ((lanes["prims"][m, :p].astype(np.int64) + int(offs[m, 2])) & 0xffffffff)[keep].astype(dtype)
        at = (int(offs[m, 1]) + vertex_offset + np.arange(v)) & 0xffffffff
        keep = at < vert_cap
        pos[at[keep]] = lanes["positions"][m, :v].view(np.uint32)[keep]
        if target_style >= TEXTURED:
            attr[at[keep]] = lanes["attributes"][m, :v][keep]
        if target_style >= SKINNED:
            skin[at[keep]] = lanes["skin"][m, :v][keep]
    return out
