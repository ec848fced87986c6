"""MESHLET4 mesh files (vulkan/mesh/meshlet.hpp): a reader of the container and decode() on the device through the host library's C ABI
(gra_meshlet_describe, gra_meshlet_decode; Granite::Meshlet::create_mesh_view and decode_mesh underneath).

File layout: magic "MESHLET4"; FormatHeader {style, stream_count, meshlet_count, payload_size_words}; meshlet_count Bounds of 32 bytes;
ceil(meshlet_count / 8) chunk Bounds; meshlet_count * stream_count Streams {base_value[2], bits, offset_in_words}; the payload words."""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import app as gapp
from . import capi
from .capi import MESHLET_DECODE_INDEX_16, MESHLET_DECODE_UNROLLED_MESH

MAGIC = b"MESHLET4"
CHUNK_FACTOR = 8
STYLE_WIREFRAME, STYLE_TEXTURED, STYLE_SKINNED = 0, 1, 2
RUNTIME_MDI, RUNTIME_MESHLET = 0, 1


class MeshletError(RuntimeError):
    pass


@dataclass
class MeshletFile:
    style: int
    stream_count: int
    meshlet_count: int
    payload_size_words: int
    bounds: np.ndarray        # (meshlet_count, 8) float32: centre, radius, cone axis and cutoff
    chunk_bounds: np.ndarray  # (ceil(meshlet_count / 8), 8) float32
    streams: np.ndarray       # (meshlet_count, stream_count, 4) uint32
    payload: np.ndarray       # (payload_size_words,) uint32

    @property
    def counts(self) -> np.ndarray:
        """(meshlet_count, 2) uint32 {prim_count, vert_count}"""
        return self.streams[:, 0, :2]


def describe(path: str) -> gapp.MeshletInfo:
    """Counts and totals of the file, through create_mesh_view's checks; no device."""
    info = gapp.MeshletInfo()
    err = C.create_string_buffer(512)
    if gapp.load_library().gra_meshlet_describe(str(path).encode(), C.byref(info), err, len(err)) < 0:
        raise MeshletError(err.value.decode())
    return info


def read(path: str) -> MeshletFile:
    """The container's sections as arrays.  The sizes are checked; what a decode needs beyond them is describe()'s to check."""
    data = open(path, "rb").read()
    if len(data) < 24 or data[:8] != MAGIC:
        raise MeshletError(f"{path}: not a MESHLET4 file")
    style, stream_count, meshlet_count, payload_words = struct.unpack_from("<4I", data, 8)
    chunks = (meshlet_count + CHUNK_FACTOR - 1) // CHUNK_FACTOR
    sizes = (meshlet_count * 32, chunks * 32, meshlet_count * stream_count * 16, payload_words * 4)
    if len(data) < 24 + sum(sizes):
        raise MeshletError(f"{path}: the file is shorter than its header says")
    at, parts = 24, []
    for size, dtype in zip(sizes, (np.float32, np.float32, np.uint32, np.uint32)):
        parts.append(np.frombuffer(data, dtype, size // 4, at))
        at += size
    return MeshletFile(style, stream_count, meshlet_count, payload_words, parts[0].reshape(-1, 8), parts[1].reshape(-1, 8),
                       parts[2].reshape(meshlet_count, stream_count, 4), parts[3])


def decode(application: "gapp.Application", path: str, target_style: Optional[int] = None, flags: int = 0, runtime_style: int = RUNTIME_MDI,
           primitive_offset: int = 0, vertex_offset: int = 0, guard: int = 0) -> Dict[str, np.ndarray]:
    """Decode the file on the application's device.  Returns indices (P, 3) of uint32 / uint16 / uint8 by `flags`, positions (V, 3) float32,
    attributes (V, 4) uint32 {normal, tangent as A2BGR10, uv as two float bit patterns} for target_style >= 1, skin (V, 2) uint32 {bone
    indices, bone weights} for target_style 2, and indirect: (8 * chunks, 4) uint32 {primitive_offset, vertex_offset, primitive_count,
    vertex_count} for RUNTIME_MESHLET, (chunks, 3) uint32 {indexCount, firstIndex, vertexOffset} for RUNTIME_MDI.  P and V include the
    two offsets; the elements before them hold the byte `guard`."""
    info = describe(path)
    target_style = info.style if target_style is None else int(target_style)
    dtype = np.uint32 if flags & MESHLET_DECODE_UNROLLED_MESH else (np.uint16 if flags & MESHLET_DECODE_INDEX_16 else np.uint8)
    prims, verts = primitive_offset + info.total_primitives, vertex_offset + info.total_vertices

    def filled(shape, dt):
        a = np.empty(shape, dt)
        a.view(np.uint8)[...] = guard
        return a
    out = {"indices": filled((prims, 3), dtype), "positions": filled((verts, 3), np.float32)}
    if target_style >= STYLE_TEXTURED:
        out["attributes"] = filled((verts, 4), np.uint32)
    if target_style >= STYLE_SKINNED:
        out["skin"] = filled((verts, 2), np.uint32)
    out["indirect"] = filled((info.chunk_count * CHUNK_FACTOR, 4) if runtime_style == RUNTIME_MESHLET else (info.chunk_count, 3), np.uint32)
    r = gapp.MeshletRequest()
    r.flags, r.target_style, r.runtime_style, r.primitive_offset, r.vertex_offset = int(flags), target_style, int(runtime_style), int(primitive_offset), int(vertex_offset)
    for key, a in out.items():
        setattr(r, key, a.ctypes.data if a.nbytes else None)
        setattr(r, key + "_bytes", a.nbytes)
    application.decode_meshlet(path, r)
    return out


class CullScene:
    """The buffers gr_meshlet_cull reads and writes, uploaded from arrays: tasks (T, 5) uint32, aabbs (A, 8) float32, transforms (N, 12)
    float32, bounds (B, 8) float32, draws (B, 3) uint32, occluders (O,) uint32, output (D,) uint32 as it is before the first launch (count
    words zero), and optionally the HiZ chain (flat float32, or a capi.DeviceBuffer that gr_hiz wrote) with its width, height and levels."""

    def __init__(self, ctx: "capi.Context", tasks, aabbs, transforms, bounds, draws, occluders, output, chain=None, chain_width=0, chain_height=0, chain_levels=0):
        self.ctx = ctx
        arrays = {"tasks": (tasks, np.uint32, 5), "aabbs": (aabbs, np.float32, 8), "transforms": (transforms, np.float32, 12), "bounds": (bounds, np.float32, 8),
                  "draws": (draws, np.uint32, 3), "occluders": (occluders, np.uint32, 1), "output": (output, np.uint32, 1)}
        self.counts, self.buffers = {}, {}
        for key, (array, dtype, width) in arrays.items():
            a = np.ascontiguousarray(array, dtype).reshape(-1, width)
            self.counts[key] = len(a)
            self.buffers[key] = capi.DeviceBuffer(ctx, max(a.nbytes, 16))
            if a.nbytes:
                self.buffers[key].upload(a)
        if chain is not None and not isinstance(chain, capi.DeviceBuffer):
            chain = capi.DeviceBuffer(ctx, max(np.asarray(chain).nbytes, 16)).upload(np.ascontiguousarray(chain, np.float32))
        self.chain, self.chain_shape = chain, (int(chain_width), int(chain_height), int(chain_levels))

    def reset(self, occluders, output):
        """the occluder words and the output buffer as they are before a launch"""
        for key, array in (("occluders", occluders), ("output", output)):
            a = np.ascontiguousarray(array, np.uint32).ravel()
            assert len(a) == self.counts[key]
            if a.nbytes:
                self.buffers[key].upload(a)

    def args(self, frustum, camera_position, phase: int, flags: int) -> "capi.MeshletCullArgs":
        a = capi.MeshletCullArgs()
        for key, count in (("tasks", "task_count"), ("aabbs", "aabb_count"), ("transforms", "transform_count"), ("bounds", "bound_count"), ("draws", "draw_count"),
                           ("occluders", "occluder_count")):
            setattr(a, key, self.buffers[key].ptr)
            setattr(a, count, self.counts[key])
        a.output, a.output_dwords = self.buffers["output"].ptr, self.counts["output"]
        if self.chain is not None:
            a.chain = self.chain.ptr
            a.chain_width, a.chain_height, a.chain_levels = self.chain_shape
        a.phase, a.flags = int(phase), int(flags)
        a.camera_position[:] = [float(v) for v in camera_position]
        C.memmove(C.byref(a.frustum), np.ascontiguousarray(frustum, np.uint32).ctypes.data, 224)
        return a

    def download(self):
        """(output dwords, occluder words)"""
        self.ctx.sync()
        return self.buffers["output"].download(np.uint32, self.counts["output"]), self.buffers["occluders"].download(np.uint32, self.counts["occluders"])


def cull(scene: CullScene, frustum, camera_position, phase: int, flags: int, offset: int, count: int, mdi_count_offset: int, draw_indirect_offset: int, stream=None):
    """One gr_meshlet_cull launch over `count` tasks from `offset`: survivors are appended as five-dword draw records at
    output[draw_indirect_offset + 5 * slot] behind the count word output[mdi_count_offset].  frustum: the 224-byte block as 56 uint32."""
    scene.ctx.meshlet_cull(scene.args(frustum, camera_position, phase, flags), offset, count, mdi_count_offset, draw_indirect_offset, stream)
