"""Device-side copies of a tests/decal_cases.py case and the two decal launches on them (tests/test_gpu_decals.py, tools/decal_time.py)."""
import ctypes as C

import numpy as np

import decal_ref as ref
from granite_amd import capi

POISON = 0xCDCDCDCD
TAIL_WORDS = 64


def params_struct(prm):
    s = capi.ClusterParams()
    C.memmove(C.byref(s), prm.tobytes(), 176)
    return s


def poisoned(gr, words):
    """a buffer of `words` + TAIL_WORDS dwords, all poison"""
    return capi.DeviceBuffer(gr, 4 * (words + TAIL_WORDS)).upload(np.full(words + TAIL_WORDS, POISON, np.uint32))


def binning(gr, case):
    """gr_cluster_binning_decal into a poisoned buffer -> (words, tail)"""
    prm = params_struct(case["prm"])
    words = prm.resolution_xy[0] * prm.resolution_xy[1] * prm.num_decals_32
    mvps = capi.DeviceBuffer(gr, max(64, 64 * prm.num_decals)).upload(np.ascontiguousarray(case["mvps"], np.float32).reshape(-1)) if prm.num_decals else None
    out = poisoned(gr, words)
    gr.check(gr.lib.gr_cluster_binning_decal(gr.handle, None, mvps.ptr if mvps else None, out.ptr, C.byref(prm)))
    gr.sync()
    got = out.download(np.uint32)
    return got[:words], got[words:]


def z_ranges(gr, case, num_ranges):
    """gr_cluster_z_range over the case's slice intervals into a poisoned buffer -> (ranges (n, 2), tail)"""
    intervals = np.ascontiguousarray(case["intervals"], np.uint32)
    src = capi.DeviceBuffer(gr, intervals.nbytes).upload(intervals)
    out = poisoned(gr, 2 * num_ranges)
    push = capi.PushZRange(len(intervals), (len(intervals) + 127) // 128, num_ranges)
    gr.check(gr.lib.gr_cluster_z_range(gr.handle, None, src.ptr, out.ptr, C.byref(push)))
    gr.sync()
    got = out.download(np.uint32)
    return got[:2 * num_ranges].reshape(-1, 2), got[2 * num_ranges:]


class ApplyScene:
    """everything gr_decal_apply reads, uploaded once; run() applies the decals to a fresh copy of the albedo"""

    def __init__(self, gr, case):
        self.gr, self.case = gr, case
        w, h = case["width"], case["height"]
        self.albedo = capi.DeviceImage(gr, w, h, capi.FORMAT_R8G8B8A8_SRGB)
        self.depth = capi.DeviceImage(gr, w, h, capi.FORMAT_D32_SFLOAT).upload(np.ascontiguousarray(case["depth"], np.float32))
        self.transforms = capi.DeviceBuffer(gr, capi.TRANSFORMS_SIZE)
        rows = np.ascontiguousarray(case["decal_rows"], np.float32).reshape(-1)
        if len(rows):
            self.transforms.upload(rows, capi.TRANSFORMS_OFFSET_DECALS)
        self.bitmask = capi.DeviceBuffer(gr, max(4, 4 * len(case["bitmask_decal"]))).upload(np.ascontiguousarray(case["bitmask_decal"], np.uint32))
        self.range = capi.DeviceBuffer(gr, 8 * len(case["range_decal"])).upload(np.ascontiguousarray(case["range_decal"], np.uint32))
        self.levels = [capi.DeviceBuffer(gr, 4 * len(t["texels"])).upload(np.ascontiguousarray(t["texels"], np.uint32)) for t in case["textures"]]
        table = (capi.DecalTexture * max(1, len(case["textures"])))()
        for i, t in enumerate(case["textures"]):
            table[i] = capi.DecalTexture(self.levels[i].ptr, t["width"], t["height"], t["num_levels"], t["format"])
        self.table = capi.DeviceBuffer(gr, C.sizeof(table)).upload(np.frombuffer(bytes(table), np.uint8))
        a = capi.DecalApplyArgs()
        a.albedo, a.depth = self.albedo.desc, self.depth.desc
        a.inv_view_projection[:] = [float(v) for v in case["inv_view_projection"]]
        a.cluster = params_struct(case["prm"])
        a.transforms, a.bitmask_decal, a.range_decal, a.textures = self.transforms.ptr, self.bitmask.ptr, self.range.ptr, self.table.ptr
        a.num_textures = len(case["textures"])
        self.args = a

    def run(self):
        """-> the albedo words (h, w) after gr_decal_apply on a fresh upload of the case's albedo"""
        self.albedo.upload(np.ascontiguousarray(self.case["albedo"], np.uint32))
        self.gr.check(self.gr.lib.gr_decal_apply(self.gr.handle, None, C.byref(self.args)))
        self.gr.sync()
        return self.albedo.download().reshape(self.case["height"], self.case["width"], 4).copy().view(np.uint32)[..., 0]


def reference_bytes(colour, albedo, touched):
    """the albedo words the float colour stores to: sRGB-encoded where a decal reached, the input elsewhere; alpha always the input's"""
    e = ref.srgb_encode_bytes(colour).astype(np.uint32)
    stored = e[..., 0] | (e[..., 1] << 8) | (e[..., 2] << 16) | (np.asarray(albedo, np.uint32) & np.uint32(0xFF000000))
    return np.where(touched, stored, albedo)
