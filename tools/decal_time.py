"""Volumetric decals (csrc/decal.hip) on the synthetic G-buffer at 3840 x 2160 with the viewer's 128 x 64 x 4096 clusters: device-event
times of gr_cluster_binning_decal and gr_decal_apply with 0, 64 and 1024 synthetic decals (synth.make_decals on the default surface, three
textures: 16 x 4 with its full chain, 8 x 8 with one level, 256 x 256 with its full chain).

The library's own event brackets around each entry point (gr_timing_*): 2 warm-up calls, then 50 calls, three rounds, every one printed.
With 0 decals neither entry point launches; the line says so instead of quoting a time.  The timed apply calls run in place on one
albedo image, one after another (the work per call is the same); after them one call on a fresh copy says how many pixels the decals change.

    timeout -k 10 300 python tools/decal_time.py > profiles/decal_time.txt
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decal_cases as dc  # noqa: E402
import decal_device as dev  # noqa: E402
import decal_ref as ref  # noqa: E402
from granite_amd import capi, synth  # noqa: E402

W, H, RES = 3840, 2160, synth.CLUSTER_RESOLUTION


def build_case(cam, gbuf, count, textures):
    rp = cam.render_params()
    descs = synth.make_decals(cam, count, len(textures))
    order = ref.host_sort_order(descs["transform"], rp[99:102]) if count else np.zeros(0, np.int64)
    rows = descs["transform"][order]
    extent = ref.z_slice_extent(rp[103], RES[2])
    intervals = np.array([ref.compute_uint_range(*ref.decal_z_range(r, rp[96:99], rp[99:102]), extent, RES[2]) for r in rows] or [ref.EMPTY_RANGE], np.uint32)
    prm = dc.cluster_params(cam, RES[:2], count)
    prm["z_max_index"] = RES[2] - 1
    prm["z_scale"] = np.float32(1.0) / extent
    return {"width": W, "height": H, "prm": prm, "mvps": np.stack([ref.host_mvp(rp[32:48], r) for r in rows]) if count else np.zeros((0, 16), np.float32),
            "intervals": intervals, "decal_rows": np.stack([ref.host_world_to_texture(r) for r in rows]) if count else np.zeros((0, 12), np.float32),
            "albedo": gbuf["albedo"], "depth": gbuf["depth"], "inv_view_projection": rp[80:96], "textures": [textures[int(i)] for i in descs["texture"][order]]}


def event_us(gr, name, run):
    run()
    run()
    gr.sync()
    gr.timing_reset()
    for _ in range(50):
        run()
    gr.sync()
    count, ms = gr.timing_query().get(name, (0, 0.0))[:2]
    return ms * 1e3 / count if count else None


def main():
    gr = capi.Context(0)
    cam = synth.Camera(W, H)
    gbuf = synth.make_gbuffer(cam)
    textures = [synth.make_decal_texture(16, 4, 5, True), synth.make_decal_texture(8, 8, 1, False), synth.make_decal_texture(256, 256, 9, True)]
    gr.timing_enable(True)
    for count in (0, 64, 1024):
        case = build_case(cam, gbuf, count, textures)
        prm = dev.params_struct(case["prm"])
        words = RES[0] * RES[1] * prm.num_decals_32
        mvps = capi.DeviceBuffer(gr, max(64, case["mvps"].nbytes)).upload(case["mvps"].reshape(-1)) if count else None
        bitmask = capi.DeviceBuffer(gr, max(4, 4 * words))
        run_binning = lambda: gr.check(gr.lib.gr_cluster_binning_decal(gr.handle, None, mvps.ptr if mvps else None, bitmask.ptr, C.byref(prm)))
        case["bitmask_decal"] = np.zeros(max(words, 1), np.uint32)
        case["range_decal"], _ = dev.z_ranges(gr, case, RES[2])
        scene = dev.ApplyScene(gr, case)
        scene.args.bitmask_decal = bitmask.ptr
        scene.albedo.upload(np.ascontiguousarray(gbuf["albedo"], np.uint32))
        run_apply = lambda: gr.check(gr.lib.gr_decal_apply(gr.handle, None, C.byref(scene.args)))
        for round_ in range(3):
            b, a = event_us(gr, "cluster_binning_decal", run_binning), event_us(gr, "decal_apply", run_apply)
            text = lambda v: "no launch" if v is None else f"{v:8.1f} us"
            print(f"{W} x {H}, {RES[0]} x {RES[1]} x {RES[2]} clusters, {count:4d} decals, round {round_}: binning {text(b)};  apply {text(a)}")
        reached = int((scene.run() != gbuf["albedo"]).sum())
        print(f"{W} x {H}, {count:4d} decals: {reached} of {W * H} pixels changed by a decal")
    gr.timing_enable(False)
    gr.close()


if __name__ == "__main__":
    main()
