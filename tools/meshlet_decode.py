#!/usr/bin/env python3
"""meshlet_decode.py FILE OUT.npz [--style N] [--index 8|16|32] [--runtime mdi|meshlet]: decode a MESHLET4 mesh file on the GPU
(granite_amd.meshlet.decode) and save indices, positions, attributes, skin and the indirect records as numpy arrays.

meshlet_decode.py --time [FILE]: the time of one decode launch (gr_meshlet_decode) for each index width, on FILE or, without one, on a
synthetic Textured mesh of about a million triangles: 1024 seeded meshlets of 32 primitives and 32 vertices from tests/meshlet_cases.py,
their streams and payload repeated 32 times at their own offsets (32768 meshlets, 1048576 triangles).  Inputs are uploaded once; per
width, 20 warm-up launches, then three rounds of 2000 launches, the widths alternating inside a round; the time is the launcher's own
bracket of device events around each kernel (gr_timing_*), with the wall clock over the same launches beside it.  Printed with it: the
bytes a decode must read (stream headers, payload words, offsets) and write (indices, positions, attributes), from the counts; the
GB/s that gives; and gr_bandwidth_probe's copy rate from the same run, the floor to compare with."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from granite_amd import capi, meshlet  # noqa: E402

INDEX_FLAGS = {8: 0, 16: capi.MESHLET_DECODE_INDEX_16, 32: capi.MESHLET_DECODE_UNROLLED_MESH}


def synthetic(distinct=1024, repeat=32):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import meshlet_cases as mc
    import meshlet_ref as mr
    mesh = mr.parse(mc.random_file(31337, 1, [(32, 32)] * distinct, padding=False))
    streams = np.tile(mesh["streams"], (repeat, 1, 1))
    streams[:, :, 3] += np.repeat(np.arange(repeat, dtype=np.uint32) * mesh["payload_words"], distinct)[:, None]
    return 1, streams, np.tile(mesh["payload"], repeat)


def time_decode(path):
    if path:
        f = meshlet.read(path)
        meshlet.describe(path)  # create_mesh_view's checks
        style, streams, payload = f.style, np.array(f.streams), np.array(f.payload)
        source = path
    else:
        style, streams, payload = synthetic()
        source = "synthetic Textured mesh, seed 31337"
    counts = streams[:, 0, :2].astype(np.int64)
    meshlets, stream_count = streams.shape[:2]
    prims, verts = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    offs = np.zeros((meshlets, 3), np.uint32)  # the Meshlet runtime's: index_offset 0
    offs[1:, 0], offs[1:, 1] = np.cumsum(counts[:-1, 0]), np.cumsum(counts[:-1, 1])
    gr = capi.Context(0)
    dev = {k: capi.DeviceBuffer(gr, v.nbytes).upload(v) for k, v in (("streams", streams), ("payload", payload), ("offsets", offs))}
    out = {"indices": capi.DeviceBuffer(gr, prims * 12), "positions": capi.DeviceBuffer(gr, verts * 12), "attributes": capi.DeviceBuffer(gr, verts * 16),
           "skin": capi.DeviceBuffer(gr, verts * 8)}
    a = capi.MeshletDecodeArgs()
    a.streams, a.payload, a.offsets, a.payload_words, a.stream_count, a.target_style = dev["streams"].ptr, dev["payload"].ptr, dev["offsets"].ptr, len(payload), stream_count, style
    a.indices, a.positions, a.attributes, a.skin = (out[k].ptr for k in ("indices", "positions", "attributes", "skin"))
    a.index_capacity, a.position_capacity, a.attribute_capacity, a.skin_capacity = prims, verts, verts, verts
    read = streams.nbytes + payload.nbytes + offs.nbytes
    print(f"{source}: style {style}, {meshlets} meshlets, {prims} triangles, {verts} vertices, {len(payload)} payload words")
    print("launch shape: 256 threads = 8 meshlets of 32 lanes a workgroup, one launch; the only shape built")
    gr.timing_enable(True)
    warmup, launches = 20, 2000
    for bits, flags in INDEX_FLAGS.items():
        a.flags = flags
        for _ in range(warmup):
            gr.meshlet_decode(a, 0, 0, meshlets)
    gr.sync()
    for round_ in range(3):
        for bits, flags in INDEX_FLAGS.items():
            a.flags = flags
            written = prims * 3 * bits // 8 + verts * 12 + (verts * 16 if style >= 1 else 0) + (verts * 8 if style >= 2 else 0)
            gr.timing_reset()
            t0 = time.perf_counter()
            for _ in range(launches):
                gr.meshlet_decode(a, 0, 0, meshlets)
            gr.sync()
            wall_us = 1e6 * (time.perf_counter() - t0) / launches
            count, total_ms = gr.timing_query()["meshlet_decode"]
            us = 1e3 * total_ms / count
            print(f"index {bits:2d} round {round_}: {us:8.2f} us a decode by device events ({count} launches, {total_ms:7.1f} ms), {wall_us:8.2f} us by the wall clock;  "
                  f"reads {read / 1e6:6.2f} MB, writes {written / 1e6:6.2f} MB, {(read + written) / (us * 1e-6) / 1e9:7.1f} GB/s")
    gr.timing_enable(False)
    copy, triad = capi.C.c_double(), capi.C.c_double()
    gr.check(gr.lib.gr_bandwidth_probe(gr.handle, 256 << 20, 20, capi.C.byref(copy), capi.C.byref(triad)))
    print(f"gr_bandwidth_probe, 256 MiB, 20 repeats: copy {copy.value:7.1f} GB/s, triad {triad.value:7.1f} GB/s")
    gr.close()


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("file", nargs="?")
    p.add_argument("out", nargs="?")
    p.add_argument("--time", action="store_true")
    p.add_argument("--style", type=int, default=None)
    p.add_argument("--index", type=int, choices=(8, 16, 32), default=32)
    p.add_argument("--runtime", choices=("mdi", "meshlet"), default="mdi")
    args = p.parse_args()
    if args.time:
        return time_decode(args.file)
    if not args.file or not args.out:
        p.error("FILE and OUT.npz are needed")
    from granite_amd import app as gapp
    application = gapp.Application(64, 64, lighting=False)
    try:
        arrays = meshlet.decode(application, args.file, args.style, INDEX_FLAGS[args.index], meshlet.RUNTIME_MESHLET if args.runtime == "meshlet" else meshlet.RUNTIME_MDI)
    finally:
        application.close()
    np.savez(args.out, **arrays)
    print(f"{args.out}: " + ", ".join(f"{k} {v.shape}" for k, v in arrays.items()))


if __name__ == "__main__":
    main()
