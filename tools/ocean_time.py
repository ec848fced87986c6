"""The ocean's FFT update at the reference's default configuration (renderer/ocean.hpp: fft_resolution 1024, displacement 512), chained
entry point by entry point on one stream exactly as Granite::Ocean::update_fft_pass chains it (tests/test_gpu_ocean_pass.py holds the pass
to this chain byte for byte): three gr_ocean_generate_fft, three FFT plans one after the other, gr_ocean_bake_maps, then the mip chains
(gr_spd_downsample for the two RGBA16F chains, gr_ocean_mipmap level by level for the RG16F normal chain).

Two measurements.  Wall clock the way tools/fft_time.py takes it: 2 warm-up calls, then 10 back-to-back calls between two
synchronisations, three rounds, every one printed, for the whole update and for every stage run alone -- beside a device copy (gr_copy)
of the bytes the stage reads and writes.  Then the split inside one update by events: the library's own event brackets around every
entry point (gr_timing_*), summed per stage over 10 updates.  The brackets serialise the launches, so the event split adds up to more
than the wall clock of an update whose launches overlap their latencies.

    timeout -k 10 300 python tools/ocean_time.py > profiles/ocean_time.txt

`python tools/ocean_time.py lod` times the LOD update instead, at the default configuration (grid_count 64, grid_resolution 128, ocean_size
1024, lod_bias -3.5; camera near the origin, every block in view): gr_ocean_update_lod, gr_ocean_init_counter_buffer and
gr_ocean_cull_blocks chained on one stream as Granite::Ocean::update_lod_pass chains them, 30 back-to-back passes between two
synchronisations, three rounds, each launch alone the same way, and the FFT update beside it from the same run.

    timeout -k 10 300 python tools/ocean_time.py lod > profiles/ocean_lod_time.txt
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fft_time import per_call_ms  # noqa: E402
from granite_amd import capi, fft  # noqa: E402

N, SHIFT, VERTEX_LEVELS = 1024, 1, 7  # log2(grid_resolution 128) levels of the height / displacement chain
R16F, RG16F, RGBA16F = capi.FORMAT_R16_SFLOAT, capi.FORMAT_R16G16_SFLOAT, capi.FORMAT_R16G16B16A16_SFLOAT


def lod_pass(gr):
    """-> (stages of the LOD update at the default configuration, the buffers that keep them alive)"""
    count, resolution, size, bias = 64, 128, 1024.0, -3.5
    lods = resolution.bit_length() - 1
    block = size / count
    update = capi.PushOceanUpdateLod((1.3, 4.0, -2.1), float(lods - 1), (-32, -32), (count, count), (-32 * block, -32 * block), (block, block), bias)
    cull = capi.PushOceanCull()
    cull.image_offset[:] = [-32, -32]
    cull.num_threads[:] = [count, count]
    cull.inv_num_threads[:] = [1.0 / count, 1.0 / count]
    cull.grid_base[:] = [-32 * block, -32 * block]
    cull.grid_size[:] = [block, block]
    cull.grid_resolution[:] = [resolution, resolution]
    cull.heightmap_range[:] = [-10.0, 10.0]
    cull.guard_band, cull.lod_stride, cull.max_lod, cull.handle_edge_lods = 5.0, count * count, float(lods - 1), 1
    image = capi.DeviceImage(gr, count, count, R16F)
    patches, counters = capi.DeviceBuffer(gr, count * count * 8 * 32), capi.DeviceBuffer(gr, 8 * 32)
    planes = [0.0, 0.0, 0.0, 1.0] * 6
    # index counts of the seven LOD meshes: size * (2 * (size + 1) + 1)
    counts = [(resolution >> l) * (2 * ((resolution >> l) + 1) + 1) for l in range(lods)] + [0] * (16 - lods)
    stages = {
        "update_lod": lambda: gr.ocean_update_lod(image, update),
        "init_counters": lambda: gr.ocean_init_counter_buffer(counters, counts),
        "cull_blocks": lambda: gr.ocean_cull_blocks(image, 1, patches, counters, cull, planes),
    }

    launches = list(stages.values())

    def whole():
        for call in launches:
            call()

    stages["lod pass"] = whole
    return stages, (image, patches, counters)


def main():
    gr = capi.Context(0)
    rng = np.random.default_rng(0)
    m = N >> SHIFT
    f32 = np.float32
    period = f32(256.0 / (2.0 * np.pi))
    world = f32(128.0)  # 1024 / 64 * 1024 / 128
    mods = {"height": f32(2 * np.pi) / world, "displacement": f32(2 * np.pi) / world, "normal": f32(2 * np.pi) / (world / f32(7.3))}
    sizes = {"height": N, "displacement": m, "normal": N}
    variants = {"height": capi.OCEAN_VARIANT_HEIGHT, "displacement": capi.OCEAN_VARIANT_GRADIENT_DISPLACEMENT, "normal": capi.OCEAN_VARIANT_GRADIENT_NORMAL}
    modes = {"height": capi.FFT_C2R, "displacement": capi.FFT_INVERSE_C2C, "normal": capi.FFT_INVERSE_C2C}
    formats = {"height": R16F, "displacement": RG16F, "normal": RG16F}
    dist, spectra, images, plans, pushes = {}, {}, {}, {}, {}
    for name, n in sizes.items():
        d = (rng.standard_normal((n, n, 2)) * 10.0 ** rng.uniform(-6.0, -2.0, (n, n, 1))).astype(np.float32)
        dist[name] = capi.DeviceBuffer(gr, d.nbytes).upload(d)
        spectra[name] = capi.DeviceBuffer(gr, 4 * n * n)
        images[name] = capi.DeviceImage(gr, n, n, formats[name])
        plans[name] = fft.Plan(gr, capi.fft_options(n, n, 1, 2, modes[name], capi.FFT_FP16, capi.FFT_RESOURCE_BUFFER, capi.FFT_RESOURCE_TEXTURE))
        pushes[name] = capi.PushOceanGenerate((mods[name], mods[name]), (n, n), f32(14.0) / f32(N), 44.0, period)

    def chain_of(fmt, levels):
        bpp = capi.FORMAT_BPP[fmt]
        buf = capi.DeviceBuffer(gr, gr.lib.gr_mip_chain_size(N, N, bpp, levels))
        views = [capi.DeviceImage(gr, max(N >> l, 1), max(N >> l, 1), fmt, buf.ptr + gr.lib.gr_mip_chain_offset(N, N, bpp, l)) for l in range(levels)]
        return buf, views

    full = N.bit_length()
    gj_buf, gj = chain_of(RGBA16F, full)
    hd_buf, hd = chain_of(RGBA16F, VERTEX_LEVELS)
    normal_buf, normal = chain_of(RG16F, full)
    delta = f32(1024.0) / f32(64.0) / f32(128.0)
    bake_push = capi.PushOceanBake((1.0 / N, 1.0 / N, 1.0 / m, 1.0 / m), (1 / delta, 1 / delta, 1 / (delta * 2), 1 / (delta * 2)))
    hd_mods = (C.c_float * (4 * (VERTEX_LEVELS - 1)))(*([1.0] * (4 * (VERTEX_LEVELS - 2)) + [0.0, 1.0, 1.0, 1.0]))

    def generate():
        for name in sizes:
            gr.ocean_generate_fft(dist[name].ptr, spectra[name].ptr, pushes[name], variants[name])

    def transforms():
        for name in ("displacement", "height", "normal"):
            n = sizes[name]
            target = normal[0] if name == "normal" else images[name]
            plans[name].execute(capi.fft_image_resource(target.desc), capi.fft_buffer_resource(spectra[name].ptr, 4 * n * n, n, n * n))

    def bake():
        gr.ocean_bake_maps(images["height"], images["displacement"], gj[0], hd[0], bake_push)

    def spd(views, filter_mods=None):
        args = capi.SpdArgs()
        args.input, args.chain, args.width, args.height = views[0].desc, views[1].ptr, views[1].width, views[1].height
        args.mips, args.components, args.reduction_mode = len(views) - 1, 3, 0
        args.filter_mods = C.cast(filter_mods, C.c_void_p) if filter_mods is not None else None
        gr.check(gr.lib.gr_spd_downsample(gr.handle, None, C.byref(args)))

    def mips():
        spd(hd, hd_mods)
        spd(gj)
        for l in range(1, full):
            src, dst = normal[l - 1], normal[l]
            gr.ocean_mipmap(src, dst, capi.PushOceanMipmap((1, 1, 1, 1), (1.0 / src.width, 1.0 / src.height), (dst.width, dst.height), float(l - 1)))

    def update():
        generate()
        transforms()
        bake()
        mips()

    texels = N * N
    moved = {
        "generate x 3": (2 * texels + m * m) * (8 + 8 + 4),  # a bin, its mirror, the packed result
        "fft x 3": None,
        "bake": texels * (2 + 8 + 8) + m * m * 4,
        "mips": int(texels * 8 * (1 + 2 * 1 / 3)) * 2 + int(texels * 4 * (1 + 2 * 1 / 3)),  # every level written once, all but the last read once
    }
    if sys.argv[1:] == ["lod"]:
        lod_stages, keep = lod_pass(gr)
        for round_ in range(3):
            for name, call in lod_stages.items():
                print(f"{name:14s} round {round_}: {per_call_ms(gr, call, calls=30) * 1e3:8.1f} us a call, 30 back to back")
            print(f"{'fft update':14s} round {round_}: {per_call_ms(gr, update, calls=30) * 1e3:8.1f} us a call, 30 back to back")
        counters = keep[2].download(np.uint32).reshape(8, 8)
        print(f"blocks kept per LOD: {counters[:, 1].tolist()} of {64 * 64}")
        for plan in plans.values():
            plan.close()
        gr.close()
        return
    stages = {"generate x 3": generate, "fft x 3": transforms, "bake": bake, "mips": mips, "update": update}
    scratch_a, scratch_b = capi.DeviceBuffer(gr, 64 << 20), capi.DeviceBuffer(gr, 64 << 20)
    for round_ in range(3):
        for name, call in stages.items():
            ms = per_call_ms(gr, call)
            line = f"{name:14s} round {round_}: {ms * 1e3:8.1f} us"
            if moved.get(name):
                half = moved[name] // 2
                copy_ms = per_call_ms(gr, lambda: gr.check(gr.lib.gr_copy(gr.handle, None, scratch_b.ptr, scratch_a.ptr, half)))
                line += f";  {moved[name] / 1e6:6.1f} MB moved;  copy of those bytes {copy_ms * 1e3:7.1f} us;  ratio {ms / copy_ms:5.2f}"
            print(line)
    # the split inside one update, by the event brackets of the entry points
    events = {"generate x 3": ("ocean_generate_fft",), "fft x 3": ("fft",), "bake": ("ocean_bake_maps",), "mips": ("spd", "ocean_mipmap")}
    gr.timing_enable(True)
    for round_ in range(3):
        update()
        gr.sync()
        gr.timing_reset()
        for _ in range(10):
            update()
        gr.sync()
        q = gr.timing_query()
        total = 0.0
        for name, brackets in events.items():
            count, ms = sum(q.get(b, (0, 0.0))[0] for b in brackets), sum(q.get(b, (0, 0.0))[1] for b in brackets)
            total += ms
            print(f"{name:14s} events {round_}: {ms * 100:8.1f} us an update in {count // 10} brackets")
        print(f"{'sum':14s} events {round_}: {total * 100:8.1f} us an update")
    gr.timing_enable(False)
    for plan in plans.values():
        plan.close()
    gr.close()


if __name__ == "__main__":
    main()
