"""The ocean's FFT update called entry point by entry point on a capi.Context: gr_ocean_generate_fft x 3, the three FFT plans with the
ocean's options, gr_ocean_bake_maps, then the mip chains -- gr_spd_downsample for the two RGBA16F chains (3 components, the vertex chain's
last level times (0, 1, 1, 1)) and gr_ocean_mipmap level by level for the RG16F normal chain, or with spd=False every chain level by
level.  What Granite::Ocean::update_fft_pass must reproduce byte for byte."""
import ctypes as C

import numpy as np

import ocean_ref as ocr
from granite_amd import capi, fft

FORMATS = {1: capi.FORMAT_R16_SFLOAT, 2: capi.FORMAT_R16G16_SFLOAT, 4: capi.FORMAT_R16G16B16A16_SFLOAT}
PERIOD = np.float32(256.0 / (2.0 * np.pi))
POISON = 0xA5
ONE = (1.0, 1.0, 1.0, 1.0)
ZERO_FIRST = (0.0, 1.0, 1.0, 1.0)


def as_struct(kind, push):
    return kind.from_buffer_copy(np.ascontiguousarray(push).tobytes())


def poisoned(gr, nbytes, tail=256):
    buf = capi.DeviceBuffer(gr, nbytes + tail)
    gr.check(gr.lib.gr_fill_byte(gr.handle, None, buf.ptr, POISON, nbytes + tail))
    return buf


def run_generate(gr, d, push, variant, bands):
    ny, nx = d.shape[:2]
    src, out = capi.DeviceBuffer(gr, d.nbytes).upload(d), poisoned(gr, 4 * nx * ny)
    gr.ocean_generate_fft(src.ptr, out.ptr, as_struct(capi.PushOceanGenerate, push), variant, bands)
    gr.sync()
    raw = out.download(np.uint8)
    assert np.all(raw[4 * nx * ny:] == POISON), "bytes after out were written"
    return raw[:4 * nx * ny].view(np.uint32).reshape(ny, nx)


def downsample_distribution(d, shift):
    """bin i of the small spectrum is bin alias(i) of the large one, negative frequencies counted from its end"""
    n, m = d.shape[0], d.shape[0] >> shift
    index = np.arange(m)
    index = np.where(index > m // 2, index - m + n, index)
    return np.ascontiguousarray(d[index][:, index])


class Chain:
    """A mip chain in one allocation, level after level tightly packed (gr_mip_chain_offset), with a view per level."""

    def __init__(self, gr, size, channels, levels):
        fmt = FORMATS[channels]
        bpp = capi.FORMAT_BPP[fmt]
        self.channels = channels
        self.buffer = capi.DeviceBuffer(gr, gr.lib.gr_mip_chain_size(size, size, bpp, levels))
        self.views = [capi.DeviceImage(gr, max(size >> l, 1), max(size >> l, 1), fmt, self.buffer.ptr + gr.lib.gr_mip_chain_offset(size, size, bpp, l))
                      for l in range(levels)]

    def download(self):
        return [v.download().reshape(v.height, v.width, self.channels) for v in self.views]


def run_update(gr, height_d, disp_d, normal_d, time, *, world=128.0, normal_mod=7.3, delta=1.0, vertex_levels=5, spd=False, heightmap=True):
    """Returns every buffer as packed half2 and every image level as fp16 bits.  world: heightmap world size; delta: distance between two
    heightmap samples; vertex_levels: levels of the height / displacement chain."""
    f32 = np.float32
    n, m = height_d.shape[0], disp_d.shape[0]
    full = n.bit_length()
    world = f32(world)
    mod_world, mod_normal = f32(2.0) * f32(np.pi) / world, f32(2.0) * f32(np.pi) / (world / f32(normal_mod))
    band_mod = f32(14.0) / f32(n)
    got = {}
    got["height-fft-input"] = run_generate(gr, height_d, ocr.generate_push((mod_world, mod_world), (n, n), band_mod, time, PERIOD), ocr.HEIGHT, None)
    got["displacement-fft-input"] = run_generate(gr, disp_d, ocr.generate_push((mod_world, mod_world), (m, m), band_mod, time, PERIOD),
                                                 ocr.GRADIENT_DISPLACEMENT, None)
    got["normal-fft-input"] = run_generate(gr, normal_d, ocr.generate_push((mod_normal, mod_normal), (n, n), band_mod, time, PERIOD), ocr.GRADIENT_NORMAL, None)

    normal = Chain(gr, n, 2, full)
    gj = Chain(gr, n, 4, full)
    hd = Chain(gr, n, 4, vertex_levels) if heightmap else None
    images = {"height": capi.DeviceImage(gr, n, n, FORMATS[1]), "displacement": capi.DeviceImage(gr, m, m, FORMATS[2]), "normal": normal.views[0]}
    for name, size, mode in (("displacement", m, capi.FFT_INVERSE_C2C), ("height", n, capi.FFT_C2R), ("normal", n, capi.FFT_INVERSE_C2C)):
        plan = fft.Plan(gr, capi.fft_options(size, size, 1, 2, mode, capi.FFT_FP16, capi.FFT_RESOURCE_BUFFER, capi.FFT_RESOURCE_TEXTURE))
        src = capi.DeviceBuffer(gr, 4 * size * size).upload(got[name + "-fft-input"])
        try:
            plan.execute(capi.fft_image_resource(images[name].desc), capi.fft_buffer_resource(src.ptr, src.nbytes, size, size * size))
            gr.sync()
        finally:
            plan.close()
            src.free()
        got[name + "-fft-output"] = images[name].download()

    delta = f32(delta)
    shift = (n // m).bit_length() - 1
    push = ocr.bake_push((f32(1) / f32(n),) * 2 + (f32(1) / f32(m),) * 2, (f32(1) / delta,) * 2 + (f32(1) / (delta * f32(1 << shift)),) * 2)
    gr.ocean_bake_maps(images["height"], images["displacement"], gj.views[0], hd.views[0] if hd else None, as_struct(capi.PushOceanBake, push))
    gr.sync()
    got["bake-push"] = push

    def level_by_level(chain, last_mod):
        for i in range(1, len(chain.views)):
            src, dst = chain.views[i - 1], chain.views[i]
            mod = last_mod if i + 1 == len(chain.views) else ONE
            p = ocr.mipmap_push(mod, (f32(1) / f32(src.width), f32(1) / f32(src.height)), (dst.width, dst.height), float(i - 1))
            gr.ocean_mipmap(src, dst, as_struct(capi.PushOceanMipmap, p))

    def single_pass(chain, last_mod):
        views = chain.views
        args = capi.SpdArgs()
        args.input, args.chain, args.width, args.height = views[0].desc, views[1].ptr, views[1].width, views[1].height
        args.mips, args.components, args.reduction_mode = len(views) - 1, 3, capi.SPD_REDUCTION_COLOR
        mods = None
        if last_mod is not None:
            mods = (C.c_float * (4 * args.mips))(*([1.0] * (4 * (args.mips - 1)) + list(last_mod)))
        args.filter_mods = C.cast(mods, C.c_void_p) if mods is not None else None
        gr.check(gr.lib.gr_spd_downsample(gr.handle, None, C.byref(args)))

    if hd:
        single_pass(hd, ZERO_FIRST) if spd else level_by_level(hd, ZERO_FIRST)
    single_pass(gj, None) if spd else level_by_level(gj, ONE)
    level_by_level(normal, ONE)
    gr.sync()
    got["gradient-jacobian"] = gj.download()
    if hd:
        got["height-displacement"] = hd.download()
    got["normal"] = normal.download()
    return got
