"""Worker of tests/test_shadow_abi_cpu.py: runs under the device-less HIP stand-in of tests/hip_stub (LD_PRELOAD, HIP_STUB_TRACE=1) and prints
one JSON document: what the three shadow launchers do with each malformed argument ({case: [code, message, launches]}), what
gra_set_directional_shadows refuses, and the per-frame launch lists of an application with shadows on, switched off again, and never on."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from granite_amd import app as gapp, capi, synth  # noqa: E402
from granite_amd.capi import Image  # noqa: E402

STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")


def mark(text):
    sys.stderr.write(f"=== {text}\n")
    sys.stderr.flush()


def launcher_refusals():
    stub = C.CDLL(STUB)
    stub.hip_stub_count.restype = C.c_uint64
    stub.hip_stub_count.argtypes = [C.c_char_p]
    gr = capi.Context(0)
    lib = gr.lib
    keep, out = [], {}
    W, H = 24, 10

    def image(w, h, fmt):
        pitch = w * capi.FORMAT_BPP[fmt]
        keep.append(capi.DeviceBuffer(gr, pitch * h + 512))
        return Image(keep[-1].ptr, w, h, pitch, fmt)

    def counted(name, fn):
        before = stub.hip_stub_count(b"launches")
        code = fn()
        out[name] = [code, lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]

    def fresh(mode=capi.SHADOW_PCF, layers=4, fmt=capi.FORMAT_D16_UNORM):
        a = capi.DirectionalLightArgs()
        a.albedo, a.normal, a.pbr = image(W, H, capi.FORMAT_R8G8B8A8_SRGB), image(W, H, capi.FORMAT_A2B10G10R10_UNORM_PACK32), image(W, H, capi.FORMAT_R8G8_UNORM)
        a.depth, a.hdr = image(W, H, capi.FORMAT_D32_SFLOAT), image(W, H, capi.FORMAT_R16G16B16A16_SFLOAT)
        a.emissive = a.hdr
        a.mode, a.layers = mode, layers
        for i in range(layers):
            a.shadow_maps[i] = image(8, 6, fmt)
        a.directional.inv_resolution[:] = (1.0 / W, 1.0 / H)
        return a

    def directional(name, change, **kw):
        a = fresh(**kw)
        change(a)
        counted("directional:" + name, lambda: lib.gr_directional_light(gr.handle, None, C.byref(a)))

    def setter(path, value):
        def change(a):
            target = a
            *parents, last = path.split(".")
            for p in parents:
                target = getattr(target, p) if not p.endswith("]") else getattr(target, p.split("[")[0])[int(p.split("[")[1][:-1])]
            setattr(target, last, value)
        return change

    directional("valid", lambda a: None)
    directional("valid_vsm_plain", lambda a: None, mode=capi.SHADOW_VSM, layers=1, fmt=capi.FORMAT_R32G32_SFLOAT)
    directional("valid_wide_d32", lambda a: None, mode=capi.SHADOW_PCF_WIDE, layers=1, fmt=capi.FORMAT_D32_SFLOAT)
    counted("directional:null_args", lambda: lib.gr_directional_light(gr.handle, None, None))
    directional("packed_target", setter("hdr.format", capi.FORMAT_B10G11R11_UFLOAT_PACK32))
    directional("hdr_format", setter("hdr.format", capi.FORMAT_R8G8B8A8_UNORM))
    directional("emissive_format", lambda a: setattr(a, "emissive", image(W, H, capi.FORMAT_B10G11R11_UFLOAT_PACK32)))
    for arg in ("albedo", "normal", "pbr", "depth"):
        directional(arg + "_size", setter(arg + ".width", W - 1))
        directional(arg + "_null", setter(arg + ".ptr", None))
        directional(arg + "_format", setter(arg + ".format", capi.FORMAT_R16_SFLOAT))
    directional("hdr_pitch", setter("hdr.pitch_bytes", W * 8 - 8))
    directional("hdr_pitch_unaligned", setter("hdr.pitch_bytes", W * 8 + 4))
    directional("mode_0", setter("mode", 0))
    directional("mode_4", setter("mode", 4))
    directional("layers_2", setter("layers", 2))
    directional("layers_0", setter("layers", 0))
    directional("flags_directional_bit", setter("flags", capi.LIGHTING_DIRECTIONAL_BIT))
    directional("ao_without_fallback", setter("flags", capi.LIGHTING_AMBIENT_OCCLUSION_BIT))
    directional("ao_null", setter("flags", capi.LIGHTING_AMBIENT_OCCLUSION_BIT | capi.LIGHTING_AMBIENT_FALLBACK_BIT))
    directional("pcf_with_moments", lambda a: None, fmt=capi.FORMAT_R32G32_SFLOAT)
    directional("vsm_with_depth", lambda a: None, mode=capi.SHADOW_VSM)
    directional("layer_2_other_size", setter("shadow_maps[2].height", 5))
    directional("layer_3_other_format", lambda a: a.shadow_maps.__setitem__(3, image(8, 6, capi.FORMAT_D32_SFLOAT)))
    directional("layer_1_null", setter("shadow_maps[1].ptr", None))
    directional("map_too_wide", lambda a: a.shadow_maps.__setitem__(0, Image(a.shadow_maps[0].ptr, 16385, 1, 16385 * 4, capi.FORMAT_D32_SFLOAT)), layers=1, fmt=capi.FORMAT_D32_SFLOAT)
    directional("hdr_is_albedo", lambda a: setattr(a, "albedo", Image(a.hdr.ptr, W, H, W * 4, capi.FORMAT_R8G8B8A8_SRGB)))

    def overlapping_emissive(a):
        a.emissive = Image(a.hdr.ptr + 8, W, H, W * 8, capi.FORMAT_R16G16B16A16_SFLOAT)
    directional("emissive_overlaps_hdr", overlapping_emissive)
    directional("image_above_4_gib", setter("depth.pitch_bytes", 1 << 29))  # x 10 rows: described, never touched

    def moments(name, depth, out_image):
        counted("moments:" + name, lambda: lib.gr_vsm_moments(gr.handle, None, C.byref(depth) if depth else None, C.byref(out_image) if out_image else None))

    moments("valid_d16", image(9, 5, capi.FORMAT_D16_UNORM), image(9, 5, capi.FORMAT_R32G32_SFLOAT))
    moments("valid_d32", image(9, 5, capi.FORMAT_D32_SFLOAT), image(9, 5, capi.FORMAT_R32G32_SFLOAT))
    moments("null_depth", None, image(9, 5, capi.FORMAT_R32G32_SFLOAT))
    moments("null_moments", image(9, 5, capi.FORMAT_D32_SFLOAT), None)
    moments("depth_format", image(9, 5, capi.FORMAT_R32_SFLOAT), image(9, 5, capi.FORMAT_R32G32_SFLOAT))
    moments("moments_format", image(9, 5, capi.FORMAT_D32_SFLOAT), image(9, 5, capi.FORMAT_R16G16B16A16_SFLOAT))
    moments("moments_size", image(9, 5, capi.FORMAT_D32_SFLOAT), image(8, 5, capi.FORMAT_R32G32_SFLOAT))
    shared = image(9, 5, capi.FORMAT_R32G32_SFLOAT)
    moments("shared_bytes", Image(shared.ptr, 9, 5, 9 * 4, capi.FORMAT_D32_SFLOAT), shared)

    def blur(name, src, dst, up=0):
        counted("blur:" + name, lambda: lib.gr_vsm_blur(gr.handle, None, C.byref(src) if src else None, C.byref(dst) if dst else None, up))

    blur("valid_down", image(33, 17, capi.FORMAT_R32G32_SFLOAT), image(16, 8, capi.FORMAT_R32G32_SFLOAT))
    blur("valid_up", image(16, 8, capi.FORMAT_R32G32_SFLOAT), image(33, 17, capi.FORMAT_R32G32_SFLOAT), 1)
    blur("null_in", None, image(16, 8, capi.FORMAT_R32G32_SFLOAT))
    blur("null_out", image(16, 8, capi.FORMAT_R32G32_SFLOAT), None)
    blur("in_format", image(16, 8, capi.FORMAT_R16G16B16A16_SFLOAT), image(16, 8, capi.FORMAT_R32G32_SFLOAT))
    blur("out_format", image(16, 8, capi.FORMAT_R32G32_SFLOAT), image(16, 8, capi.FORMAT_D32_SFLOAT))
    blur("in_place", shared, shared)
    return out


def transforms():
    t = np.zeros((4, 16), np.float32)
    t[:, [0, 5, 10, 15]] = 1.0
    return t


def application_checks():
    out = {"refused": {}, "accepted": {}}
    w, h = 96, 64
    cam = synth.Camera(w, h)
    maps = np.full((4, 6, 8), 30000, np.uint16)

    def application(**kw):
        a = gapp.Application(w, h, cluster_res=(32, 16, 64), **kw)
        a.set_render_parameters(cam.render_params())
        return a

    def attempt(table, name, a, *args):
        try:
            a.set_directional_shadows(*args)
            table[name] = ""
        except capi.GraniteHipError as e:
            table[name] = str(e)

    for name, kw in (("no_lighting", dict(lighting=False)), ("aa_bench", dict(lighting=False, hdr_bloom=False, aa_bench=True)),
                     ("row_bands", dict(strip_index=0, strip_count=2)), ("hdr_packed_float", dict(rt_fp16=False))):
        a = application(**kw)
        attempt(out["refused"], name, a, maps, capi.SHADOW_PCF, transforms(), 0.0)
        a.close()
    a = application()
    attempt(out["refused"], "layers_2", a, maps[:2], capi.SHADOW_PCF, transforms(), 0.0)
    attempt(out["refused"], "layers_3", a, maps[:3], capi.SHADOW_VSM, transforms(), 0.0)
    attempt(out["refused"], "mode_7", a, maps, 7, transforms(), 0.0)
    attempt(out["refused"], "pcf_with_moments", a, np.zeros((1, 4, 4, 2), np.float32), capi.SHADOW_PCF_WIDE, transforms(), 0.0)
    desc = gapp.DirectionalShadows()
    desc.struct_size, desc.mode, desc.layers, desc.width, desc.height, desc.format = C.sizeof(desc) - 8, 1, 1, 4, 4, capi.FORMAT_D16_UNORM
    desc.texels = maps.ctypes.data
    out["refused"]["struct_size"] = "" if a.lib.gra_set_directional_shadows(a.handle, C.byref(desc)) >= 0 else a.lib.gra_last_error(a.handle).decode()
    desc.struct_size, desc.texels = C.sizeof(desc), None
    out["refused"]["null_texels"] = "" if a.lib.gra_set_directional_shadows(a.handle, C.byref(desc)) >= 0 else a.lib.gra_last_error(a.handle).decode()
    desc.texels, desc.width = maps.ctypes.data, 0
    out["refused"]["width_0"] = "" if a.lib.gra_set_directional_shadows(a.handle, C.byref(desc)) >= 0 else a.lib.gra_last_error(a.handle).decode()
    mark("refused setters")
    attempt(out["refused"], "after_refusals_nothing_launched", a, maps[:2], capi.SHADOW_PCF, transforms(), 0.0)
    mark("end")
    a.close()

    # launch lists: never on, on (PCF cascades; VSM from a depth map), and off again
    def prepared():
        a = application()
        a.set_lights(synth.make_lights(cam, 40))
        a.upload_gbuffer(synth.make_gbuffer(cam))
        return a

    def frame(a, name):
        a.render_frames(2, sync=True)  # the first frames fill retained targets
        mark(f"frame {name}")
        a.render_frames(1, sync=True)
        mark("end")

    never = prepared()
    frame(never, "never")
    never.close()
    a = prepared()
    attempt(out["accepted"], "pcf_cascades", a, maps, capi.SHADOW_PCF, transforms(), 0.0)
    frame(a, "pcf_cascades")
    mark("upload vsm")
    attempt(out["accepted"], "vsm_from_depth", a, maps, capi.SHADOW_VSM, transforms(), 0.0)
    mark("end")
    frame(a, "vsm_from_depth")
    attempt(out["accepted"], "off", a, None)
    frame(a, "off")
    a.close()
    return out


if __name__ == "__main__":
    print(json.dumps({"launchers": launcher_refusals(), "app": application_checks()}))
