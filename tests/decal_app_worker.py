"""Worker of tests/test_decal_app_cpu.py and tests/test_decal_abi_cpu.py: runs under the device-less HIP stand-in of tests/hip_stub
(LD_PRELOAD, HIP_STUB_TRACE=1) and prints one JSON document.  `app`: graphs, per-frame launch lists and the host's packed decal state
of the application in its decal configurations.  `abi`: what the two decal launchers do with each malformed argument."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from granite_amd import app as gapp, capi, synth  # noqa: E402


def mark(text):
    sys.stderr.write(f"=== {text}\n")
    sys.stderr.flush()


def app_worker():
    import decal_cases as dc
    out = {"graphs": {}, "state": {}}
    w, h = 256, 128
    cam = synth.Camera(w, h)
    textures = dc.texture_set()

    def application(**kw):
        a = gapp.Application(w, h, lighting=True, cluster_res=(32, 16, 64), **kw)
        a.set_render_parameters(cam.render_params())
        a.set_lights(synth.make_lights(cam, 40))
        a.upload_gbuffer(synth.make_gbuffer(cam))
        return a

    for name, kw, decals in (("without_field", {}, None), ("off", dict(volumetric_decals=False), None), ("on_no_decals", dict(volumetric_decals=True), 0),
                             ("on_decals", dict(volumetric_decals=True), 5)):
        a = application(**kw)
        if decals is not None:
            for i, t in enumerate(textures):
                a.set_decal_texture(i, t)
            a.set_decals(synth.make_decals(cam, decals, len(textures)))
        out["graphs"][name] = a.graph()
        a.render_frames(2, sync=True)  # the first frames fill retained targets
        mark(f"frame {name}")
        a.render_frames(1, sync=True)
        mark("end")
        a.close()

    # refusals of the application
    a = application(volumetric_decals=True)
    a.set_decal_texture(0, textures[0])
    descs = synth.make_decals(cam, 3, 1)
    descs["texture"][2] = 7
    try:
        a.set_decals(descs)
        out["missing_texture"] = ""
    except capi.GraniteHipError as e:
        out["missing_texture"] = str(e)
    a.close()
    out["refused"] = {}
    for name, kw in (("no_lighting", dict(lighting=False)), ("row_bands", dict(strip_index=0, strip_count=2)), ("aa_bench", dict(lighting=False, hdr_bloom=False, aa_bench=True))):
        try:
            gapp.Application(256, 128, device=-1, volumetric_decals=True, **kw).close()
            out["refused"][name] = ""
        except capi.GraniteHipError as e:
            out["refused"][name] = str(e)

    # host packing on two stored-case scenes, decals handed over back to front
    for name in ("three_overlap_odd", "many"):
        case = dc.apply_case(name)
        cw, ch = case["width"], case["height"]
        ccam = synth.Camera(cw, ch)
        res = tuple(int(v) for v in case["prm"]["resolution_xy"]) + (dc.RES_Z,)
        a = gapp.Application(w, h, lighting=True, cluster_res=res, volumetric_decals=True)  # the frame's size is not the case's: only its camera is
        a.set_render_parameters(ccam.render_params())
        a.upload_gbuffer(synth.make_gbuffer(cam))
        for i, t in enumerate(case["textures"]):
            a.set_decal_texture(i, t)
        n = len(case["world_rows"])
        descs = np.zeros(n, synth.DECAL_DESC_DTYPE)
        descs["transform"] = case["world_rows"][::-1]
        descs["texture"] = np.arange(n)[::-1]
        a.set_decals(descs)
        a.render_frames(1, sync=True)
        state = a.get_decal_state()
        out["state"][name] = {k: v.tolist() for k, v in state.items()}
        a.close()
    print(json.dumps(out))


def abi_worker():
    import decal_cases as dc
    import decal_device as dev
    stub = C.CDLL(os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so"))
    stub.hip_stub_count.restype = C.c_uint64
    stub.hip_stub_count.argtypes = [C.c_char_p]
    gr = capi.Context(0)
    lib = gr.lib
    golden = dc.load_golden()
    out = {}

    def counted(fn):
        before = stub.hip_stub_count(b"launches")
        code = fn()
        return [code, lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]

    case = dc.golden_case(golden, "count_33/32x16")
    mvps = capi.DeviceBuffer(gr, 64 * 33)
    bitmask = capi.DeviceBuffer(gr, 4 * 32 * 16 * 2)

    def binning(change=lambda prm: None, mvps_ptr=mvps.ptr, bitmask_ptr=bitmask.ptr, null_params=False):
        prm = dev.params_struct(case["prm"])
        change(prm)
        return counted(lambda: lib.gr_cluster_binning_decal(gr.handle, None, mvps_ptr, bitmask_ptr, None if null_params else C.byref(prm)))

    def set_decals(n):
        def change(prm):
            prm.num_decals, prm.num_decals_32 = n, (n + 31) // 32
        return change

    out["binning:valid"] = binning()
    out["binning:zero_decals"] = binning(set_decals(0))
    out["binning:zero_decals_null_pointers"] = binning(set_decals(0), None, None)
    out["binning:resolution_xy"] = binning(lambda prm: prm.resolution_xy.__setitem__(0, 36))
    out["binning:resolution_xy zero"] = binning(lambda prm: prm.resolution_xy.__setitem__(1, 0))
    out["binning:num_decals"] = binning(set_decals(4097))
    out["binning:num_decals_32"] = binning(lambda prm: setattr(prm, "num_decals_32", 1))
    out["binning:mvps"] = binning(mvps_ptr=None)
    out["binning:bitmask"] = binning(bitmask_ptr=None)
    out["binning:params"] = binning(null_params=True)

    scene = dev.ApplyScene(gr, dc.golden_case(golden, "two_overlap"))

    def apply(change=lambda a: None):
        a = capi.DecalApplyArgs()
        C.memmove(C.byref(a), C.byref(scene.args), C.sizeof(a))
        change(a)
        return counted(lambda: lib.gr_decal_apply(gr.handle, None, C.byref(a)))

    def zero(a):
        a.cluster.num_decals = a.cluster.num_decals_32 = 0

    def zero_null(a):
        zero(a)
        a.textures = a.transforms = a.bitmask_decal = a.range_decal = None

    out["apply:valid"] = apply()
    out["apply:zero_decals"] = apply(zero)
    out["apply:zero_decals_null_tables"] = apply(zero_null)
    out["apply:args"] = counted(lambda: lib.gr_decal_apply(gr.handle, None, None))
    for field in ("textures", "transforms", "bitmask_decal", "range_decal"):
        out[f"apply:{field}"] = apply(lambda a: setattr(a, field, None))
    out["apply:albedo format"] = apply(lambda a: setattr(a.albedo, "format", capi.FORMAT_R8G8B8A8_UNORM))
    out["apply:albedo ptr"] = apply(lambda a: setattr(a.albedo, "ptr", None))
    out["apply:albedo pitch"] = apply(lambda a: setattr(a.albedo, "pitch_bytes", 4 * 63))
    out["apply:albedo pitch+1"] = apply(lambda a: setattr(a.albedo, "pitch_bytes", 4 * 64 + 1))
    out["apply:depth format"] = apply(lambda a: setattr(a.depth, "format", capi.FORMAT_R8G8B8A8_SRGB))
    out["apply:depth size"] = apply(lambda a: setattr(a.depth, "height", 31))
    out["apply:depth ptr"] = apply(lambda a: setattr(a.depth, "ptr", None))
    out["apply:cluster.resolution_xy"] = apply(lambda a: a.cluster.resolution_xy.__setitem__(0, 33))
    out["apply:cluster.num_decals"] = apply(lambda a: setattr(a.cluster, "num_decals", 5000))
    out["apply:cluster.z_max_index"] = apply(lambda a: setattr(a.cluster, "z_max_index", -1))
    print(json.dumps(out))


if __name__ == "__main__":
    {"app": app_worker, "abi": abi_worker}[sys.argv[1]]()
