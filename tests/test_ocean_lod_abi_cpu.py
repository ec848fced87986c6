"""CPU: the parts of the LOD update's ABI that need no device, against the device-less HIP stand-in of tests/hip_stub: the push blocks and
records have the shaders' std140 / std430 layout in the ctypes binding (the header asserts the same in C), a valid call of each entry point
costs one launch, everything they refuse is refused with gr_last_error text before a launch, and an ocean whose configuration has a zeroed
tail makes the stub calls it made before the LOD update existed."""
import ctypes as C
import json
import os
import subprocess
import sys

from granite_amd import app as gapp
from granite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")


def offsets(struct):
    return {name: getattr(struct, name).offset for name, *_ in struct._fields_}


def test_struct_sizes_and_offsets():
    u, c = capi.PushOceanUpdateLod, capi.PushOceanCull
    assert C.sizeof(u) == 64
    assert {k: v for k, v in offsets(u).items() if k != "padding"} == dict(shifted_camera_pos=0, max_lod=12, image_offset=16, num_threads=24, grid_base=32,
                                                                           grid_size=40, lod_bias=48)
    assert C.sizeof(c) == 96
    assert {k: v for k, v in offsets(c).items() if not k.startswith("padding")} == dict(
        world_offset=0, image_offset=16, num_threads=24, inv_num_threads=32, grid_base=40, grid_size=48, grid_resolution=56, heightmap_range=64,
        guard_band=72, lod_stride=76, max_lod=80, handle_edge_lods=84)
    assert C.sizeof(capi.OceanPatch) == 32 and offsets(capi.OceanPatch) == dict(offsets=0, inner_lod=8, padding=12, lods=16)
    d = capi.OceanIndirectDraw
    assert C.sizeof(d) == 32 and [getattr(d, n).offset for n, _ in d._fields_] == list(range(0, 32, 4))
    assert [n for n, _ in d._fields_][:5] == ["index_count", "instance_count", "first_index", "vertex_offset", "first_instance"]
    assert C.sizeof(capi.OceanBuffer) == 16 and capi.OCEAN_MAX_LOD_INDIRECT == 8
    # the application's side: the configuration grows at its end only
    cfg = gapp.OceanConfig
    assert (cfg.frequency_bands.offset, cfg.lod_update.offset, cfg.fixed_position.offset, cfg.center_position.offset, C.sizeof(cfg)) == (60, 92, 96, 100, 112)
    assert C.sizeof(gapp.OceanDrawInfo) == 80 and gapp.OceanDrawInfo.lods.offset == 64 and C.sizeof(gapp.OceanMeshInfo) == 24


def test_entry_points_are_bound():
    lib = capi.load_library()
    for name in ("gr_ocean_update_lod", "gr_ocean_init_counter_buffer", "gr_ocean_cull_blocks"):
        assert name in capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    app_lib = gapp.load_library()
    for name in ("gra_ocean_set_camera", "gra_ocean_draw_info", "gra_ocean_mesh_describe", "gra_ocean_mesh_read"):
        assert name in gapp.EXPORTED_SYMBOLS and getattr(app_lib, name).argtypes is not None
    cfg = gapp.OceanConfig()
    cfg.lod_update, cfg.fixed_position = 7, 7
    cfg.center_position[:] = [1.0, 2.0, 3.0]
    app_lib.gra_ocean_default_config(C.byref(cfg))
    assert (cfg.lod_update, cfg.fixed_position, list(cfg.center_position)) == (0, 0, [0.0, 0.0, 0.0]) and cfg.grid_count == 64


WORKER = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from granite_amd import capi
stub = C.CDLL(%(stub)r); stub.hip_stub_count.restype = C.c_uint64; stub.hip_stub_count.argtypes = [C.c_char_p]
gr = capi.Context(0)
N = 16
lods = capi.DeviceImage(gr, N, N, capi.FORMAT_R16_SFLOAT)
patches, counters = capi.DeviceBuffer(gr, N * N * 8 * 32), capi.DeviceBuffer(gr, 8 * 32)
planes = (C.c_float * 24)(*([0.0, 0.0, 0.0, 1.0] * 6))
counts = (C.c_uint32 * 16)(*range(16))
def launches(fn):
    before = stub.hip_stub_count(b"launches")
    code = fn()
    return [code, gr.lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]
def update_push(n=(N, N), max_lod=4.0):
    p = capi.PushOceanUpdateLod(); p.num_threads[:] = n; p.max_lod = max_lod; p.grid_size[:] = [16.0, 16.0]; return p
def cull_push(n=(N, N), max_lod=4.0, stride=N * N):
    p = capi.PushOceanCull(); p.num_threads[:] = n; p.max_lod = max_lod; p.lod_stride = stride; p.grid_size[:] = [16.0, 16.0]; return p
def buf(b, size=None):
    return C.byref(capi.OceanBuffer(b.ptr if b is not None else None, b.nbytes if size is None else size))
def update(image=lods, push=None, null_push=False, desc=None):
    p = None if null_push else C.byref(push or update_push())
    d = desc if desc is not None else (image.desc if image is not None else None)
    return launches(lambda: gr.lib.gr_ocean_update_lod(gr.handle, None, d, p))
def init(b=buf(counters), c=counts):
    return launches(lambda: gr.lib.gr_ocean_init_counter_buffer(gr.handle, None, b, c))
def cull(image=lods, wrap=1, p=buf(patches), c=buf(counters), push=None, null_push=False, frustum=planes):
    ps = None if null_push else C.byref(push or cull_push())
    return launches(lambda: gr.lib.gr_ocean_cull_blocks(gr.handle, None, image.desc if image is not None else None, wrap, p, c, ps, frustum))
rg16, big, r32 = capi.DeviceImage(gr, N, N, capi.FORMAT_R16G16_SFLOAT), capi.DeviceImage(gr, 32, 32, capi.FORMAT_R16_SFLOAT), capi.DeviceImage(gr, N, N, capi.FORMAT_R32_SFLOAT)
l4, l128 = capi.DeviceImage(gr, 4, 4, capi.FORMAT_R16_SFLOAT), capi.DeviceImage(gr, 128, 128, capi.FORMAT_R16_SFLOAT)
p128 = capi.DeviceBuffer(gr, 128 * 128 * 8 * 32)
out = {
    "ok_update": update(), "ok_init": init(), "ok_cull": cull(), "ok_cull_clamp": cull(wrap=0),
    "ok_update_4": update(l4, update_push((4, 4), 0.0)), "ok_update_128": update(l128, update_push((128, 128), 7.0)),
    "ok_cull_128": cull(l128, p=buf(p128), push=cull_push((128, 128), 7.0, 128 * 128)),
    "ok_cull_wide_stride": cull(l4, push=cull_push((4, 4), 7.0, 256)),
    "update_null_image": update(None), "update_null_push": update(null_push=True),
    "update_null_ptr": update(desc=C.byref(capi.Image(None, N, N, 2 * N, capi.FORMAT_R16_SFLOAT))),
    "update_not_square": update(push=update_push((16, 8))), "update_not_pot": update(push=update_push((12, 12))),
    "update_small": update(push=update_push((2, 2))), "update_large": update(push=update_push((256, 256))),
    "update_negative": update(push=update_push((-16, -16))),
    "update_format": update(rg16), "update_format_r32": update(r32), "update_image_size": update(big),
    "update_max_lod_8": update(push=update_push(max_lod=8.0)), "update_max_lod_negative": update(push=update_push(max_lod=-1.0)),
    "update_max_lod_fraction": update(push=update_push(max_lod=2.5)), "update_max_lod_nan": update(push=update_push(max_lod=float("nan"))),
    "init_null_buffer": init(None), "init_null_ptr": init(buf(None, 256)), "init_null_counts": init(c=None), "init_small": init(buf(counters, 255)),
    "cull_null_image": cull(None), "cull_null_patches": cull(p=None), "cull_null_patches_ptr": cull(p=buf(None, 1 << 20)),
    "cull_null_counters": cull(c=None), "cull_null_push": cull(null_push=True), "cull_null_frustum": cull(frustum=None),
    "cull_not_square": cull(push=cull_push((16, 8))), "cull_not_pot": cull(push=cull_push((24, 24))), "cull_small": cull(push=cull_push((2, 2))),
    "cull_large": cull(push=cull_push((256, 256))), "cull_huge": cull(push=cull_push((0x80000010, 0x80000010))),
    "cull_format": cull(rg16), "cull_image_size": cull(big),
    "cull_max_lod_8": cull(push=cull_push(max_lod=8.0)), "cull_max_lod_fraction": cull(push=cull_push(max_lod=0.5)),
    "cull_stride_small": cull(push=cull_push(stride=N * N - 1)),
    "cull_patches_small": cull(p=buf(patches, N * N * 5 * 32 - 1)), "cull_patches_small_for_stride": cull(push=cull_push(stride=N * N * 2)),
    "cull_counters_small": cull(c=buf(counters, 128)),
    "cull_overlap": cull(p=buf(patches), c=C.byref(capi.OceanBuffer(patches.ptr + 1024, 256))),
}
print(json.dumps(out))
'''


def ensure_stub():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])


def run_worker(text):
    ensure_stub()
    r = subprocess.run([sys.executable, "-c", text % {"root": ROOT, "stub": STUB}], env=dict(os.environ, LD_PRELOAD=STUB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_launches_and_refusals_need_no_device():
    out = run_worker(WORKER)
    for key, got in out.items():
        if key.startswith("ok_"):
            assert got == [0, "", 1], (key, got)  # exactly one launch
    texts = {"update_null_image": "lod_image", "update_null_push": "push", "update_null_ptr": "lod_image", "update_not_square": "not square",
             "update_not_pot": "power of two", "update_small": "power of two", "update_large": "power of two", "update_negative": "power of two",
             "update_format": "lod_image", "update_format_r32": "lod_image", "update_image_size": "lod_image",
             "update_max_lod_8": "max_lod", "update_max_lod_negative": "max_lod", "update_max_lod_fraction": "max_lod", "update_max_lod_nan": "max_lod",
             "init_null_buffer": "counters", "init_null_ptr": "counters", "init_null_counts": "counts16", "init_small": "below 8 * 32",
             "cull_null_image": "lod_image", "cull_null_patches": "patches", "cull_null_patches_ptr": "patches", "cull_null_counters": "counters",
             "cull_null_push": "push", "cull_null_frustum": "frustum", "cull_not_square": "not square", "cull_not_pot": "power of two",
             "cull_small": "power of two", "cull_large": "power of two", "cull_huge": "power of two", "cull_format": "lod_image",
             "cull_image_size": "lod_image", "cull_max_lod_8": "max_lod", "cull_max_lod_fraction": "max_lod", "cull_stride_small": "lod_stride",
             "cull_patches_small": "patches has", "cull_patches_small_for_stride": "patches has", "cull_counters_small": "counters has",
             "cull_overlap": "overlap"}
    assert set(texts) == {k for k in out if not k.startswith("ok_")}
    for key, text in texts.items():
        got = out[key]
        assert got[0] == -1 and text in got[1] and got[2] == 0, (key, got)


OCEAN_WORKER = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from granite_amd import app as gapp
from granite_amd import capi
from granite_amd.ocean import Ocean
stub = C.CDLL(%(stub)r); stub.hip_stub_count.restype = C.c_uint64; stub.hip_stub_count.argtypes = [C.c_char_p]
KEYS = ["launches", "memcpys", "memsets", "event_records", "stream_waits", "syncs"]
snap = lambda: [int(stub.hip_stub_count(k.encode())) for k in KEYS]
diff = lambda a, b: [y - x for x, y in zip(a, b)]
a = gapp.Application(64, 64, lighting=False)
CONFIG = dict(fft_resolution=128, displacement_downsample=1, grid_count=4, grid_resolution=32, ocean_size=(128.0, 128.0))
out = {}
for lod in (0, 1):
    for route in (0, 1):
        s0 = snap()
        o = Ocean(a, through_render_graph=route, lod_update=lod, **CONFIG)
        s1 = snap(); o.update(1.5); s2 = snap(); o.update(2.5); s3 = snap()
        exists = [int(o.describe(n).exists) for n in ("ocean-lods", "ocean-lod-counter", "ocean-lod-data")]
        meshes = [int(o.mesh_info(w).exists) * (1 + int(o.mesh_info(w).on_device)) for w in (0, 4, 5, "border")]
        out["lod%%d_route%%d" %% (lod, route)] = {"create": diff(s0, s1), "update1": diff(s1, s2), "update2": diff(s2, s3), "exists": exists, "meshes": meshes}
        o.close()
def refused(**kw):
    before = snap()
    try:
        Ocean(a, **{**CONFIG, **kw})
    except capi.GraniteHipError as e:
        return [str(e), diff(before, snap())]
    return ["", diff(before, snap())]
out["refused"] = {"no_heightmap": refused(lod_update=1, heightmap=0), "count_3": refused(lod_update=1, grid_count=3), "count_256": refused(lod_update=1, grid_count=256),
                  "resolution_48": refused(lod_update=1, grid_resolution=48), "resolution_256": refused(lod_update=1, grid_resolution=256),
                  "resolution_2": refused(lod_update=1, grid_resolution=2)}
print(json.dumps(out))
'''


def test_a_zeroed_tail_is_the_ocean_of_before():
    """launches, memcpys, memsets, event records, stream waits, syncs of creating an ocean and of two updates, direct and through a
    render graph, as counted on the commit before the LOD update existed (same configuration, same stand-in)."""
    out = run_worker(OCEAN_WORKER)
    before = {"route0": {"create": [0, 6, 12, 0, 0, 19], "update1": [21, 0, 0, 0, 0, 4], "update2": [21, 0, 0, 0, 0, 4]},
              "route1": {"create": [0, 6, 4, 0, 0, 11], "update1": [21, 0, 10, 2, 0, 13], "update2": [21, 0, 10, 2, 0, 13]}}
    for route in (0, 1):
        got = out[f"lod0_route{route}"]
        assert {k: got[k] for k in ("create", "update1", "update2")} == before[f"route{route}"], (route, got)
        assert got["exists"] == [0, 0, 0]
        assert got["meshes"] == [1, 1, 0, 1]  # five LOD meshes and the border, read from the host's copy
        # with the LOD update: three more launches an update, and the uploads of five LOD meshes and the border at creation
        lod = out[f"lod1_route{route}"]
        assert lod["exists"] == [1, 1, 1] and lod["meshes"] == [2, 2, 0, 2]
        for update in ("update1", "update2"):
            assert lod[update][0] == got[update][0] + 3, (route, update, lod[update])
        assert lod["create"][0] == 0 and lod["create"][1] == got["create"][1] + 12
    for key, (text, calls) in out["refused"].items():
        assert "LOD update" in text and calls == [0] * 6, (key, text, calls)  # before anything is allocated or uploaded
