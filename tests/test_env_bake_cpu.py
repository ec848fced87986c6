"""CPU: the environment-bake ABI where it needs no device: symbols bound in both libraries, every refusal of gr_env_equirect_to_cube /
gr_env_specular / gr_env_diffuse against the device-less HIP stand-in of tests/hip_stub (its code and message, zero launches), and the
command line of tools/convert_equirect_to_environment.py."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from granite_amd import app as gapp
from granite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")


def test_symbols_are_bound():
    lib = gapp.load_library()
    assert "gra_environment_bake" in gapp.EXPORTED_SYMBOLS and hasattr(lib, "gra_environment_bake")
    for name in ("gr_env_equirect_to_cube", "gr_env_specular", "gr_env_diffuse", "gr_cube_chain_bytes", "gr_cube_chain_offset"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.load_library(), name)
    assert hasattr(gapp.Application, "bake_environment")


WORKER = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from granite_amd import capi
stub = C.CDLL(%(stub)r); stub.hip_stub_count.restype = C.c_uint64; stub.hip_stub_count.argtypes = [C.c_char_p]
gr = capi.Context(0)
src, out = capi.DeviceBuffer(gr, 1 << 16), capi.DeviceBuffer(gr, 1 << 20)
half4 = capi.FORMAT_R16G16B16A16_SFLOAT
def counted(fn):
    before = stub.hip_stub_count(b"launches")
    code = fn()
    return [code, gr.lib.gr_last_error(gr.handle).decode() if code < 0 else "", stub.hip_stub_count(b"launches") - before]
def equirect(cube=out.ptr, size=5, levels=3, fmt=half4, ptr=src.ptr, w=16, h=8, pitch=128, image=True):
    img = C.byref(capi.Image(ptr, w, h, pitch, fmt)) if image else None
    return counted(lambda: gr.lib.gr_env_equirect_to_cube(gr.handle, None, img, cube, size, levels))
def specular(src_ptr=src.ptr, src_size=8, src_levels=4, out_ptr=out.ptr, out_size=8, out_levels=4, cube=True):
    c = C.byref(capi.Cube(src_ptr, src_size, src_levels)) if cube else None
    return counted(lambda: gr.lib.gr_env_specular(gr.handle, None, c, out_ptr, out_size, out_levels))
def diffuse(src_ptr=src.ptr, src_size=8, src_levels=4, out_ptr=out.ptr, out_size=4, cube=True):
    c = C.byref(capi.Cube(src_ptr, src_size, src_levels)) if cube else None
    return counted(lambda: gr.lib.gr_env_diffuse(gr.handle, None, c, out_ptr, out_size))
print(json.dumps({
    "equirect_ok": equirect(), "specular_ok": specular(), "diffuse_ok": diffuse(),
    "equirect_format": equirect(fmt=capi.FORMAT_R8G8B8A8_UNORM), "equirect_size0": equirect(size=0), "equirect_levels": equirect(levels=4),
    "equirect_levels0": equirect(levels=0), "equirect_null_cube": equirect(cube=None), "equirect_null_image": equirect(image=False),
    "equirect_null_ptr": equirect(ptr=None), "equirect_unaligned": equirect(cube=out.ptr + 8), "equirect_pitch": equirect(pitch=120),
    "specular_null_src": specular(cube=False), "specular_null_ptr": specular(src_ptr=None), "specular_null_out": specular(out_ptr=None),
    "specular_size0": specular(out_size=0), "specular_levels": specular(out_levels=5), "specular_src_levels": specular(src_levels=5),
    "specular_unaligned": specular(src_ptr=src.ptr + 4),
    "diffuse_null_src": diffuse(cube=False), "diffuse_null_out": diffuse(out_ptr=None), "diffuse_size0": diffuse(out_size=0),
    "diffuse_src_size0": diffuse(src_size=0), "diffuse_unaligned": diffuse(out_ptr=out.ptr + 2),
}))
'''


def test_refusals_need_no_device_and_launch_nothing():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT, "stub": STUB}], env=dict(os.environ, LD_PRELOAD=STUB),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["equirect_ok"] == [0, "", 3]  # level 0 and two blits
    assert out["specular_ok"] == [0, "", 1] and out["diffuse_ok"] == [0, "", 1]
    INVALID, UNSUPPORTED = -1, -3
    for key, code, text in (("equirect_format", UNSUPPORTED, "not R16G16B16A16_SFLOAT"), ("equirect_size0", INVALID, "size 0"),
                            ("equirect_levels", INVALID, "beyond the chain"), ("equirect_levels0", INVALID, "beyond the chain"),
                            ("equirect_null_cube", INVALID, "null pointer"), ("equirect_null_image", INVALID, "equirect"),
                            ("equirect_null_ptr", INVALID, "equirect->ptr"), ("equirect_unaligned", INVALID, "16-byte aligned"),
                            ("equirect_pitch", INVALID, "pitch"), ("specular_null_src", INVALID, "src"), ("specular_null_ptr", INVALID, "null pointer"),
                            ("specular_null_out", INVALID, "null pointer"), ("specular_size0", INVALID, "size 0"),
                            ("specular_levels", INVALID, "beyond the chain"), ("specular_src_levels", INVALID, "beyond the chain"),
                            ("specular_unaligned", INVALID, "16-byte aligned"), ("diffuse_null_src", INVALID, "src"),
                            ("diffuse_null_out", INVALID, "null pointer"), ("diffuse_size0", INVALID, "size 0"), ("diffuse_src_size0", INVALID, "size 0"),
                            ("diffuse_unaligned", INVALID, "16-byte aligned")):
        got = out[key]
        assert got[0] == code and text in got[1] and got[2] == 0, (key, got)


def tool():
    spec = importlib.util.spec_from_file_location("convert_equirect_to_environment", os.path.join(ROOT, "tools", "convert_equirect_to_environment.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_tool_command_line():
    p = tool().parser()
    a = p.parse_args(["--reflection", "r.gtx", "--irradiance", "i.gtx", "--cube", "c.gtx", "--cube-scale", "0.5", "in.gtx"])
    assert (a.reflection, a.irradiance, a.cube, a.cube_scale, a.equirect) == ("r.gtx", "i.gtx", "c.gtx", 0.5, "in.gtx")
    a = p.parse_args(["in.gtx"])
    assert (a.reflection, a.irradiance, a.cube, a.cube_scale) == (None, None, None, 1.0)
    assert ".hdr" in p.format_help() and "out of scope" in " ".join(p.format_help().split())
    with pytest.raises(SystemExit):
        p.parse_args([])
    with pytest.raises(SystemExit):
        p.parse_args(["a.gtx", "b.gtx"])
    assert tool().main(["in.gtx"]) == 1  # nothing asked for: no device is opened
