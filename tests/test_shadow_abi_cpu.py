"""CPU: the shadow ABI.  include/granite_hip.h declares gr_directional_light, gr_vsm_moments and gr_vsm_blur, include/granite_app.h
gra_set_directional_shadows; the libraries export them, capi and app bind them, and the new structures are the same in C and in ctypes.
gra_config and gra_config_ext keep their layouts: shadows are runtime state.  Under the device-less HIP stand-in of tests/hip_stub
(tests/shadow_app_worker.py) every refusal of the three launchers returns GR_ERR_INVALID_ARGUMENT, names its argument and launches nothing,
every refusal of gra_set_directional_shadows carries its message and launches nothing, and a frame's launch list gains exactly
k_directional_light in front of k_lighting while shadows are on -- and is the list of an application that never had them once they are off."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from granite_amd import app as gapp, capi
from host_program import ROOT, c_layout

HEADER = open(os.path.join(ROOT, "include", "granite_hip.h")).read()
APP_HEADER = open(os.path.join(ROOT, "include", "granite_app.h")).read()
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
INVALID = -1


@pytest.fixture(scope="module")
def worker():
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [STUB, env.get("LD_PRELOAD", "")]))
    env["HIP_STUB_TRACE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shadow_app_worker.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_the_entry_points_are_declared_exported_and_bound():
    assert re.search(r"int gr_directional_light\(gr_ctx \*ctx, gr_stream stream, const gr_directional_light_args \*args\);", HEADER)
    assert re.search(r"int gr_vsm_moments\(gr_ctx \*ctx, gr_stream stream, const gr_image \*depth, const gr_image \*moments\);", HEADER)
    assert re.search(r"int gr_vsm_blur\(gr_ctx \*ctx, gr_stream stream, const gr_image \*in, const gr_image \*out, int up\);", HEADER)
    assert re.search(r"int gra_set_directional_shadows\(gra_app \*app, const gra_directional_shadows \*desc\);", APP_HEADER)
    lib = capi.load_library()
    for name in ("gr_directional_light", "gr_vsm_moments", "gr_vsm_blur"):
        assert name in capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    assert callable(capi.Context.directional_light) and callable(capi.Context.vsm_moments) and callable(capi.Context.vsm_blur)
    host = gapp.load_library()
    assert "gra_set_directional_shadows" in gapp.EXPORTED_SYMBOLS and host.gra_set_directional_shadows.argtypes
    assert callable(gapp.Application.set_directional_shadows)
    assert (capi.SHADOW_PCF, capi.SHADOW_PCF_WIDE, capi.SHADOW_VSM) == (1, 2, 3)
    for name, value in (("GR_SHADOW_PCF", 1), ("GR_SHADOW_PCF_WIDE", 2), ("GR_SHADOW_VSM", 3)):
        assert re.search(rf"#define {name} {value}u", HEADER)


def test_the_structures_are_the_same_in_c_and_in_ctypes(tmp_path):
    for header, c_name, ct in (("granite_hip.h", "gr_directional_light_args", capi.DirectionalLightArgs), ("granite_app.h", "gra_directional_shadows", gapp.DirectionalShadows)):
        fields = [name for name, _ in ct._fields_]
        assert c_layout(tmp_path, c_name, fields, header=header) == [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields], c_name
    assert "GR_ASSERT_SIZE(gr_directional_light_args, 696);" in HEADER and "GR_ASSERT_OFFSET(gr_directional_light_args, transforms, 440);" in HEADER


def test_the_configuration_structures_keep_their_layouts(tmp_path):
    assert gapp.Config._fields_[-1] == ("volumetric_decals", C.c_int32), "gra_config still ends where it ended"
    for c_name, ct in (("gra_config", gapp.Config), ("gra_config_ext", gapp.ConfigExt)):
        fields = [name for name, _ in ct._fields_]
        assert c_layout(tmp_path, c_name, fields, header="granite_app.h") == [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields], c_name
    assert not re.search(r"shadow", re.search(r"typedef struct gra_config\b.*?\} gra_config;", APP_HEADER, re.S).group(0), re.I)
    assert not re.search(r"shadow", re.search(r"typedef struct gra_config_ext\b.*?\} gra_config_ext;", APP_HEADER, re.S).group(0), re.I)


def test_the_kernel_file_is_built_without_contraction():
    makefile = open(os.path.join(ROOT, "granite_amd", "csrc", "Makefile")).read()
    exact = re.search(r"^EXACT_SRCS := (.*)$", makefile, re.M).group(1).split()
    kernels = re.search(r"^KERNEL_SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "shadow.hip" in exact and "shadow.hip" in kernels


NAMES = {  # case -> words its message must hold
    "directional:null_args": ["args"], "directional:packed_target": ["hdr", "B10G11R11_UFLOAT_PACK32"], "directional:hdr_format": ["hdr", "format"],
    "directional:emissive_format": ["emissive", "format"], "directional:hdr_pitch": ["hdr", "pitch_bytes"], "directional:hdr_pitch_unaligned": ["hdr", "multiple of the texel size"],
    "directional:mode_0": ["mode"], "directional:mode_4": ["mode"], "directional:layers_2": ["layers"], "directional:layers_0": ["layers"],
    "directional:flags_directional_bit": ["flags"], "directional:ao_without_fallback": ["AMBIENT_FALLBACK"], "directional:ao_null": ["ambient_occlusion", "null pointer"],
    "directional:pcf_with_moments": ["shadow_maps[0]", "format"], "directional:vsm_with_depth": ["shadow_maps[0]", "format"],
    "directional:layer_2_other_size": ["shadow_maps[2]", "width and height"], "directional:layer_3_other_format": ["shadow_maps[3]", "format"],
    "directional:layer_1_null": ["shadow_maps[1]", "null pointer"], "directional:map_too_wide": ["shadow_maps[0]", "16384"],
    "directional:hdr_is_albedo": ["hdr shares bytes with albedo"], "directional:emissive_overlaps_hdr": ["hdr shares bytes with emissive"],
    "directional:image_above_4_gib": ["depth", "4 GiB"],
    "moments:null_depth": ["depth", "null pointer"], "moments:null_moments": ["moments", "null pointer"], "moments:depth_format": ["depth", "format"],
    "moments:moments_format": ["moments", "format"], "moments:moments_size": ["moments", "width and height"], "moments:shared_bytes": ["moments shares bytes with depth"],
    "blur:null_in": ["in", "null pointer"], "blur:null_out": ["out", "null pointer"], "blur:in_format": ["in", "format"], "blur:out_format": ["out", "format"],
    "blur:in_place": ["out shares bytes with in"],
}
for _arg in ("albedo", "normal", "pbr", "depth"):
    NAMES[f"directional:{_arg}_size"] = [_arg, "width and height"]
    NAMES[f"directional:{_arg}_null"] = [_arg, "null pointer"]
    NAMES[f"directional:{_arg}_format"] = [_arg, "format"]


def test_every_launcher_refusal_names_its_argument_and_launches_nothing(worker):
    got = worker[0]["launchers"]
    valid = [k for k in got if ":valid" in k]
    assert len(valid) == 7
    for case in valid:
        assert got[case] == [0, "", 1], case
    refused = set(got) - set(valid)
    assert refused == set(NAMES), refused ^ set(NAMES)
    for case, words in NAMES.items():
        code, message, launches = got[case]
        assert code == INVALID and launches == 0, (case, got[case])
        entry = {"directional": "gr_directional_light", "moments": "gr_vsm_moments", "blur": "gr_vsm_blur"}[case.split(":")[0]]
        for word in [entry] + words:
            assert word in message, (case, word, message)


def launches(stderr, name):
    body = stderr.split(f"=== {name}\n")[1].split("=== end")[0]
    return [re.sub(r".*?(k_[a-z_0-9]+).*", r"\1", line.split(" ", 2)[2]) for line in body.splitlines() if line.startswith("L ")]


def test_the_application_refuses_with_a_message_and_launches_nothing(worker):
    got, stderr = worker
    refused = got["app"]["refused"]
    for name, words in (("no_lighting", "without lighting"), ("aa_bench", "without lighting"), ("row_bands", "strip_count"), ("hdr_packed_float", "hdr_packed_float"),
                        ("layers_2", "layers must be 1 or 4"), ("layers_3", "layers must be 1 or 4"), ("mode_7", "mode must be"),
                        ("pcf_with_moments", "format does not fit the mode"), ("struct_size", "struct_size"), ("null_texels", "null texels"),
                        ("width_0", "width and height")):
        assert "gra_set_directional_shadows" in refused[name] and words in refused[name], (name, refused[name])
    assert launches(stderr, "refused setters") == []


def test_a_frame_gains_exactly_the_directional_launch(worker):
    got, stderr = worker
    assert got["app"]["accepted"] == {"pcf_cascades": "", "vsm_from_depth": "", "off": ""}
    never = launches(stderr, "frame never")
    assert "k_directional_light" not in " ".join(never) and any(k.startswith("k_lighting") for k in never)
    for name in ("pcf_cascades", "vsm_from_depth"):
        on = launches(stderr, "frame " + name)
        at = next(i for i, k in enumerate(on) if k.startswith("k_directional_light"))
        assert on[at + 1].startswith("k_lighting"), on[at:at + 3]
        assert on[:at] + on[at + 1:] == never, name
    assert launches(stderr, "frame off") == never, "off again: the launches of an application that never had shadows"
    chain = [k for k in launches(stderr, "upload vsm") if k.startswith("k_vsm")]
    assert [re.sub(r"[^a-z_].*", "", k) for k in chain] == ["k_vsm_moments", "k_vsm_blur", "k_vsm_blur"] * 4, "the chain runs on upload, every layer"
