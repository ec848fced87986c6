"""CPU: the decal ABI.  include/granite_hip.h declares gr_cluster_binning_decal and gr_decal_apply with size and offset assertions on the
new structures, the library exports them, capi binds them, and the structures are the same in C and in ctypes.  Under the device-less HIP
stand-in of tests/hip_stub (tests/decal_app_worker.py): every refusal the launchers document returns GR_ERR_INVALID_ARGUMENT, names the
argument and launches nothing; a valid call launches once; zero decals return GR_OK without a launch, whatever the pointers."""
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
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
INVALID = -1


def run_worker(what, trace=False):
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    env = dict(os.environ)
    env["LD_PRELOAD"] = " ".join(filter(None, [STUB, env.get("LD_PRELOAD", "")]))
    if trace:
        env["HIP_STUB_TRACE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "decal_app_worker.py"), what], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_the_entry_points_are_declared_exported_and_bound():
    assert re.search(r"int gr_cluster_binning_decal\(gr_ctx \*ctx, gr_stream stream, const float \*mvps, uint32_t \*bitmask, const gr_cluster_params \*params\);", HEADER)
    assert re.search(r"int gr_decal_apply\(gr_ctx \*ctx, gr_stream stream, const gr_decal_apply_args \*args\);", HEADER)
    lib = capi.load_library()
    for name in ("gr_cluster_binning_decal", "gr_decal_apply"):
        assert name in capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    host = gapp.load_library()
    for name in ("gra_set_decals", "gra_set_decal_texture", "gra_get_decal_state"):
        assert name in gapp.EXPORTED_SYMBOLS and getattr(host, name).argtypes
    assert gapp.Config._fields_[-1] == ("volumetric_decals", C.c_int32), "the new member is the last one"
    assert capi.MAX_DECALS_BINDLESS == 4096 and "#define GR_MAX_DECALS_BINDLESS 4096" in HEADER


def test_the_header_asserts_the_new_structures():
    for line in ("GR_ASSERT_SIZE(gr_decal_texture, 24);", "GR_ASSERT_SIZE(gr_decal_apply_args, 328);", "GR_ASSERT_OFFSET(gr_decal_apply_args, cluster, 112);",
                 "GR_ASSERT_OFFSET(gr_decal_apply_args, textures, 312);", "GR_ASSERT_OFFSET(gr_decal_apply_args, num_textures, 320);"):
        assert line in HEADER, line
    core = open(os.path.join(ROOT, "granite_amd", "csrc", "decal_core.hpp")).read()
    assert "static_assert(sizeof(Texture) == 24" in core


@pytest.mark.parametrize("c_name, ct", [("gr_decal_texture", capi.DecalTexture), ("gr_decal_apply_args", capi.DecalApplyArgs)])
def test_the_structures_are_the_same_in_c_and_in_ctypes(tmp_path, c_name, ct):
    fields = [name for name, _ in ct._fields_]
    assert c_layout(tmp_path, c_name, fields) == [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields]


def test_the_application_structures_are_the_same_in_c_and_in_ctypes(tmp_path):
    from granite_amd import synth
    got = c_layout(tmp_path, "gra_config", ["volumetric_decals"], "granite_app.h") + c_layout(tmp_path, "gra_decal_desc", ["texture"], "granite_app.h")
    assert got == [C.sizeof(gapp.Config), gapp.Config.volumetric_decals.offset, synth.DECAL_DESC_DTYPE.itemsize, synth.DECAL_DESC_DTYPE.fields["texture"][1]]


def test_refusals_name_the_argument_and_launch_nothing():
    got, _ = run_worker("abi")
    assert got["binning:valid"] == [0, "", 1] and got["apply:valid"] == [0, "", 1]
    for case in ("binning:zero_decals", "binning:zero_decals_null_pointers", "apply:zero_decals", "apply:zero_decals_null_tables"):
        assert got[case] == [0, "", 0], case
    refusals = {case: row for case, row in got.items() if "valid" not in case and "zero_decals" not in case}
    assert len(refusals) == 22
    for case, (code, message, launches) in refusals.items():
        entry, argument = case.split(":")
        assert code == INVALID and launches == 0, (case, code, launches)
        assert message.startswith("gr_cluster_binning_decal: " if entry == "binning" else "gr_decal_apply: "), (case, message)
        word = argument.split(" ")[0].split(".")[-1]
        assert re.search(rf"(?<![A-Za-z0-9_]){re.escape(word)}(?![A-Za-z0-9_])", message.split(": ", 1)[1]), (case, message)
