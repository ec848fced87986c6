"""CPU: the host-only part of the ocean's LOD update (granite_amd/csrc/host/ocean_lod.cpp) through the stand-alone
tests/cpp/ocean_lod_host.cpp, built plainly and once with -fsanitize=address,undefined (host code with its own main; nothing is preloaded):
the push blocks set_camera leads to equal tests/ocean_lod_ref.pass_pushes -- and with it the golden's, which were derived the same way --
bit for bit, OceanDrawInfo holds the reference's values, the meshes equal the numpy restatement byte for byte, and what must be refused is."""
import os

import numpy as np
import pytest

import ocean_lod_ref as olr
from host_program import ROOT, program_fixtures, run_program
from ocean_lod_cases import CASES, GOLDEN, spec

HOST = os.path.join(ROOT, "granite_amd", "csrc", "host")
plain, sanitized = program_fixtures(["ocean_lod_host.cpp", os.path.join(HOST, "ocean_lod.cpp"), os.path.join(HOST, "ocean_distribution.cpp")],
                                    extra=["-D__HIP_PLATFORM_AMD__"])


def state(exe, fft, gc, gr, size, bias, heightmap, fixed, center, camera, planes=None):
    args = ["state", str(fft), str(gc), str(gr), repr(float(size)), repr(float(bias)), str(int(heightmap)), str(int(fixed)),
            *[repr(float(np.float32(v))) for v in center], *[repr(float(np.float32(v))) for v in camera]]
    if planes is not None:
        args += [repr(float(v)) for v in np.asarray(planes, np.float32).reshape(24)]
    raw = run_program(exe, *args)
    out, at = {}, 0

    def take(count, dtype):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    out["update"], out["cull"], out["frustum"], out["wrap"] = take(16, np.uint32), take(24, np.uint32), take(24, np.float32), int(take(1, np.uint32)[0])
    out["counts"], out["data"] = take(16, np.uint32), take(16, np.float32)
    out["lods"], out["lod_stride"], out["border_count"], out["index_type"] = (int(v) for v in take(4, np.uint32))
    out["meshes"] = []
    for _ in range(out["lods"]):
        nv, ni = (int(v) for v in take(2, np.uint32))
        out["meshes"].append((take(nv * 8, np.uint8).reshape(nv, 8), take(ni, np.uint16)))
    nv, ni = (int(v) for v in take(2, np.uint32))
    out["border"] = (take(nv * 3, np.float32).reshape(nv, 3), take(ni, np.uint16))
    assert at == len(raw)
    return out


def check_case(exe, name):
    gc, gr, fixed, wrap = spec(name)
    cfg = GOLDEN[name + "/config"]
    s = state(exe, 128, gc, gr, cfg[0], cfg[2], 1, fixed, cfg[6:9], cfg[3:6], GOLDEN[name + "/frustum"])
    assert np.array_equal(s["update"], GOLDEN[name + "/update_push"]), name
    assert np.array_equal(s["cull"], GOLDEN[name + "/cull_push"]), name
    assert np.array_equal(s["frustum"].view(np.uint32), GOLDEN[name + "/frustum"].reshape(24).view(np.uint32)) and s["wrap"] == wrap
    pushes = olr.pass_pushes(gc, gr, cfg[0:2], cfg[2], cfg[3:6], bool(fixed), cfg[6:9])
    want = olr.draw_data(128, gc, gr, cfg[0:2], 7.3, pushes["world_offset"], pushes["coord_offset"])
    assert np.array_equal(s["data"].view(np.uint32), want.view(np.uint32)), name
    meshes = olr.lod_meshes(gr)
    assert s["lods"] == len(meshes) == olr.lod_count(gr) and s["lod_stride"] == gc * gc * 32 and s["index_type"] == 0
    assert s["counts"].tolist() == [len(i) for _, i in meshes] + [0] * (16 - len(meshes))
    for (v, i), (rv, ri) in zip(s["meshes"], meshes):
        assert np.array_equal(v, rv) and np.array_equal(i, ri)
    positions, indices = olr.border_mesh(gc, gr, True, bool(fixed))
    assert s["border_count"] == len(indices) == len(s["border"][1])
    assert np.array_equal(s["border"][0].view(np.uint32), positions.view(np.uint32)) and np.array_equal(s["border"][1], indices)
    assert (s["border_count"] == 0) == bool(fixed)


@pytest.mark.parametrize("name", [c for c in CASES if "_all_" in c or "_perspective_" in c])
def test_pushes_draw_info_and_meshes(plain, name):
    check_case(plain, name)


def test_before_a_camera_everything_is_in_view(plain):
    s = state(plain, 128, 16, 32, 256.0, -3.5, 1, 0, (0, 0, 0), (0, 0, 0))
    assert s["frustum"].reshape(6, 4).tolist() == [[0.0, 0.0, 0.0, 1.0]] * 6
    assert s["update"][4:6].view(np.int32).tolist() == [-8, -8] and s["update"][0:3].view(np.float32).tolist() == [0.0, 0.0, 0.0]


def test_without_a_heightmap_the_plane_grid_and_border_are_built(plain):
    # derive_ocean_parameters recomposes 64 x 128 to 8 x 1024
    s = state(plain, 128, 64, 128, 1024.0, -3.5, 0, 0, (0, 0, 0), (0, 0, 0))
    positions, indices = olr.border_mesh(8, 1024, heightmap=False)
    assert s["lods"] == 0 and s["meshes"] == []
    assert np.array_equal(s["border"][0], positions) and np.array_equal(s["border"][1], indices) and s["border_count"] == len(indices)
    assert len(positions) == 17 * 17 + 4 * 17 * 2 + 16 + 4 * 19 * 2


def test_refusals(plain):
    run_program(plain, "refusals")


def test_under_address_and_undefined_behaviour_sanitizers(sanitized):
    run_program(sanitized, "refusals")
    for name in ("lod_g16_negative_perspective_moving", "lod_g4_origin_perspective_fixed", "lod_g64_default_origin_all_moving"):
        check_case(sanitized, name)
    state(sanitized, 128, 64, 128, 1024.0, -3.5, 0, 0, (0, 0, 0), (0, 0, 0))
