"""CPU: the culling pass's host arithmetic as the host library computes it (granite_amd/csrc/host/mesh/meshlet_cull.cpp), built into a
stand-alone program with no device and with -fsanitize=address,undefined (tests/cpp/meshlet_cull_host.cpp).

fill_meshlet_culling_ubo against Renderer::bind_meshlet_culling_ubo's arithmetic (renderer/renderer.cpp:540-572) restated in fp32, for a
perspective and an orthographic projection, with and without a depth hierarchy, and against values worked by hand; build_task_infos
against the loop of update_task_buffer for ranges of 1, 32, 33 and 96 chunks, and refused for a misaligned offset; place_mesh_chunks on
MESHLET4 files; and the phase, flags and push block build_mdi_culling_pass gives each call."""
import os
import subprocess

import numpy as np
import pytest

import meshlet_cases as files
import meshlet_cull_cases as mc
import meshlet_cull_ref as ref
import meshlet_ref as mr
from host_program import ROOT, program_fixtures, run_program

HOST = os.path.join(ROOT, "granite_amd", "csrc", "host")
program = program_fixtures(["meshlet_cull_host.cpp", os.path.join(HOST, "mesh", "meshlet_cull.cpp"), os.path.join(HOST, "mesh", "meshlet.cpp"),
                            os.path.join(HOST, "math.cpp")], extra=["-D__HIP_PLATFORM_AMD__"]).sanitized


def camera_words(cam, viewport, cw, hiz, extra=()):
    """projection and view column-major, the planes, the viewport, then the dwords the program reads"""
    f = np.concatenate([cam.projection.T.astype(np.float32).ravel(), cam.view.T.astype(np.float32).ravel(), cam.planes.ravel(), np.array(viewport, np.float32)])
    return np.concatenate([f.view(np.uint32), np.array([int(cw), int(hiz is not None), *(hiz or (0, 0, 0, 0)), *extra], np.uint32)])


def expected_ubo(cam, viewport, cw, hiz):
    F = np.float32
    x, y, w, h = (F(v) for v in viewport)
    p = cam.projection.T.astype(np.float32)  # [column][row]
    sb = [F(0.5) * w, F(0.5) * h, F(0.5) * w, F(0.5) * h]
    sb[2] = sb[2] + sb[0] * p[3][0]
    sb[3] = sb[3] + sb[1] * p[3][1]
    sb[0] = sb[0] * p[0][0]
    sb[1] = sb[1] * -p[1][1]
    res, lo, hi = (0, 0), 0, 0
    if hiz:
        res, lo, hi = (hiz[0] << hiz[3], hiz[1] << hiz[3]), hiz[3], hiz[2] - 1 + hiz[3]
    return ref.pack_frustum(cam.planes, cam.view.T.astype(np.float32), sb, [x + F(0.5) * w - F(0.5), y + F(0.5) * h - F(0.5), F(0.5) * w, F(0.5) * h], res,
                            -1.0 if cw else 1.0, lo, hi)


@pytest.mark.parametrize("ortho", [False, True])
def test_fill_meshlet_culling_ubo(program, tmp_path, ortho):
    cam = mc.Camera(ortho, "a")
    for viewport, cw, hiz in (((0, 0, 100, 60), False, (64, 32, 5, 1)), ((3, 7, 200, 40), True, (128, 32, 6, 1)), ((0, 0, 1920, 1080), False, None),
                              ((0, 0, 101, 61), False, (64, 32, 5, 0))):
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(camera_words(cam, viewport, cw, hiz).tobytes())
        run_program(program, "ubo", str(src), str(dst), timeout=60)
        got = np.fromfile(dst, np.uint32)
        assert got.shape == (56,)
        assert np.array_equal(got, expected_ubo(cam, viewport, cw, hiz)), (viewport, cw, hiz)
    # the same block the golden scenes carry
    src.write_bytes(camera_words(cam, (0, 0, 100, 60), False, (64, 32, 5, 1)).tobytes())
    run_program(program, "ubo", str(src), str(dst), timeout=60)
    assert np.array_equal(np.fromfile(dst, np.uint32), cam.frustum(mc.chains()["a"]))


def test_fill_meshlet_culling_ubo_by_hand(program, tmp_path):
    """1920 x 1080 at (10, 20), projection[0].x = 1.5, projection[1].y = -2, projection[3].xy = (0.25, -0.5): exact in fp32"""
    cam = mc.Camera(False, "a")
    cam.projection = np.zeros((4, 4))
    cam.projection[0, 0], cam.projection[1, 1], cam.projection[0, 3], cam.projection[1, 3], cam.projection[3, 2] = 1.5, -2.0, 0.25, -0.5, -1.0
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(camera_words(cam, (10, 20, 1920, 1080), True, (960, 576, 9, 1)).tobytes())
    run_program(program, "ubo", str(src), str(dst), timeout=60)
    got = ref.frustum_fields(np.fromfile(dst, np.uint32))
    assert list(got["viewport"]) == [969.5, 559.5, 960.0, 540.0]
    assert list(got["scale_bias"]) == [1440.0, 1080.0, 1200.0, 270.0]
    assert list(got["hiz_resolution"]) == [1920, 1152] and got["hiz_min_lod"] == 1 and got["hiz_max_lod"] == 9 and got["winding"] == -1.0


@pytest.mark.parametrize("count", [0, 1, 32, 33, 96])
def test_build_task_infos(program, tmp_path, count):
    dst = tmp_path / "tasks.bin"
    run_program(program, "tasks", "7", "9", "0x123456", "40", "64", str(count), str(dst), timeout=60)
    got = np.fromfile(dst, np.uint32).reshape(-1, 5)
    want = [[7, 40 + t, 9, 64 + j + (min(count - j, 32) - 1), 0x123456] for t, j in enumerate(range(0, count, 32))]
    assert got.tolist() == want
    assert len(got) == (count + 31) // 32


def test_build_task_infos_refuses_a_misaligned_offset(program, tmp_path):
    r = subprocess.run([program, "tasks", "0", "0", "0", "0", "48", "5", str(tmp_path / "t.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5 and "offset 48 is not a multiple of 32" in r.stderr


def test_place_mesh_chunks(program, tmp_path):
    """three files of 1, 9 and 40 meshlets (1, 2 and 5 chunks): each at a 32-aligned offset, bounds_256 and the MDI records in place"""
    paths, metas = [], []
    for k, count in enumerate((1, 9, 40)):
        counts = [(i % 5 + 1, i % 7 + 3) for i in range(count)]
        path = tmp_path / f"mesh{k}.msh4"
        path.write_bytes(files.random_file(70 + k, 1, counts, padding=bool(k & 1)))
        paths.append(str(path))
        metas.append((np.array(counts, np.int64), mr.parse(path.read_bytes())))
    dst = tmp_path / "place.bin"
    run_program(program, "place", str(dst), "11", "5", *paths, timeout=60)
    raw = np.fromfile(dst, np.uint32)
    ranges = raw[:6].reshape(3, 2)
    assert ranges.tolist() == [[0, 1], [32, 2], [64, 5]]
    total = 69
    bounds = raw[6:6 + total * 8].view(np.float32).reshape(total, 8)
    draws = raw[6 + total * 8:].reshape(total, 3)
    prim, vert = 11, 5
    for (offset, count), (counts, mesh) in zip(ranges, metas):
        data = mesh.get("chunk_bounds")
        assert np.array_equal(bounds[offset:offset + count], np.asarray(data, np.float32).reshape(-1, 8))
        assert np.array_equal(draws[offset:offset + count], mr.indirect(counts, mr.MDI, prim, vert).reshape(-1, 3))
        prim, vert = prim + int(counts[:, 0].sum()), vert + int(counts[:, 1].sum())
    used = np.zeros(total, bool)
    for offset, count in ranges:
        used[offset:offset + count] = True
    assert not bounds[~used].any() and not draws[~used].any(), "the padding records are zero"


@pytest.mark.parametrize("ortho", [False, True])
def test_build_mdi_culling_pass_arguments(program, tmp_path, ortho):
    """CullingPhase::{OneShot, First, MotionVector, Second} -> 0, 1, 1, 2; ORTHO from projection[3].w == 1; byte offsets to dwords"""
    cam = mc.Camera(ortho, "b")
    for phase_enum, phase in ((0, 0), (1, 1), (2, 1), (3, 2)):
        for force, skinned in ((0, 0), (1, 1), (0, 1)):
            src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
            src.write_bytes(camera_words(cam, (0, 0, 0, 0), False, (128, 32, 6, 1), extra=(phase_enum, force, 200, 40, 8, 4096, 77, 5, 50, skinned)).tobytes())
            run_program(program, "describe", str(src), str(dst), timeout=60)
            got = np.fromfile(dst, np.uint32)
            flags = (ref.ORTHO if ortho else 0) | (ref.SKINNED if skinned else 0) | (ref.FORCE_VISIBLE if force else 0)
            assert got[:6].tolist() == [phase, flags, 5, 50, 2, 1024]
            assert np.array_equal(got[6:], expected_ubo(cam, (0, 0, 200, 40), False, (128, 32, 6, 1)))
