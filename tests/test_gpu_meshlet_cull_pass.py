"""GPU: the culling pass as an integrator drives it.  Seeded MESHLET4 files (tests/meshlet_cases.py) go through create_mesh_view,
place_mesh_chunks, build_task_infos and build_mdi_culling_pass in a C++ program (tests/cpp/meshlet_cull_pass.cpp) linked against the
built libraries, one scene per CullingPhase; the program's tasks, bounds and draws and the device's output and occluder words are held
to tests/meshlet_cull_ref.py.  A second MDICall with indirect_count_max = 0 and offsets no launch would accept must be skipped."""
import numpy as np
import pytest

import meshlet_cases as files
import meshlet_cull_cases as mc
import meshlet_cull_ref as ref
from host_program import PRODUCT, program_fixtures, run_program

pytestmark = pytest.mark.gpu
program = program_fixtures("meshlet_cull_pass.cpp", extra=PRODUCT).plain


def mesh_file(seed, meshlets, cam, rng):
    """a Textured file whose chunk bounds are replaced by spheres around the screen (the container stores them verbatim)"""
    data = bytearray(files.random_file(seed, 1, [(i % 7 + 1, i % 9 + 3) for i in range(meshlets)], padding=bool(seed & 1)))
    chunks = (meshlets + 7) // 8
    at = 24 + meshlets * 32
    bounds = np.zeros((chunks, 8), np.float32)
    for k in range(chunks):
        centre, radius = mc.random_sphere(cam, rng)
        cone = mc.random_cone(cam, rng, centre)
        axis, cutoff = (np.array([0.0, 0.0, 1.0]), 1.0) if cone is None else cone
        bounds[k] = [*centre, radius, *axis, cutoff]
    data[at:at + chunks * 32] = bounds.tobytes()
    return bytes(data), bounds


@pytest.mark.parametrize("phase_enum,phase,force", [(0, 0, 0), (1, 1, 0), (2, 1, 0), (3, 2, 0), (3, 2, 1)], ids=["OneShot", "First", "MotionVector", "Second", "Second-force"])
def test_files_through_the_host_helpers_equal_the_restatement(program, tmp_path, phase_enum, phase, force):
    rng = np.random.default_rng(100 + phase_enum)
    cam = mc.Camera(False, "a")
    chain = mc.chains()["a"]
    meshes = [mesh_file(300 + k, count, cam, rng) for k, count in enumerate((5, 8, 70, 257, 300))]  # 1, 1, 9, 33 and 38 chunks
    instances = [int(rng.integers(0, len(meshes))) for _ in range(40)]
    # instances sit where their file's bounds are: identity rotation, unit scale, a small translation; the AABB holds the moved spheres
    transforms = np.zeros((len(instances), 3, 4), np.float32)
    aabbs = np.zeros((len(instances), 8), np.float32)
    for i, m in enumerate(instances):
        shift = rng.normal(scale=0.5, size=3)
        transforms[i, :, :3] = np.eye(3)
        transforms[i, :, 3] = shift
        b = meshes[m][1]
        aabbs[i, 0:3] = (b[:, 0:3] - b[:, 3:4]).min(axis=0) + shift
        aabbs[i, 4:7] = (b[:, 0:3] + b[:, 3:4]).max(axis=0) + shift
    head = np.array([phase_enum, force, cam.width, cam.height, len(meshes), len(instances), chain[1], chain[2], chain[3], 1], np.uint32)
    floats = np.concatenate([cam.projection.T.astype(np.float32).ravel(), cam.view.T.astype(np.float32).ravel(), cam.planes.ravel(), cam.position.astype(np.float32)])
    per_instance = np.array([[m, 0x1000 + i] for i, m in enumerate(instances)], np.uint32)
    parts = [head, floats, per_instance, aabbs, transforms, chain[0]]
    blob = b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
    for data, _ in meshes:
        blob += np.array([len(data)], np.uint32).tobytes() + data + b"\0" * (-len(data) % 4)
    src, dst = tmp_path / "scene.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    run_program(program, src, dst, timeout=120)
    raw = np.fromfile(dst, np.uint32)
    n_tasks, n_chunks, n_out = (int(v) for v in raw[:3])
    at = 3
    tasks = raw[at:at + 5 * n_tasks].reshape(-1, 5); at += 5 * n_tasks
    bounds = raw[at:at + 8 * n_chunks].view(np.float32).reshape(-1, 8); at += 8 * n_chunks
    draws = raw[at:at + 3 * n_chunks].reshape(-1, 3); at += 3 * n_chunks
    output = raw[at:at + n_out]; at += n_out
    occluders = raw[at:at + n_tasks]
    assert at + n_tasks == len(raw)
    # the host helpers: one task per 32 chunks of each instance, at the file's 32-aligned offset
    chunk_counts = [len(b) for _, b in meshes]
    offsets = np.cumsum([0] + [(c + 31) // 32 * 32 for c in chunk_counts])
    want_tasks = []
    for i, m in enumerate(instances):
        for j in range(0, chunk_counts[m], 32):
            want_tasks.append([i, len(want_tasks), i, offsets[m] + j + min(chunk_counts[m] - j, 32) - 1, 0x1000 + i])
    assert tasks.tolist() == [[int(v) for v in t] for t in want_tasks]
    for m, (_, b) in enumerate(meshes):
        assert np.array_equal(bounds[offsets[m]:offsets[m] + chunk_counts[m]], b)
    start = np.array([0 if i % 5 == 0 else ((i * 2654435761) & 0xFFFFFFFF) ^ 0x5bd1e995 for i in range(n_tasks)], np.uint32)
    blank = np.full(n_out, ref.POISON_WORD, np.uint32)
    blank[:mc.COUNT_WORDS] = 0
    scene = {"tasks": tasks, "aabbs": aabbs, "transforms": transforms.reshape(-1, 12), "bounds": bounds, "draws": draws, "occluders": start, "output": blank,
             "frustum": cam.frustum(chain), "camera": cam.position.astype(np.float32), "chain": chain[0], "chain_width": chain[1], "chain_height": chain[2],
             "chain_levels": chain[3], "dispatches": np.array([[0, n_tasks, 0, mc.COUNT_WORDS]], np.uint32)}
    flags = ref.FORCE_VISIBLE if force else 0
    want_output, want_occluders, info = mc.run_reference(scene, phase, flags)
    assert 0 < info["draws"] < sum((int(t[3]) & 31) + 1 for t in tasks)
    mc.assert_same(scene, output, occluders, want_output, want_occluders, f"pass phase {phase_enum}")
