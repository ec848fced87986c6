"""gr_meshlet_cull (csrc/meshlet_cull.hip) on a synthetic scene of 32 768 tasks of 32 chunks -- 1 048 576 chunks -- placed so that
roughly half of them are culled, in each phase: 0 (frustum and cone), 1 (the same behind random occluder words), 2 (with the depth
hierarchy of a 1920 x 1080 synthetic depth: 960 x 544, 9 levels), perspective, not skinned.

Per phase: the kernel alone by the library's own event bracket (gr_timing_*, span "meshlet_cull"), 200 launches a round, three rounds,
every one printed; the wall clock over the same launches, which includes restoring the count word and the occluder words from device
copies before every launch (a launch changes both) and the brackets' own cost.  The survivor count of the last launch is compared with
tests/meshlet_cull_ref.py on the same scene.

Bytes a launch has to move, from the reference's counts: per task 20 (task) + 32 (AABB), 4 more for the occluder word in phases 1 and 2;
per processed task 48 (transform); per candidate chunk 32 (bound); per survivor 12 read (draw) and 20 written; in phase 2 4 written per
task (occluder word).  The depth hierarchy's texels (up to four a test) are not counted: 2.9 MB in all, cache-resident.

    timeout -k 10 600 python tools/meshlet_cull_time.py > profiles/meshlet_cull_time.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meshlet_cull_cases as mc  # noqa: E402
import meshlet_cull_ref as ref  # noqa: E402
from granite_amd import capi, meshlet  # noqa: E402

TASKS, CHUNKS = 32768, 32
SCREEN = (1920, 1080)
LAUNCHES, ROUNDS = 200, 3


def build_scene(seed=20261019):
    mc.SCREENS["time"] = SCREEN
    cam = mc.Camera(False, "time")
    rng = np.random.default_rng(seed)
    sb = cam.scale_bias().astype(np.float64)
    # task clusters in the shader's view space: depth log-uniform, pixels over and around the screen
    z = np.exp(rng.uniform(np.log(2.0), np.log(120.0), TASKS))
    px, py = rng.uniform(-0.12, 1.12, TASKS) * SCREEN[0], rng.uniform(-0.12, 1.12, TASKS) * SCREEN[1]
    centre = np.stack([(px - sb[2]) / sb[0] * z, (py - sb[3]) / sb[1] * z, z], 1)
    view = centre[:, None, :] + rng.normal(scale=0.4, size=(TASKS, CHUNKS, 3))
    world = cam.position[None, None, :] + (view * np.array([1.0, -1.0, -1.0])) @ cam.rotation
    radius = rng.uniform(0.05, 0.3, (TASKS, CHUNKS))
    # one node per task: a non-uniform scale and a translation
    scale, shift = rng.uniform(0.5, 2.0, (TASKS, 3)), rng.uniform(-3.0, 3.0, (TASKS, 3))
    transforms = np.zeros((TASKS, 3, 4))
    for i in range(3):
        transforms[:, i, i] = scale[:, i]
    transforms[:, :, 3] = shift
    local = (world - shift[:, None, :]) / scale[:, None, :]
    to_camera = cam.position[None, None, :] - world
    to_camera /= np.linalg.norm(to_camera, axis=2, keepdims=True)
    kind = rng.integers(0, 4, (TASKS, CHUNKS))  # none, facing, facing, away
    axis = np.where((kind == 3)[..., None], -to_camera, to_camera) + rng.normal(scale=0.2, size=(TASKS, CHUNKS, 3))
    axis = axis / scale[:, None, :]
    axis /= np.linalg.norm(axis, axis=2, keepdims=True)
    cutoff = np.where(kind == 0, 1.0, rng.uniform(0.1, 0.7, (TASKS, CHUNKS)))
    bounds = np.concatenate([local, (radius / scale.max(axis=1)[:, None])[..., None], axis, cutoff[..., None]], 2).astype(np.float32).reshape(-1, 8)
    lo, hi = (world - radius[..., None]).min(axis=1), (world + radius[..., None]).max(axis=1)
    aabbs = np.concatenate([lo, np.zeros((TASKS, 1)), hi, np.zeros((TASKS, 1))], 1).astype(np.float32)
    index = np.arange(TASKS, dtype=np.uint32)
    tasks = np.stack([index, index, index, index * CHUNKS + (CHUNKS - 1), np.zeros(TASKS, np.uint32)], 1).astype(np.uint32)
    chunk = np.arange(TASKS * CHUNKS, dtype=np.uint32)
    draws = np.stack([np.full_like(chunk, 768), chunk * 768, chunk * 256], 1).astype(np.uint32)
    occluders = (rng.integers(0, 1 << 32, TASKS, dtype=np.uint64) | rng.integers(0, 1 << 32, TASKS, dtype=np.uint64)).astype(np.uint32)
    occluders[::7] = 0
    output = np.full(mc.COUNT_WORDS + 5 * TASKS * CHUNKS, ref.POISON_WORD, np.uint32)
    output[:mc.COUNT_WORDS] = 0
    depth = np.full((SCREEN[1], SCREEN[0]), 150.0, np.float32)
    depth[:, :SCREEN[0] // 2] = 25.0  # a wall over the left half
    chain = mc.max_chain(depth)
    return {"tasks": tasks, "aabbs": aabbs, "transforms": transforms.astype(np.float32).reshape(-1, 12), "bounds": bounds, "draws": draws, "occluders": occluders,
            "output": output, "frustum": cam.frustum(chain), "camera": cam.position.astype(np.float32), "chain_key": "time", "chain": chain[0],
            "chain_width": chain[1], "chain_height": chain[2], "chain_levels": chain[3], "dispatches": np.array([[0, TASKS, 0, mc.COUNT_WORDS]], np.uint32)}


def main():
    scene = build_scene()
    gr = capi.Context(0)
    device = meshlet.CullScene(gr, scene["tasks"], scene["aabbs"], scene["transforms"], scene["bounds"], scene["draws"], scene["occluders"], scene["output"],
                               scene["chain"], scene["chain_width"], scene["chain_height"], scene["chain_levels"])
    pristine_occluders = capi.DeviceBuffer(gr, scene["occluders"].nbytes).upload(scene["occluders"])
    zero = capi.DeviceBuffer(gr, 16)
    print(f"{TASKS} tasks of {CHUNKS} chunks = {TASKS * CHUNKS} chunks; depth hierarchy {scene['chain_width']} x {scene['chain_height']}, {scene['chain_levels']} levels;"
          f" one wave64 a group, {TASKS // 64} groups")
    expected = {}
    for phase in (0, 1, 2):
        _, _, info = mc.run_reference(scene, phase, 0)
        expected[phase] = info
    args = {phase: device.args(scene["frustum"], scene["camera"], phase, 0) for phase in (0, 1, 2)}

    def launch(phase):
        gr.check(gr.lib.gr_copy(gr.handle, None, device.buffers["output"].ptr, zero.ptr, 16))
        gr.check(gr.lib.gr_copy(gr.handle, None, device.buffers["occluders"].ptr, pristine_occluders.ptr, scene["occluders"].nbytes))
        gr.meshlet_cull(args[phase], 0, TASKS, 0, mc.COUNT_WORDS)

    for phase in (0, 1, 2):
        for _ in range(20):
            launch(phase)
    gr.sync()
    gr.timing_enable(True)
    for round_ in range(ROUNDS):
        for phase in (0, 1, 2):
            gr.sync()
            gr.timing_reset()
            t0 = time.perf_counter()
            for _ in range(LAUNCHES):
                launch(phase)
            gr.sync()
            wall = (time.perf_counter() - t0) / LAUNCHES
            count, ms = gr.timing_query().get("meshlet_cull", (0, 0.0))[:2]
            info = expected[phase]
            survivors = int(device.buffers["output"].download(np.uint32, 1)[0])
            read = TASKS * (52 + (4 if phase else 0)) + info["tasks_processed"] * 48 + info["chunk_candidates"] * 32 + info["draws"] * 12
            written = info["draws"] * 20 + (TASKS * 4 if phase == 2 else 0)
            us = ms * 1e3 / max(count, 1)
            print(f"phase {phase} round {round_}: {us:8.2f} us a launch by device events ({count} launches), {wall * 1e6:8.2f} us by the wall clock with the resets;"
                  f"  {survivors} of {TASKS * CHUNKS} chunks drawn (restatement {info['draws']});  reads {read / 1e6:6.2f} MB, writes {written / 1e6:6.2f} MB,"
                  f" {(read + written) / us / 1e3:7.1f} GB/s")
            assert survivors == info["draws"], (phase, survivors, info["draws"])
    gr.timing_enable(False)
    for phase in (0, 1, 2):
        info = expected[phase]
        print(f"phase {phase}: tasks processed {info['tasks_processed']}, candidate chunks {info['chunk_candidates']}, cone rejects {info['chunk_cone_reject']},"
              f" plane rejects {sum(info[f'chunk_plane_{i}_reject'] for i in range(6))}, HiZ rejects {info['chunk_hiz_reject']} (chunks) {info['aabb_hiz_reject']} (tasks)")
    gr.close()


if __name__ == "__main__":
    main()
