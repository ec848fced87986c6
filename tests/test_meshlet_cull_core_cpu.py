"""CPU: the culling decisions of granite_amd/csrc/meshlet_cull.hpp built for the host (tests/cpp/meshlet_cull_core_host.cpp, a stand-alone
program, -ffp-contract=off, walking tasks as k_meshlet_cull does) and held to the reference's meshlet_cull.comp executed on the CPU
(tests/golden/meshlet_cull_shader_v1.npz): every case in every specialisation set, count words exact, records exact as sets sorted by
(task_index, first_index), each task's records contiguous and in lane order, occluder words exact, every other dword untouched.
The program is built plainly and with -fsanitize=address,undefined and run directly (its own main; nothing is preloaded).  The same
cases run on the device in tests/test_gpu_meshlet_cull.py."""
import numpy as np
import pytest

import meshlet_cull_cases as mc
import meshlet_cull_ref as ref
from host_program import program_fixtures, run_program

GOLDEN = mc.load_golden()
plain, sanitized = program_fixtures("meshlet_cull_core_host.cpp", exact=True)


def case_bytes(scene, phase, flags):
    header = np.array([phase, flags, len(scene["tasks"]), len(scene["aabbs"]), len(scene["transforms"]), len(scene["bounds"]), len(scene["occluders"]),
                       len(scene["output"]), len(scene["chain"]), scene["chain_width"], scene["chain_height"], scene["chain_levels"], len(scene["dispatches"])], np.uint32)
    parts = [header, scene["camera"], scene["frustum"], scene["dispatches"], scene["tasks"], scene["aabbs"], scene["transforms"], scene["bounds"], scene["draws"],
             scene["occluders"], scene["output"], scene["chain"]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def run(exe, tmp_path, scene, phase, flags):
    raw = run_program(exe, input_bytes=case_bytes(scene, phase, flags), tmp_path=tmp_path)
    words = np.frombuffer(raw, np.uint32)
    assert len(words) == len(scene["output"]) + len(scene["occluders"])
    return words[:len(scene["output"])], words[len(scene["output"]):]


def check(exe, tmp_path, name, sets):
    for phase, flags in sets:
        scene = mc.golden_scene(GOLDEN, name, bool(flags & ref.ORTHO))
        output, occluders = run(exe, tmp_path, scene, phase, flags)
        want_output, want_occluders = mc.golden_result(GOLDEN, name, phase, flags)
        mc.assert_same(scene, output, occluders, want_output, want_occluders, f"{name} {mc.set_name(phase, flags)}: host build against the executed shader")


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_against_the_golden(plain, tmp_path, name):
    check(plain, tmp_path, name, mc.sets())


@pytest.mark.parametrize("name", ["tasks_33", "two_lists", "occlusion", "lod_clamp", "span_sides", "phase_words"])
def test_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, name):
    check(sanitized, tmp_path, name, mc.sets())


def test_indices_outside_their_buffers_under_sanitizers(sanitized, tmp_path):
    """Device data is not trusted: tasks naming an AABB, a transform, chunks or an occluder word past their arrays, a dispatch reaching past
    the task array, an output too small for the records, and floats no int can hold on the way to the depth hierarchy.  The program must
    neither read nor write outside an array (ASan, UBSan) and agree with the restatement, which treats such elements as not visible."""
    for phase, flags in mc.sets():
        scene = mc.hostile_scene(bool(flags & ref.ORTHO))
        output, occluders = run(sanitized, tmp_path, scene, phase, flags)
        want_output, want_occluders, _ = mc.run_reference(scene, phase, flags)
        mc.assert_same(scene, output, occluders, want_output, want_occluders, f"hostile {mc.set_name(phase, flags)}")
