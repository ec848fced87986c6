"""CPU: the LOD update's arithmetic of granite_amd/csrc/ocean_core.hpp built for the host (tests/cpp/ocean_lod_core_host.cpp, a stand-alone
program, -ffp-contract=off) and held to the reference's shaders executed on the CPU (tests/golden/ocean_lod_shader_v1.npz): the LOD image
byte for byte outside the near-tie mask and within one fp16 code inside it, the counters exactly, the patches as sorted sets per bucket.
The program is built plainly and with -fsanitize=address,undefined and run directly (its own main; nothing is preloaded).  The same cases
run on the device in tests/test_gpu_ocean_lod.py."""
import numpy as np
import pytest

from host_program import program_fixtures, run_program
from ocean_lod_cases import CASES, GOLDEN, SMALL, assert_cull, assert_lods, spec

plain, sanitized = program_fixtures("ocean_lod_core_host.cpp", exact=True, extra=["-D__HIP_PLATFORM_AMD__"])


def run(exe, tmp_path, name):
    gc, _, _, wrap = spec(name)
    case = (np.array([gc, wrap], np.int32).tobytes() + GOLDEN[name + "/update_push"].tobytes() + GOLDEN[name + "/cull_push"].tobytes() +
            GOLDEN[name + "/frustum"].tobytes() + GOLDEN["init/counts16"].tobytes() + GOLDEN[name + "/lods"].tobytes())
    raw = run_program(exe, input_bytes=case, tmp_path=tmp_path)
    sizes = [gc * gc * 2, 256, 256, gc * gc * 8 * 32]
    assert len(raw) == sum(sizes)
    at = np.cumsum([0] + sizes)
    lods, init, draws, patches = (raw[a:b] for a, b in zip(at[:-1], at[1:]))
    return np.frombuffer(lods, np.uint16), np.frombuffer(init, np.uint32), np.frombuffer(draws, np.uint32), np.frombuffer(patches, np.uint32)


def check(exe, tmp_path, name):
    lods, init, draws, patches = run(exe, tmp_path, name)
    differing = assert_lods(name, lods, "host build")
    assert np.array_equal(init.reshape(8, 8), GOLDEN["init/draws"])
    assert_cull(name, draws, patches, "host build")
    return differing


@pytest.mark.parametrize("name", CASES)
def test_against_the_golden(plain, tmp_path, name):
    print(f"{name}: {check(plain, tmp_path, name)} texels differ from the golden")


@pytest.mark.parametrize("name", [c for c in SMALL if "perspective" in c or "negative_all" in c])
def test_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, name):
    check(sanitized, tmp_path, name)
