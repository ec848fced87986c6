"""CPU: the LOD update's arithmetic of granite_amd/csrc/ocean_core.hpp built for the host (tests/cpp/ocean_lod_core_host.cpp, a stand-alone
program, -ffp-contract=off) and held to the reference's shaders executed on the CPU (tests/golden/ocean_lod_shader_v1.npz): the LOD image
byte for byte outside the near-tie mask and within one fp16 code inside it, the counters exactly, the patches as sorted sets per bucket.
The program is built plainly and with -fsanitize=address,undefined and run directly (its own main; nothing is preloaded).  The same cases
run on the device in tests/test_gpu_ocean_lod.py."""
import os
import subprocess

import numpy as np
import pytest

from ocean_lod_cases import CASES, GOLDEN, SMALL, assert_cull, assert_lods, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "ocean_lod_core_host.cpp")


def build(tmp, name, flags):
    exe = tmp / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", *flags, "-o", str(exe), SOURCE])
    return str(exe)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("ocean_lod_core"), "ocean_lod_core_host", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("ocean_lod_core_san"), "ocean_lod_core_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, tmp_path, name):
    gc, _, _, wrap = spec(name)
    case = tmp_path / "case.bin"
    case.write_bytes(np.array([gc, wrap], np.int32).tobytes() + GOLDEN[name + "/update_push"].tobytes() + GOLDEN[name + "/cull_push"].tobytes() +
                     GOLDEN[name + "/frustum"].tobytes() + GOLDEN["init/counts16"].tobytes() + GOLDEN[name + "/lods"].tobytes())
    raw = subprocess.run([exe, str(case)], capture_output=True, check=True).stdout
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
