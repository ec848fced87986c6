"""CPU: granite_amd/csrc/texture_encode_core.hpp built for the host (tests/cpp/texture_encode_core_host.cpp, a stand-alone program,
-ffp-contract=off, walking channel blocks in groups of lanes and mip texels as the kernels of texture_encode.hip do) and held to the
reference's own compressor and mip filter (tests/golden/texture_encode_v1.npz), byte for byte.  The program is built plainly and with
-fsanitize=address,undefined and run directly (its own main; nothing is preloaded).  The same cases run on the device in
tests/test_gpu_texture_encode.py."""
import numpy as np
import pytest

import texture_encode_cases as tc
from host_program import program_fixtures, run_program

GOLDEN = tc.load_golden()
ENCODE = [(name, fmt) for name, case in tc.ENCODE_CASES.items() for fmt in case[3]]
plain, sanitized = program_fixtures("texture_encode_core_host.cpp", exact=True)


def run(exe, tmp_path, words, data):
    case = np.asarray(words, np.uint32).tobytes() + np.ascontiguousarray(data).tobytes()
    return np.frombuffer(run_program(exe, input_bytes=case, tmp_path=tmp_path), np.uint8)


def check_encode(exe, tmp_path, name, fmt, pad=0):
    image = GOLDEN[f"enc/{name}/input"]
    h, w, c = image.shape
    rows = np.full((h, w * c + pad), 0x5a, np.uint8)
    rows[:, :w * c] = image.reshape(h, w * c)
    got = run(exe, tmp_path, [0, w, h, c, 2 if fmt == tc.BC5 else 1, w * c + pad], rows)
    assert np.array_equal(got, GOLDEN[f"enc/{name}/{fmt}/blocks"].reshape(-1)), f"{name}: host build against the reference"


def check_mips(exe, tmp_path, name):
    fmt, w, h, layers, levels = tc.MIP_CASES[name]
    payload = GOLDEN[f"mip/{name}/payload"]
    for level in range(1, levels):
        above, below = (tc.chain_level(payload, fmt, w, h, layers, levels, l) for l in (level - 1, level))
        for layer in range(layers):
            got = run(exe, tmp_path, [1, above.shape[2], above.shape[1], tc.CHANNELS[fmt]], above[layer])
            assert np.array_equal(got, below[layer].reshape(-1)), f"{name} level {level} layer {layer}: host build against the reference"


@pytest.mark.parametrize("name,fmt", ENCODE)
def test_encode_against_the_golden(plain, tmp_path, name, fmt):
    check_encode(plain, tmp_path, name, fmt)


def test_encode_from_a_padded_pitch(plain, tmp_path):
    check_encode(plain, tmp_path, "edge_rg8", tc.BC5, pad=5)


@pytest.mark.parametrize("name", tc.MIP_CASES)
def test_mips_against_the_golden(plain, tmp_path, name):
    check_mips(plain, tmp_path, name)


@pytest.mark.parametrize("name,fmt", ENCODE)
def test_encode_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, name, fmt):
    check_encode(sanitized, tmp_path, name, fmt)


@pytest.mark.parametrize("name", tc.MIP_CASES)
def test_mips_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, name):
    check_mips(sanitized, tmp_path, name)
