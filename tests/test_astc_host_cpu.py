"""CPU: granite_amd/csrc/astc_decode.hpp -- the ASTC decode the device kernel calls -- built for the host (tests/cpp/astc_decode_host.cpp,
which walks blocks and texels in the kernel's order through the same block half and texel half) against the reference's decode shader
executed on the CPU (tests/golden/astc_decode_shader_v1.npz), byte for byte; its compile-time tables against the recorded contents of the
shader's buffers, entry for entry; and the same program built with -fsanitize=address,undefined -fno-sanitize-recover run on the golden
blocks and on 4096 uniformly random 16-byte blocks per footprint class: the decoder is total, any 16 bytes decode without undefined
behaviour and to what tests/astc_ref.py gives."""
import numpy as np

import astc_cases
import astc_ref
from host_program import program_fixtures, run_program

CASES = astc_cases.golden()
plain, sanitized = program_fixtures("astc_decode_host.cpp")


def run(exe, tmp_path, bw, bh, w, h, blocks):
    src, dst = str(tmp_path / "blocks.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(blocks, np.uint8).tofile(src)
    run_program(exe, "decode", bw, bh, w, h, src, dst)
    return np.fromfile(dst, np.uint8).reshape(h, w, 4)


def strip(exe, tmp_path, bw, bh, blocks):
    """Every block of (N, 16) decoded as one row of blocks -> (N, bh, bw, 4)."""
    n = len(blocks)
    return run(exe, tmp_path, bw, bh, n * bw, bh, blocks).reshape(bh, n, bw, 4).transpose(1, 0, 2, 3)


def check_golden(exe, tmp_path):
    for bw, bh in astc_ref.FOOTPRINTS:
        group = [(n, c) for n, c in CASES.items() if astc_ref.format_footprint(c[0]) == (bw, bh)]
        texels = strip(exe, tmp_path, bw, bh, np.concatenate([c[3].reshape(-1, 16) for _, c in group]))  # more than 64 blocks: several waves' worth
        at = 0
        for name, (fmt, w, h, blocks, out) in group:
            count = blocks.shape[0] * blocks.shape[1]
            assert np.array_equal(astc_ref.assemble(texels[at:at + count], bw, bh, w, h), out), name
            at += count
            if "_tail_" in name:  # partial blocks at the right and bottom edge, in the kernel's walk
                assert np.array_equal(run(exe, tmp_path, bw, bh, w, h, blocks), out), name


def test_host_build_equals_the_executed_shader(plain, tmp_path):
    check_golden(plain, tmp_path)


def test_compile_time_tables_equal_the_recorded_ones(plain, tmp_path):
    recorded = astc_cases.golden_tables()
    path = str(tmp_path / "tables.bin")
    run_program(plain, "tables", path)
    raw, at = np.fromfile(path, np.uint8), 0
    for key, dtype, shape in (("endpoint_quantiser", np.uint16, (9, 128, 4)), ("endpoint_unquant", np.uint8, (1192,)), ("weight_quantiser", np.uint8, (16, 4)),
                              ("weight_unquant", np.uint8, (142,)), ("trits_quints", np.uint16, (384,))):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert recorded[key].shape == shape and np.array_equal(raw[at:at + nbytes].view(dtype).reshape(shape), recorded[key]), key
        at += nbytes
    assert at == raw.size
    for bw, bh in astc_cases.FULL:  # the partition index is computed, not looked up: the table it would have been read from
        run_program(plain, "partition", bw, bh, path)
        assert np.array_equal(np.fromfile(path, np.uint8).reshape(32 * bh, 32 * bw), recorded[f"partition_{bw}x{bh}"]), (bw, bh)


def test_sanitized_build_on_golden_and_random_blocks(sanitized, tmp_path):
    check_golden(sanitized, tmp_path)
    rng = np.random.default_rng(4096)
    for bw, bh in astc_cases.FULL:
        blocks = rng.integers(0, 256, (4096, 16), dtype=np.uint8)
        blocks[:256, 0], blocks[:256, 1] = 0xfc, blocks[:256, 1] | 1  # void extents are one in 512 of uniform blocks: force some
        assert np.array_equal(strip(sanitized, tmp_path, bw, bh, blocks), astc_ref.decode_blocks(blocks, bw, bh)), (bw, bh)
