"""CPU: granite_amd/csrc/meshlet_decode.hpp -- the mesh decode the device kernel calls -- built for the host (tests/cpp/meshlet_decode_host.cpp,
which walks groups, meshlets and lanes as the kernel launches them) against the reference's decode shader executed on the CPU
(tests/golden/meshlet_decode_shader_v1.npz), byte for byte; and the same program built with -fsanitize=address,undefined
-fno-sanitize-recover run on the golden cases and on seeded random headers, malformed ones included: counts above 32, bit widths up to
255, offsets past the end and about to wrap, capacities short of what the counts ask for, the payload allocated at exactly
payload_size_words words.  With the kernel's own clamps the sanitizers stay silent, nothing outside the output arrays changes, and the
outputs are what tests/meshlet_ref.py gives.  This program is the only place malformed device data is exercised."""
import numpy as np

import meshlet_cases as mc
import meshlet_ref as mr
from host_program import program_fixtures, run_program

CASES = mc.golden()
plain, sanitized = program_fixtures("meshlet_decode_host.cpp", exact=True)


def run(exe, tmp_path, streams, payload, offs, primitive_offset, vertex_offset, target, flags, caps, base_offset=0):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    head = np.array([len(streams), streams.shape[1], len(payload), target, flags, primitive_offset, vertex_offset, *caps], np.uint32)
    with open(src, "wb") as f:
        for part in (head, streams, payload, offs):
            f.write(np.ascontiguousarray(part, np.uint32).tobytes())
    run_program(exe, src, dst, base_offset)
    raw, out, at = np.fromfile(dst, np.uint8), {}, 0
    for key, size in (("indices", caps[0] * 3 * mr.index_bytes(flags)), ("positions", caps[1] * 12), ("attributes", caps[1] * 16), ("skin", caps[1] * 8)):
        out[key] = raw[at:at + size]
        at += size
    assert at == raw.size
    return out


def check_golden(exe, tmp_path):
    for name, case in CASES.items():
        mesh = mr.parse(case["file"].tobytes())
        counts = mr.counts_of(mesh["streams"])
        po, vo = (int(x) for x in case["push"])
        caps = mc.capacities(counts, po, vo)
        for target, flags in mc.sets_of(mesh["style"]):
            offs = mr.offsets(counts, int(case["runtime_style"]), flags)
            for base_offset in ((0, 1) if name in ("offsets", "tail_nopad") else (0,)):
                got = run(exe, tmp_path, mesh["streams"], mesh["payload"], offs, po, vo, target, flags, caps, base_offset)
                for key, want in mc.golden_outputs(case, target, flags).items():
                    assert np.array_equal(got[key], want), (name, target, flags, key)


def test_host_build_equals_the_executed_shader(plain, tmp_path):
    check_golden(plain, tmp_path)


def malformed(rng, stream_count):
    meshlets = int(rng.integers(1, 20))
    words = int(rng.integers(1, 200))
    payload = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    streams = np.zeros((meshlets, stream_count, 4), np.uint32)
    streams[:, :, :2] = rng.integers(0, 1 << 32, (meshlets, stream_count, 2), dtype=np.uint64)
    streams[:, 0, :2] = rng.integers(0, 41, (meshlets, 2))  # counts, a fifth of them above 32
    bits = rng.choice([0, 1, 5, 8, 13, 16, 17, 31, 32, 33, 64, 255], (meshlets, stream_count))
    aux = rng.integers(0, 1 << 16, (meshlets, stream_count))
    streams[:, :, 2] = bits | (aux << 16) | (rng.integers(0, 2, (meshlets, stream_count)) << 8)  # the byte above `bits` is ignored
    kind = rng.integers(0, 4, (meshlets, stream_count))
    near_end = words - rng.integers(0, 4, (meshlets, stream_count))
    streams[:, :, 3] = np.where(kind == 0, rng.integers(0, words, (meshlets, stream_count)),
                                np.where(kind == 1, near_end, np.where(kind == 2, 0xffffffff - rng.integers(0, 3, (meshlets, stream_count)),
                                                                       rng.integers(0, 1 << 32, (meshlets, stream_count), dtype=np.uint64))))
    return streams, payload


def test_sanitized_build_on_golden_and_malformed_headers(sanitized, tmp_path):
    check_golden(sanitized, tmp_path)
    rng = np.random.default_rng(20261019)
    for round_ in range(48):
        stream_count = (2, 4, 6)[round_ % 3]
        streams, payload = malformed(rng, stream_count)
        counts = mr.counts_of(streams)
        flags = mc.INDEX_FLAGS[(round_ // 3) % 3]
        offs = mr.offsets(np.minimum(counts, 32), mr.MDI, flags)
        po, vo = (3, 2) if round_ % 2 else (0, 0)
        total = np.minimum(counts, 32).sum(0)
        caps = (int(total[0]) + po, int(total[1]) + vo) if round_ % 4 < 2 else (int(total[0]) // 2 + 1, int(total[1]) // 2 + 1)  # short: elements are dropped
        target = stream_count // 2 - 1
        got = run(sanitized, tmp_path, streams, payload, offs, po, vo, target, flags, caps, base_offset=round_ % 2)
        want = mr.decode(streams, payload, offs, po, vo, target, flags, caps)
        for key in want:
            assert np.array_equal(got[key], want[key]), (round_, key)
