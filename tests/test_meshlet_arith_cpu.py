"""CPU: decode_mesh's host arithmetic as the host library computes it (granite_amd/csrc/host/mesh/meshlet.cpp: build_decode_offsets,
build_indirect_records, over a view from create_mesh_view), built into a stand-alone program with no device and with
-fsanitize=address,undefined, against tests/meshlet_ref.py -- whose answers tests/test_meshlet_ref_cpu.py holds to hand-written ones --
for meshlet counts 0, 1, 8, 9, 17, both runtime styles, the decode flags and non-zero push offsets."""
import os
import subprocess

import numpy as np
import pytest

import meshlet_cases as mc
import meshlet_ref as mr
from host_program import ROOT, program_fixtures, run_program

program = program_fixtures(["meshlet_host.cpp", os.path.join(ROOT, "granite_amd", "csrc", "host", "mesh", "meshlet.cpp")],
                           extra=["-D__HIP_PLATFORM_AMD__"]).sanitized


@pytest.mark.parametrize("count", [0, 1, 8, 9, 17])
def test_offsets_and_indirect_records_equal_the_restatement(program, tmp_path, count):
    counts = [(i % 3 + 1, i % 4 + 2) for i in range(count)]
    src, dst = tmp_path / "mesh.msh4", tmp_path / "out.bin"
    src.write_bytes(mc.random_file(40 + count, 0, counts, padding=bool(count & 1)))
    counts = np.array(counts, np.int64).reshape(-1, 2)
    for runtime_style in (mr.MDI, mr.MESHLET):
        for flags in (0, mr.UNROLLED_MESH, mr.INDEX_16):
            for po, vo in ((0, 0), (11, 5)):
                run_program(program, src, runtime_style, flags, po, vo, dst, timeout=60)
                raw = np.fromfile(dst, np.uint32)
                assert np.array_equal(raw[:count * 3].reshape(-1, 3), mr.offsets(counts, runtime_style, flags)), (runtime_style, flags)
                assert np.array_equal(raw[count * 3:], mr.indirect(counts, runtime_style, po, vo).reshape(-1)), (runtime_style, flags, po, vo)


def test_a_refused_file_is_refused_with_its_reason(program, tmp_path):
    src = tmp_path / "mesh.msh4"
    src.write_bytes(mc.build_file(1, [mc.random_meshlet(np.random.default_rng(3), 1, 4, 4)], header_overrides={(0, 3, 2): 17}))
    r = subprocess.run([program, str(src), "0", "0", "0", "0", str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5 and "meshlet 0, stream 3: 17 bits" in r.stderr
