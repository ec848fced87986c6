"""GPU: gr_meshlet_decode.  Every case of tests/golden/meshlet_decode_shader_v1.npz (the reference's decode shader executed on the CPU),
in every set its file provides, equals the executed shader on every byte of every output: the outputs start filled with a guard byte,
and everything before, between and after the written elements must survive -- non-zero primitive_offset / vertex_offset and an index
buffer whose base pointer is moved by 1 and by 4 bytes included.  Shapes beyond the golden are held to tests/meshlet_ref.py: meshlet
counts at half-wave, wave and workgroup boundaries and past a thousand, the three index widths, the three target styles of a Skinned
file, and a decode split by wg_offset into launches with shortened grids, which must leave the bytes of one full launch."""
import numpy as np
import pytest

import meshlet_cases as mc
import meshlet_ref as mr
from meshlet_device import device_decode

pytestmark = pytest.mark.gpu
CASES = mc.golden()


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case_equals_the_executed_shader(gr, name):
    case = CASES[name]
    mesh = mr.parse(case["file"].tobytes())
    counts = mr.counts_of(mesh["streams"])
    po, vo = (int(x) for x in case["push"])
    caps = mc.capacities(counts, po, vo)
    for target, flags in mc.sets_of(mesh["style"]):
        offs = mr.offsets(counts, int(case["runtime_style"]), flags)
        for base_offset in ((0, 1, 4) if name in ("offsets", "tail_nopad", "counts_32_32") else (0,)):
            got, _ = device_decode(gr, mesh["streams"], mesh["payload"], offs, po, vo, target, flags, caps, base_offset)
            assert np.all(got["before"] == mr.GUARD), (name, target, flags, base_offset)
            for key, want in mc.golden_outputs(case, target, flags).items():
                assert np.array_equal(got[key], want), (name, target, flags, base_offset, key)


@pytest.fixture(scope="module")
def meshes():
    """meshlet count -> (streams, payload, counts) of a seeded Skinned file with unequal counts, full and empty meshlets among them"""
    out = {}
    for count in (1, 2, 3, 7, 8, 9, 65, 1031):
        rng = np.random.default_rng(count)
        counts = np.stack([rng.integers(0, 33, count), rng.integers(0, 33, count)], -1)
        counts[::5] = (32, 32)
        mesh = mr.parse(mc.random_file(1000 + count, 2, [tuple(c) for c in counts], padding=bool(count & 1),
                                       pos_bits=int(rng.choice([0, 7, 12, 16])), uv_bits=int(rng.choice([3, 10, 16])), byte_bits=int(rng.choice([0, 4, 8]))))
        out[count] = (mesh["streams"], mesh["payload"], mr.counts_of(mesh["streams"]))
    return out


@pytest.mark.parametrize("count", [1, 2, 3, 7, 8, 9, 65, 1031])
def test_counts_at_wave_and_workgroup_boundaries(gr, meshes, count):
    streams, payload, counts = meshes[count]
    caps = mc.capacities(counts, 7, 3)
    for target, flags, runtime in ((2, 0, mr.MDI), (2, mr.INDEX_16, mr.MDI), (2, mr.UNROLLED_MESH, mr.MDI), (1, mr.INDEX_16, mr.MESHLET), (0, mr.UNROLLED_MESH, mr.MESHLET)):
        offs = mr.offsets(counts, runtime, flags)
        want = mr.decode(streams, payload, offs, 7, 3, target, flags, caps)
        got, _ = device_decode(gr, streams, payload, offs, 7, 3, target, flags, caps)
        for key in want:
            assert np.array_equal(got[key], want[key]), (count, target, flags, key)


@pytest.mark.parametrize("count,split", [(9, 1), (65, 4), (1031, 100)])
def test_wg_offset_with_a_shortened_grid_decodes_the_same_bytes(gr, meshes, count, split):
    streams, payload, counts = meshes[count]
    caps = mc.capacities(counts, 0, 0)
    flags = mr.INDEX_16
    offs = mr.offsets(counts, mr.MDI, flags)
    full, _ = device_decode(gr, streams, payload, offs, 0, 0, 2, flags, caps)
    tail, outputs = device_decode(gr, streams, payload, offs, 0, 0, 2, flags, caps, wg_offsets=(split,))
    first = int(counts[:8 * split, 0].sum()), int(counts[:8 * split, 1].sum())  # the groups before `split` stay guard
    assert np.all(tail["indices"][:first[0] * 6] == mr.GUARD) and np.all(tail["positions"][:first[1] * 12] == mr.GUARD)
    assert np.array_equal(tail["indices"][first[0] * 6:], full["indices"][first[0] * 6:]) and np.array_equal(tail["skin"][first[1] * 8:], full["skin"][first[1] * 8:])
    head = mr.decode(streams[:8 * split], payload, offs[:8 * split], 0, 0, 2, flags, caps)
    both, _ = device_decode(gr, streams[:8 * split], payload, offs[:8 * split], 0, 0, 2, flags, caps, outputs=outputs)  # the first groups, into the same buffers
    assert np.array_equal(head["indices"][:first[0] * 6], both["indices"][:first[0] * 6])
    for key in full:
        assert np.array_equal(both[key], full[key]), (count, split, key)
