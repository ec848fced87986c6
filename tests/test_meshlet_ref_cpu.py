"""CPU: tests/meshlet_ref.py -- the numpy restatement of the MESHLET4 decode -- equals the reference's decode shader executed on the CPU
(tests/golden/meshlet_decode_shader_v1.npz) on every case, set and byte (positions and UV as bit patterns: the buffers are bytes); its
host arithmetic (decode_mesh's Offsets and both indirect layouts) equals hand-written answers; the golden holds the classes
tests/meshlet_cases.py lists, the 13 .. 15-bit loss among them; and packUnorm4x8(unpackUnorm4x8(b)) is b for all 256 bytes, which is
what lets the decoder copy bone weights."""
import numpy as np
import pytest

import meshlet_cases as mc
import meshlet_ref as mr

CASES = mc.golden()
# seventeen meshlets: prim_count i % 3 + 1, vert_count i % 4 + 2, and their running sums, written out
PRIMS = [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2]
VERTS = [2, 3, 4, 5, 2, 3, 4, 5, 2, 3, 4, 5, 2, 3, 4, 5, 2]
PRIM_BEFORE = [0, 1, 3, 6, 7, 9, 12, 13, 15, 18, 19, 21, 24, 25, 27, 30, 31]
VERT_BEFORE = [0, 2, 5, 9, 14, 16, 19, 23, 28, 30, 33, 37, 42, 44, 47, 51, 56]
VERT_BEFORE_IN_CHUNK = [0, 2, 5, 9, 14, 16, 19, 23, 0, 2, 5, 9, 14, 16, 19, 23, 0]
MDI_DRAWS = {1: [(3, 33, 5)], 8: [(45, 33, 5)], 9: [(45, 33, 5), (9, 78, 33)], 17: [(45, 33, 5), (48, 78, 33), (6, 126, 61)]}  # push offsets 11 and 5


def test_the_golden_holds_the_listed_classes():
    assert set(CASES) == set(mc.cases())
    for name, (data, po, vo, runtime_style) in mc.cases().items():  # the writer is deterministic: the files are the recorded ones
        assert np.array_equal(np.frombuffer(data, np.uint8), CASES[name]["file"]), name
    assert {f"pos_bits_{b}" for b in (0, 1, 5, 8, 11, 12, 13, 14, 15, 16)} <= set(CASES)
    assert {f"uv_bits_{b}" for b in range(17)} | {f"byte_bits_{b}" for b in range(9)} | {f"tangent_mode_{a}" for a in (1, 2, 3)} <= set(CASES)
    padded, bare = CASES["tail_pad"]["file"], CASES["tail_nopad"]["file"]
    assert len(padded) == len(bare) + 4 and np.array_equal(padded[:-4], bare) and not padded[-4:].any()
    mesh = mr.parse(bare.tobytes())
    last = mesh["streams"][-1, -1]
    assert int(last[3]) + 32 == mesh["payload_words"] and int(last[2]) & 0xff == 8  # 32 elements of 32 bits end at the last word


@pytest.mark.parametrize("name", sorted(CASES))
def test_ref_equals_the_executed_shader(name):
    case = CASES[name]
    mesh = mr.parse(case["file"].tobytes())
    counts = mr.counts_of(mesh["streams"])
    po, vo = (int(x) for x in case["push"])
    caps = mc.capacities(counts, po, vo)
    for target, flags in mc.sets_of(mesh["style"]):
        offs = mr.offsets(counts, int(case["runtime_style"]), flags)
        got = mr.decode(mesh["streams"], mesh["payload"], offs, po, vo, target, flags, caps)
        for key, want in mc.golden_outputs(case, target, flags).items():
            assert np.array_equal(got[key], want), (name, target, flags, key)


def ideal_positions(mesh):
    """base + delta of the position stream read bit by bit, with no window: what 13 .. 15 bits would give if nothing were lost"""
    bits = np.unpackbits(mesh["payload"].view(np.uint8), bitorder="little")
    out = []
    for m in range(mesh["meshlet_count"]):
        s = mesh["streams"][m, 1]
        b, base = int(s[2]) & 0xff, (int(s[0]) & 0xffff, int(s[0]) >> 16, int(s[1]) & 0xffff)
        for lane in range(int(mesh["streams"][m, 0, 1])):
            for c in range(3):
                at = int(s[3]) * 32 + (lane * 3 + c) * b
                out.append((int(bits[at:at + b].dot(1 << np.arange(b))) + base[c]) & 0xffff)
    return np.array(out, np.uint16).view(np.int16)


@pytest.mark.parametrize("bits,loses", [(12, False), (13, True), (14, True), (15, True), (16, False)])
def test_13_to_15_bits_lose_the_high_bits_the_shader_loses(bits, loses):
    case = CASES[f"pos_bits_{bits}"]
    mesh = mr.parse(case["file"].tobytes())
    exponent = int(mesh["streams"][0, 1, 2].astype(np.int32) >> 16)
    vertices = int(mr.counts_of(mesh["streams"])[:, 1].sum())
    recorded = case["positions"][:vertices * 12].view(np.float32)
    ideal = np.ldexp(ideal_positions(mesh).astype(np.float32), exponent).astype(np.float32)
    assert (not np.array_equal(recorded, ideal)) == loses


@pytest.mark.parametrize("count", [1, 8, 9, 17])
def test_offsets_and_indirect_records_equal_known_answers(count):
    counts = np.array(list(zip(PRIMS, VERTS))[:count], np.int64)
    zeros = [0] * count
    for runtime_style, flags, index_offset in ((mr.MESHLET, 0, zeros), (mr.MESHLET, mr.UNROLLED_MESH, zeros), (mr.MESHLET, mr.INDEX_16, zeros),
                                               (mr.MDI, mr.UNROLLED_MESH, VERT_BEFORE[:count]), (mr.MDI, mr.UNROLLED_MESH | mr.INDEX_16, VERT_BEFORE[:count]),
                                               (mr.MDI, 0, VERT_BEFORE_IN_CHUNK[:count]), (mr.MDI, mr.INDEX_16, VERT_BEFORE_IN_CHUNK[:count])):
        want = np.array(list(zip(PRIM_BEFORE[:count], VERT_BEFORE[:count], index_offset)), np.uint32)
        assert np.array_equal(mr.offsets(counts, runtime_style, flags), want), (runtime_style, flags)
    chunks = (count + 7) // 8
    want = np.zeros((chunks * 8, 4), np.uint32)  # the last chunk is zero-padded
    want[:count] = [(11 + PRIM_BEFORE[i], 5 + VERT_BEFORE[i], PRIMS[i], VERTS[i]) for i in range(count)]
    assert np.array_equal(mr.indirect(counts, mr.MESHLET, 11, 5), want)
    assert np.array_equal(mr.indirect(counts, mr.MDI, 11, 5), np.array(MDI_DRAWS[count], np.uint32))
    assert np.array_equal(mr.indirect(counts, mr.MDI)[0], [3 * sum(PRIMS[:min(count, 8)]), 0, 0])


def test_unorm4x8_round_trip_is_the_identity_on_every_byte():
    assert [mr.unorm4x8_round_trip(b) for b in range(256)] == list(range(256))
