"""CPU: tests/texture_encode_ref.py (numpy) against the reference's own compressor and mip filter run on the CPU
(tests/golden/texture_encode_v1.npz), every byte; the conditions the case set was chosen for, re-asserted from the fixture; the blocks the
issue's table lists; and the fixture's blocks through the project's BC4 / BC5 decoder restatement (tests/bc_ref.py) against the texels the
reference's own decompress_rgtc_red_block recorded."""
import numpy as np
import pytest

import bc_ref
import texture_encode_cases as tc
import texture_encode_ref as ref

GOLDEN = tc.load_golden()
ENCODE = [(name, fmt) for name, case in tc.ENCODE_CASES.items() for fmt in case[3]]


def test_the_fixture_holds_the_inputs_the_case_file_makes():
    for name, image in tc.make_encode_inputs().items():
        assert np.array_equal(GOLDEN[f"enc/{name}/input"], image), name
    for name, level0 in tc.make_mip_inputs().items():
        assert np.array_equal(GOLDEN[f"mip/{name}/level0"], level0), name


@pytest.fixture(scope="module")
def encoded():
    return {(name, fmt): ref.encode_image(GOLDEN[f"enc/{name}/input"], fmt) for name, fmt in ENCODE}


@pytest.mark.parametrize("name,fmt", ENCODE)
def test_encode_matches_the_reference_on_every_byte(encoded, name, fmt):
    w, h, _, _ = tc.ENCODE_CASES[name]
    blocks = GOLDEN[f"enc/{name}/{fmt}/blocks"]
    assert blocks.shape == ((h + 3) // 4, (w + 3) // 4, tc.BLOCK_BYTES[fmt])
    assert np.array_equal(encoded[name, fmt][0], blocks)


def test_the_case_set_reaches_every_class_and_both_ties(encoded):
    infos = [info for _, info in encoded.values()]
    form = np.concatenate([i["form"] for i in infos])
    for kind in (ref.FLAT, ref.SMALL_RANGE, ref.KEPT, ref.SWITCHED):
        assert (form == kind).sum() >= 16, kind
    assert sum(int(i["endpoint_tie"].sum()) for i in infos) >= 16
    assert sum(int(i["incumbent_tie"].sum()) for i in infos) >= 16
    assert (encoded["tiles", tc.BC4][1]["form"] == ref.FLAT).all() and encoded["one", tc.BC4][1]["form"][0] == ref.FLAT


def test_the_hand_made_blocks_give_what_the_reference_gave():
    blocks = GOLDEN[f"enc/hand/{tc.BC4}/blocks"][0]
    for block, (_, ends, bits) in zip(blocks, tc.HAND_BLOCKS):
        assert (int(block[0]), int(block[1])) == ends and int.from_bytes(bytes(block[2:]), "little") == bits


def test_blue_and_alpha_do_not_matter():
    image = GOLDEN["enc/edge_rgba8/input"].copy()
    image[:, :, 2:] ^= 0xff
    for fmt in (tc.BC4, tc.BC5):
        assert np.array_equal(ref.encode_image(image, fmt)[0], GOLDEN[f"enc/edge_rgba8/{fmt}/blocks"])


@pytest.mark.parametrize("name,fmt", ENCODE)
def test_the_blocks_decode_to_what_the_reference_decodes(name, fmt):
    blocks, recorded = GOLDEN[f"enc/{name}/{fmt}/blocks"], GOLDEN[f"enc/{name}/{fmt}/decoded"]
    h, w, _ = recorded.shape
    decoded, ties = bc_ref.decode(fmt, blocks, w, h)
    decoded = np.asarray(decoded).reshape(recorded.shape).astype(np.int64)
    ties = np.asarray(ties).reshape(recorded.shape)
    diff = np.abs(decoded - recorded)
    assert not diff[~ties].any() and diff.max() <= 1  # an exact half may go either way (bc_ref.py)


@pytest.mark.parametrize("name", tc.MIP_CASES)
def test_mips_match_the_reference_on_every_byte(name):
    fmt, w, h, layers, levels = tc.MIP_CASES[name]
    chain = ref.mip_chain(GOLDEN[f"mip/{name}/level0"], levels)
    assert [c.shape[1:3] for c in chain] == [(tc.level_extent(h, l), tc.level_extent(w, l)) for l in range(levels)]
    assert np.array_equal(ref.pack_chain(chain, fmt), GOLDEN[f"mip/{name}/payload"])


def test_the_two_to_one_case_separates_roundf_from_rintf():
    level0 = GOLDEN["mip/rg8_16x16/level0"][0]
    v = ref.mip_level_float(level0)
    halves = (v - np.floor(v) == 0.5) & (np.floor(v) % 2 == 0)
    assert halves.sum() >= 16
    level1 = tc.chain_level(GOLDEN["mip/rg8_16x16/payload"], *tc.MIP_CASES["rg8_16x16"], 1)[0]
    assert np.array_equal(level1[halves], (np.floor(v[halves]) + 1).astype(np.uint8))  # away from zero; rint would give the even one below
    assert not np.array_equal(np.rint(v).astype(np.uint8), level1)
