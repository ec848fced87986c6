"""CPU: tests/bc_ref.py and the text the device kernel runs, held to the reference's decode shaders executed on the CPU
(tests/golden/bc_decode_shader_v1.npz, recorded by tests/golden/make_bc_decode_golden.py: decode/{s3tc,rgtc,bc7,bc6}.comp on every forced
branch of tests/bc_cases.py).  tests/bc_ref.py is written from the formats' specification (sequential bit reader, the specification's
bit-placement table for BC6H, exact rationals for BC1-BC5); granite_amd/csrc/bc_decode.hpp is built here for the host
(tests/cpp/bc_decode_host.cpp), with the kernel's split of a block over one lane and over four.

BC7 and BC6H must equal the shader's output on every sample.  BC1-BC5 must equal it outside bc_ref's tie mask (exact value ending in
1/2: only BC1's three-colour midpoint, endpoint sums 31 / 21, 63, 105) and lie within one code inside it; ties may cover at most 2 % of
a case's samples, except in the cases that force tie sums, whose differences must lie on tie samples only.  Tie shares the maker
printed: bc1_rgb_random 0.22 %, bc1_rgba_random 0.19 %, bc1_rgb_tie_sums 18.97 %, bc1_rgba_tie_sums 21.39 %, every other case 0 %;
bc_ref differed from the shaders on no sample of any case, tie or not."""
import numpy as np
import pytest

import bc_cases
import bc_ref
from host_program import build_program, run_program

KIND = {131: 0, 132: 0, 133: 1, 134: 1, 135: 2, 136: 2, 137: 3, 138: 3, 139: 4, 141: 5, 143: 6, 144: 7, 145: 8, 146: 8}
CASES = bc_cases.golden()


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    exe = build_program(tmp_path_factory.mktemp("bc_decode"), "bc_decode_host", "bc_decode_host.cpp")

    def run(fmt, blocks, w, h, lanes, tmp):
        src, dst = tmp / "blocks.bin", tmp / "out.bin"
        np.ascontiguousarray(blocks).tofile(src)
        run_program(exe, KIND[fmt], lanes, w, h, src, dst)
        return np.fromfile(dst, np.uint8)
    return run


def held_to_golden(got, name, what):
    """The issue's rule for one decoded image against the shader's."""
    fmt, _, _, _, out = CASES[name]
    _, ties = bc_cases.reference(name)
    got = got.view(out.dtype).reshape(out.shape)
    diff = np.abs(got.astype(np.int64) - out.astype(np.int64))
    if fmt in (bc_ref.BC6H_UFLOAT, bc_ref.BC6H_SFLOAT, bc_ref.BC7_UNORM):
        assert not ties.any() and not diff.any(), (what, name, int((diff > 0).sum()))
    else:
        assert not diff[~ties].any(), (what, name, int((diff[~ties] > 0).sum()))
        assert diff.max(initial=0) <= 1, (what, name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bc_ref_matches_the_executed_shaders(name):
    ref, ties = bc_cases.reference(name)
    print(f"{name}: tie share {100 * ties.mean():.2f} %")
    if not name.endswith("tie_sums"):
        assert ties.mean() <= 0.02, name
    held_to_golden(ref, name, "bc_ref")


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_on_the_host_matches_the_executed_shaders(name, host_decoder, tmp_path):
    fmt, w, h, blocks, _ = CASES[name]
    integer = fmt in (bc_ref.BC6H_UFLOAT, bc_ref.BC6H_SFLOAT, bc_ref.BC7_UNORM)
    for lanes in ((1, 4) if integer else (1,)):
        held_to_golden(host_decoder(fmt, blocks, w, h, lanes, tmp_path), name, f"bc_decode.hpp, {lanes} lane(s) per block")


def test_golden_holds_the_cases_the_generator_makes():
    made = bc_cases.cases()
    assert sorted(made) == sorted(CASES)
    for name, (fmt, w, h, blocks) in made.items():
        assert (fmt, w, h) == CASES[name][:3] and np.array_equal(np.asarray(blocks).reshape(-1), CASES[name][3].reshape(-1)), name


def test_tie_mask_is_bc1_midpoints_only():
    """Ties come from the three-colour midpoint alone: a block with color0 > color1 (four colours) has none, whatever its endpoints."""
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 256, (64, 8), dtype=np.uint8)
    c0 = blocks[:, 0].astype(int) | (blocks[:, 1].astype(int) << 8)
    c1 = blocks[:, 2].astype(int) | (blocks[:, 3].astype(int) << 8)
    hi, lo = np.maximum(c0, c1), np.minimum(c0, c1)
    keep = hi > lo
    blocks[:, 0], blocks[:, 1], blocks[:, 2], blocks[:, 3] = hi & 0xff, hi >> 8, lo & 0xff, lo >> 8
    _, ties = bc_ref.decode(bc_ref.BC1_RGBA_UNORM, blocks[keep].reshape(1, -1, 8), 4 * int(keep.sum()), 4)
    assert not ties.any()


def test_known_blocks():
    """Hand-computed samples: BC1 white / black endpoints, BC4 ramps, the BC7 reserved block, a BC6H reserved block."""
    img, _ = bc_ref.decode(bc_ref.BC1_RGB_UNORM, np.array([0xff, 0xff, 0x00, 0x00, 0xe4, 0xe4, 0xe4, 0xe4], np.uint8), 4, 4)
    assert img[0].tolist() == [[255, 255, 255, 255], [0, 0, 0, 255], [170, 170, 170, 255], [85, 85, 85, 255]]
    img, _ = bc_ref.decode(bc_ref.BC1_RGBA_UNORM, np.array([0x00, 0x00, 0xff, 0xff, 0xe4, 0xe4, 0xe4, 0xe4], np.uint8), 4, 4)
    assert img[0].tolist() == [[0, 0, 0, 255], [255, 255, 255, 255], [128, 128, 128, 255], [0, 0, 0, 0]]
    img, _ = bc_ref.decode(bc_ref.BC1_RGB_UNORM, np.array([0x00, 0x00, 0xff, 0xff, 0xe4, 0xe4, 0xe4, 0xe4], np.uint8), 4, 4)
    assert img[0, 3].tolist() == [0, 0, 0, 255]
    # BC4: e0 = 255 > e1 = 0, indices 0..7 in the first eight texels: 255, 0, then 6/7 .. 1/7 of 255
    idx = sum(k << (3 * k) for k in range(8))
    raw = np.frombuffer((255 | (0 << 8) | (idx << 16)).to_bytes(8, "little"), np.uint8)
    img, _ = bc_ref.decode(bc_ref.BC4_UNORM, raw, 4, 4)
    assert img.reshape(-1)[:8].tolist() == [255, 0, 219, 182, 146, 109, 73, 36]
    raw = np.frombuffer((0 | (255 << 8) | (idx << 16)).to_bytes(8, "little"), np.uint8)
    img, _ = bc_ref.decode(bc_ref.BC4_UNORM, raw, 4, 4)
    assert img.reshape(-1)[:8].tolist() == [0, 255, 51, 102, 153, 204, 0, 255]
    img, _ = bc_ref.decode(bc_ref.BC7_UNORM, np.array([0] + [0xff] * 15, np.uint8), 4, 4)
    assert not img.any()
    img, _ = bc_ref.decode(bc_ref.BC6H_SFLOAT, np.array([0x13] + [0xff] * 15, np.uint8), 4, 4)
    assert (img == np.array([0, 0, 0, 0x3c00], np.uint16)).all()
