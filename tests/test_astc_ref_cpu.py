"""CPU: tests/astc_ref.py -- the NumPy decoder of ASTC LDR blocks the GPU tests use where the golden holds no case -- against the
reference's decode shader executed on the CPU (tests/golden/astc_decode_shader_v1.npz): byte for byte on every case (the decode is
integer, there are no ties), its tables entry for entry against the ones the reference's builders made, and the conditions that keep the
case sets honest, asserted again on the recorded outputs."""
import numpy as np
import pytest

import astc_cases
import astc_ref

CASES = astc_cases.golden()


def test_reference_equals_the_executed_shader_on_every_case():
    assert len(CASES) > 250
    for name, (fmt, w, h, blocks, out) in CASES.items():
        assert out.shape == (h, w, 4) and np.array_equal(astc_cases.reference(name), out), name


def test_tables_equal_the_recorded_ones():
    recorded, mine = astc_cases.golden_tables(), astc_ref.tables()
    for key in ("endpoint_quantiser", "endpoint_unquant", "weight_quantiser", "weight_unquant", "trits_quints"):
        assert recorded[key].dtype == mine[key].dtype and np.array_equal(recorded[key], mine[key]), key
    for bw, bh in astc_cases.FULL:
        assert np.array_equal(recorded[f"partition_{bw}x{bh}"], astc_ref.partition_table(bw, bh)), (bw, bh)
    # the scalar statement of the partition function and the table built from all seeds at once
    for seed in (0, 1, 2, 3, 16, 19, 341, 1023):
        for count in (2, 3, 4):
            for bw, bh in ((4, 4), (12, 12)):
                got = [[astc_ref.select_partition(seed, x, y, count, bw * bh < 31) for x in range(bw)] for y in range(bh)]
                table = astc_ref.partition_table(bw, bh)[(seed >> 5) * bh:(seed >> 5) * bh + bh, (seed & 31) * bw:(seed & 31) * bw + bw]
                assert np.array_equal(np.array(got), (table >> (2 * count - 4)) & 3), (seed, count, bw)


def test_every_class_is_present_where_it_can_be():
    for bw, bh in astc_cases.FULL:
        names = {n[len(f"f{bw}x{bh}_"):] for n in CASES if n.startswith(f"f{bw}x{bh}_")}
        want = {"void_ldr", "void_hdr", "err_void_reserved", "err_void_inverted", "err_reserved_mode", "err_reserved_range", "dual_1part", "dual_2part",
                "dual_3part", "part1", "part2", "part3", "part4", "endpoint_bits", "endpoint_trits", "endpoint_quints", "err_weight_bits_low",
                "err_weight_bits_high", "err_dual_4part", "err_endpoint_count", "err_endpoint_bits"}
        want |= {f"cem{m}" for m in astc_ref.LDR_MODES} | {f"err_hdr_cem{m}" for m in astc_ref.HDR_MODES}
        want |= {f"range{r}" for r in range(16) if astc_ref.WEIGHT_QUANTS[r]}
        want |= {f"{c}_{p}part" for c in ("mixed_cem", "same_cem_coded_apart", "err_ldr_and_hdr") for p in (2, 3, 4)}
        assert want <= names, (bw, bh, sorted(want - names))
        for k in range(10):  # every layout of the block-mode table: legal where a grid of it fits the footprint, an error where none does
            assert (f"layout{k}" in names) != (f"err_layout{k}" in names), (bw, bh, k)
        if (bw, bh) != (4, 4):  # a 4 x 4 footprint holds at most 32 weights
            assert "err_weight_count" in names
    assert all(f"layout{k}" in {n[len("f12x12_"):] for n in CASES} for k in range(10))
    for bw, bh in astc_ref.FOOTPRINTS:
        for w, h in astc_cases.tail_sizes(bw, bh):
            assert f"f{bw}x{bh}_tail_{w}x{h}" in CASES
        if (bw, bh) not in astc_cases.FULL:
            assert f"f{bw}x{bh}_parts_single" in CASES and f"f{bw}x{bh}_parts_dual" in CASES


def test_error_classes_hold_errors_and_the_others_at_most_a_quarter():
    for name, (fmt, w, h, blocks, out) in CASES.items():
        share = astc_cases.blocks_with_error(out, *astc_ref.format_footprint(fmt)).mean()
        if astc_cases.is_error_class(name):
            assert share == 1.0, (name, share)
        else:
            assert share <= 0.25, (name, share)


def test_mixed_blocks_keep_their_ldr_texels():
    """The error colour is a texel's: a block with an LDR and an HDR partition holds both error texels and decoded ones."""
    for name, (fmt, w, h, blocks, out) in CASES.items():
        if "err_ldr_and_hdr" in name:
            errors = astc_cases.error_texels(out)
            bw, bh = astc_ref.format_footprint(fmt)
            per_block = errors.reshape(h // bh, bh, w // bw, bw)
            assert per_block.any((1, 3)).all() and not per_block.all((1, 3)).any(), name


def _single_partition_endpoint_values(raw):
    """(N, 8) unquantised endpoint values of single-partition blocks (N, 16), from the fields as the specification places them."""
    t = astc_ref.tables()
    out = np.zeros((len(raw), 8), np.int64)
    for i, block in enumerate(raw):
        v = int.from_bytes(block.tobytes(), "little")
        _, gw, gh, r, dual = astc_ref.block_mode(v & 0x7ff)
        wbits = astc_ref.sequence_bits(astc_ref.WEIGHT_QUANTS[r], gw * gh * (1 + dual))
        pairs = (((v >> 13) & 15) >> 2) + 1
        bits, trits, quints, offset = (int(x) for x in t["endpoint_quantiser"][pairs - 1, 128 - 17 - 2 * dual - wbits])
        lo, hi = astc_ref._keep_low(np.array([v & (2 ** 64 - 1)], np.uint64), np.array([v >> 64], np.uint64), 17 + astc_ref.sequence_bits((bits, trits, quints), 2 * pairs))
        for k in range(2 * pairs):
            out[i, k] = t["endpoint_unquant"][offset + int(astc_ref._sequence_value(lo, hi, 17, np.array([k]), np.array([bits]), np.array([trits]), np.array([quints]))[0])]
    return out


def test_blue_contraction_and_offset_signs_are_both_met():
    """The classes of endpoint modes 8 / 12 hold blocks on either side of the blue-contraction comparison, those of 9 / 13 on either side
    of the sign of the summed offsets, mode 5 offsets of either sign."""
    for mode in (5, 8, 9, 12, 13):
        raw = np.concatenate([CASES[f"f{bw}x{bh}_cem{mode}"][3].reshape(-1, 16) for bw, bh in astc_cases.FULL])
        v = _single_partition_endpoint_values(raw[(raw[:, 1] >> 3) & 3 == 0])  # the single-partition half of the class
        if mode in (8, 12):
            side = v[:, 1] + v[:, 3] + v[:, 5] >= v[:, 0] + v[:, 2] + v[:, 4]
        else:
            offsets = [astc_ref._bit_transfer_signed(v[:, k + 1], v[:, k])[0] for k in (0, 2, 4)]
            side = offsets[0] >= 0 if mode == 5 else offsets[0] + offsets[1] + offsets[2] >= 0
        assert side.any() and not side.all(), mode


def test_hand_computed_blocks():
    # a void extent with colour (0x1234, 0x5678, 0x9abc, 0xdef0): the top bytes
    v = 0x1fc | (3 << 10) | (((1 << 52) - 1) << 12) | (0xdef09abc56781234 << 64)
    block = np.frombuffer(v.to_bytes(16, "little"), np.uint8)
    assert (astc_ref.decode((6, 5), block, 6, 5) == np.array([0x12, 0x56, 0x9a, 0xde], np.uint8)).all()
    # 4 x 4 grid of 2-bit weights (mode 0x42: layout 0, B = 0, A = 2, range 4), one partition, CEM 0 (luminance, 8-bit endpoints 0 and 255), weights 0, 1, 2, 3 ...
    v = 0x42 | (0 << 13) | (0 << 17) | (255 << 25)
    weights = [i % 4 for i in range(16)]
    for i, wgt in enumerate(weights):  # weight i sits at bits 127 - 2 i and 126 - 2 i, its low bit on top
        v |= (wgt & 1) << (127 - 2 * i) | (wgt >> 1) << (126 - 2 * i)
    img = astc_ref.decode((4, 4), np.frombuffer(v.to_bytes(16, "little"), np.uint8), 4, 4)
    # weights 0, 21, 43, 64 of 64: (255 w + 32) >> 6
    assert img[0, :, 0].tolist() == [0, 84, 171, 255] and (img[..., 3] == 255).all() and (img[..., 0] == img[..., 2]).all()
    # all zero but the mode: a reserved weight range -> the error colour
    img = astc_ref.decode((4, 4), np.zeros(16, np.uint8), 4, 4)
    assert (img == np.array(astc_ref.ERROR_COLOUR, np.uint8)).all()
