"""CPU: the two fp16 conversions of granite_amd/csrc/core_base.hpp built for the host (tests/cpp/core_base_host.cpp, a stand-alone program
that includes that header alone) and held to numpy's float16 conversion.  float_to_half: for every non-NaN half code its value, the value's
two fp32 neighbours, the exact midpoint to the next code (a tie: to even) and the midpoint's two neighbours; +-0, half of the smallest
subnormal, the overflow boundary 0x477fefff / 0x477ff000 and +-inf; 2^20 bit patterns from a fixed seed.  A NaN input must give a NaN of the
same sign with bit 9 (the quiet bit) set; which payload bits survive is not pinned.  half_to_float: all 65536 codes, exactly on every
non-NaN code; a NaN code must give a NaN of the same sign (numpy builds differ in whether they quiet a signalling NaN, the header keeps
the payload as it is).  The program is built plainly and with -fsanitize=address,undefined and run directly (its own main; nothing is
preloaded).  On the device both functions are the hardware conversion, which the GPU tests of env bake, ocean, CACAO, FFT, sky, AA and
post run."""
import numpy as np

from host_program import program_fixtures, run_program


def half_bits(values):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return values.astype(np.float16).view(np.uint16)


def inputs():
    """fp32 bit patterns: the exact cases first, then NaNs"""
    codes = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    codes = codes[(codes & 0x7fff) <= 0x7c00]  # every non-NaN code
    values = codes.view(np.float16).astype(np.float32)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    # the midpoint between code h and the next code of the same sign, exact in fp32 (a 12-bit significand; 2^-25 at the least); the one
    # after the largest finite code is 65520, where the next code would be 2^16.  Nothing lies beyond infinity.
    finite = codes[(codes & 0x7fff) < 0x7c00]
    below = finite.view(np.float16).astype(np.float64)
    above = np.where((finite & 0x7fff) == 0x7bff, np.copysign(65536.0, below), (finite + np.uint16(1)).view(np.float16).astype(np.float64))
    middle = ((below + above) * 0.5).astype(np.float32)
    assert np.array_equal(middle.astype(np.float64), (below + above) * 0.5), "the midpoints are fp32 numbers"
    special = np.array([0x00000000, 0x80000000, 0x33000000, 0xb3000000, 0x477fefff, 0x477ff000, 0xc77fefff, 0xc77ff000, 0x7f800000, 0xff800000],
                       np.uint32)
    random = np.random.default_rng(20261020).integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32)
    is_nan = (random & 0x7fffffff) > 0x7f800000
    exact = np.concatenate([a.view(np.uint32) for a in (values, np.nextafter(values, up), np.nextafter(values, down), middle,
                                                         np.nextafter(middle, up), np.nextafter(middle, down))] + [special, random[~is_nan]])
    nans = np.concatenate([np.array([0x7f800001, 0xff800001, 0x7f802000, 0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff], np.uint32), random[is_nan]])
    return exact, nans


EXACT, NANS = inputs()


plain, sanitized = program_fixtures("core_base_host.cpp", exact=True)


def check(exe, tmp_path):
    out = run_program(exe, input_bytes=np.concatenate([EXACT, NANS]).tobytes(), tmp_path=tmp_path)
    count = EXACT.size + NANS.size
    assert len(out) == 2 * count + 4 * 65536
    halves = np.frombuffer(out, np.uint16, count)
    floats = np.frombuffer(out, np.uint32, 65536, offset=2 * count)

    want = half_bits(EXACT.view(np.float32))
    wrong = np.flatnonzero(halves[:EXACT.size] != want)
    assert wrong.size == 0, [(hex(EXACT[i]), hex(halves[i]), hex(want[i])) for i in wrong[:8]]
    got = halves[EXACT.size:]
    assert np.all((got & 0x7c00) == 0x7c00) and np.all(got & 0x0200), "a NaN stays a NaN, quiet"
    assert np.array_equal(got >> 15, (NANS >> 31).astype(np.uint16)), "a NaN keeps its sign"

    codes = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    is_nan = (codes & 0x7fff) > 0x7c00
    want = codes.view(np.float16).astype(np.float32).view(np.uint32)
    assert np.array_equal(floats[~is_nan], want[~is_nan])
    assert np.all((floats[is_nan] & 0x7fffffff) > 0x7f800000) and np.array_equal(floats[is_nan] >> 31, (codes[is_nan] >> 15).astype(np.uint32))


def test_the_cases_are_what_the_docstring_says():
    assert EXACT.size == 3 * 63490 + 3 * 63488 + 10 + (2 ** 20 - NANS.size + 7) and NANS.size > 7
    assert not np.any((EXACT & 0x7fffffff) > 0x7f800000) and np.all((NANS & 0x7fffffff) > 0x7f800000)
    ties = EXACT[3 * 63490:3 * 63490 + 63488]
    assert np.all((ties & 0xfff) == 0) and np.all((ties[(ties & 0x7fffffff) >= 0x38800000] & 0x1fff) == 0x1000), "midpoints of normal codes: bit 12 alone"


def test_fp16_conversions_equal_numpy(plain, tmp_path):
    check(plain, tmp_path)


def test_fp16_conversions_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path):
    check(sanitized, tmp_path)
