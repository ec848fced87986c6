"""CPU: the host layer's part of the VSM chain.  Granite::vsm_half_size is the render graph's rule for the chain's middle image -- an absolute
size times 0.5, converted to unsigned (truncated) and at least 1 -- which tests/shadow_cases.py restates for the golden's 33 x 17 -> 16 x 8;
the three images of a layer are the map's size, that half size, and the map's size again (tests/test_shadow_abi_cpu.py sees the three
launches a layer on upload, tests/test_gpu_shadow_pass.py their result)."""
import shadow_cases as sc
from host_program import PRODUCT, build_program, run_program

SIZES = [1, 2, 3, 4, 5, 17, 33, 1023, 1024, 2047, 2048, 16384]


def test_the_middle_image_is_the_truncated_half_and_at_least_one(tmp_path):
    exe = build_program(tmp_path, "shadow_host", "shadow_host.cpp", extra=PRODUCT)
    got = [int(v) for v in run_program(exe, *SIZES).split()]
    assert got == [max(n // 2, 1) for n in SIZES] == [sc.half_size(n) for n in SIZES]
    assert got[SIZES.index(33)] == 16 and got[SIZES.index(17)] == 8
