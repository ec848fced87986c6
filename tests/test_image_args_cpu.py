"""CPU: granite_amd/csrc/image_args.hpp, the one statement of what a launcher asks of a gr_image, through the stand-alone
tests/cpp/image_args_host.cpp built plainly and once with -fsanitize=address,undefined (host code with its own main; nothing is
preloaded).  The program checks the texel-size table against host/vk_subset.hpp, the 64-bit row cover at the three widths that wrap in
32 bits, the alignment rule at exactly the texel size and one byte off, and the byte-range overlap; the table it prints is compared with
capi.FORMAT_BPP here."""
import json
import os

import pytest

from granite_amd import capi
from host_program import ROOT, build_program, run_program


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_contract_on_the_host(tmp_path, sanitized):
    exe = build_program(tmp_path, "image_args_host", "image_args_host.cpp", sanitized=sanitized)
    table = {int(fmt): size for fmt, size in json.loads(run_program(exe, timeout=120)).items()}
    assert table == capi.FORMAT_BPP
    assert not set(table) & set(capi.BLOCK_FORMATS)


def test_no_other_table_and_no_other_row_cover_in_the_kernel_library():
    """What the contract replaced stays replaced: no launcher compares pitch_bytes with a row of its own or converts a gr_image by hand."""
    import glob
    import re
    csrc = os.path.join(ROOT, "granite_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        text = open(path).read()
        assert not re.search(r"(->|\.)pitch_bytes\s*(>=|<)", text), path  # (gr_texture_decode's block_row_pitch_bytes is no gr_image's)
        assert not re.search(r"DevImage(RW)?\s*\{static_cast", text), path
