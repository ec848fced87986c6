"""CPU: granite_amd/csrc/image_args.hpp, the one statement of what a launcher asks of a gr_image, through the stand-alone
tests/cpp/image_args_host.cpp built plainly and once with -fsanitize=address,undefined (host code with its own main; nothing is
preloaded).  The program checks the texel-size table against host/vk_subset.hpp, the 64-bit row cover at the three widths that wrap in
32 bits, the alignment rule at exactly the texel size and one byte off, and the byte-range overlap; the table it prints is compared with
capi.FORMAT_BPP here."""
import json
import os
import subprocess

import pytest

from granite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "image_args_host.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_contract_on_the_host(tmp_path, flags):
    exe = tmp_path / "image_args_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), SOURCE])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    table = {int(fmt): size for fmt, size in json.loads(r.stdout).items()}
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
