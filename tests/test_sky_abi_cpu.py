"""CPU: the sky ABI.  include/granite_hip.h declares gr_sky_apply and gr_sky_cube with size and offset assertions on the new structures,
the library exports them, capi binds them, and the structures are the same in C and in ctypes.  The launchers' refusals run on the
device (tests/test_gpu_sky.py): they return before a launch."""
import ctypes as C
import os
import re

import pytest

from granite_amd import capi
from host_program import ROOT, c_layout

HEADER = open(os.path.join(ROOT, "include", "granite_hip.h")).read()


def test_the_entry_points_are_declared_exported_and_bound():
    assert re.search(r"int gr_sky_apply\(gr_ctx \*ctx, gr_stream stream, const gr_sky_args \*args\);", HEADER)
    assert re.search(r"int gr_sky_cube\(gr_ctx \*ctx, gr_stream stream, void \*out_chain, uint32_t size, const gr_sky_cube_params \*params\);", HEADER)
    lib = capi.load_library()
    for name in ("gr_sky_apply", "gr_sky_cube"):
        assert name in capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    assert callable(capi.Context.sky_apply) and callable(capi.Context.sky_cube)


def test_the_header_asserts_the_new_structures():
    for line in ("GR_ASSERT_SIZE(gr_sky_args, 160);", "GR_ASSERT_OFFSET(gr_sky_args, inv_local_view_projection, 48);", "GR_ASSERT_OFFSET(gr_sky_args, cube, 144);",
                 "GR_ASSERT_SIZE(gr_sky_cube_params, 32);", "GR_ASSERT_OFFSET(gr_sky_cube_params, sun_direction, 16);"):
        assert line in HEADER, line


@pytest.mark.parametrize("c_name, ct", [("gr_sky_args", capi.SkyArgs), ("gr_sky_cube_params", capi.SkyCubeParams)])
def test_the_structures_are_the_same_in_c_and_in_ctypes(tmp_path, c_name, ct):
    fields = [name for name, _ in ct._fields_]
    assert c_layout(tmp_path, c_name, fields) == [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields]


def test_the_kernel_file_is_built_without_contraction():
    makefile = open(os.path.join(ROOT, "granite_amd", "csrc", "Makefile")).read()
    exact = re.search(r"^EXACT_SRCS := (.*)$", makefile, re.M).group(1).split()
    kernels = re.search(r"^KERNEL_SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "sky.hip" in exact and "sky.hip" in kernels
