"""CPU: the sky in the host layer and the application, without a device (gra_config.device = -1).  gra_config keeps its layout (an
existing test pins volumetric_decals as its last member), so the mode travels in gra_config_ext.sky through gra_create_ext; both
structures are the same in C and in ctypes; the new symbols are bound; gra_create_ext refuses sky without lighting, with aa_bench, with
row bands and outside 0 .. 2, and without the structure it is gra_create;
RenderContext's inv_local_view_projection -- through set_camera and through the hook that installs precomputed parameters -- equals, bit
for bit, what the reference's own math library gave for the golden's cameras (tests/golden/sky_shader_v1.npz: view, projection, inv);
and the Skybox without a cube pushes the directional light's colour and direction and camera_position.y."""
import ctypes as C
import os

import numpy as np
import pytest

import sky_cases as sc
from granite_amd import app as gapp, capi
from host_program import ROOT, c_layout

GOLDEN = sc.load_golden()


def test_the_config_field_and_the_symbols():
    assert gapp.ConfigExt._fields_ == [("struct_size", C.c_uint32), ("sky", C.c_int32)]
    assert "sky" not in [name for name, _ in gapp.Config._fields_], "gra_config's layout is the parent's"
    assert (gapp.SKY_OFF, gapp.SKY_ATMOSPHERE, gapp.SKY_CUBE) == (0, 1, 2)
    host = gapp.load_library()
    for name in ("gra_create_ext", "gra_set_sky_cube", "gra_set_sky_cube_gtx", "gra_get_sky_state"):
        assert name in gapp.EXPORTED_SYMBOLS and getattr(host, name).argtypes
    header = open(os.path.join(ROOT, "include", "granite_app.h")).read()
    for text in ("int32_t sky;", "gra_app *gra_create_ext(const gra_config *config, const gra_config_ext *ext, char *error, size_t error_size);",
                 "#define GRA_SKY_ATMOSPHERE 1", "#define GRA_SKY_CUBE 2",
                 "int gra_set_sky_cube(gra_app *app, uint32_t size, uint32_t levels, const void *rgba16f_chain, const float color[3]);"):
        assert text in header, text


def test_gra_config_and_gra_config_ext_are_the_same_in_c_and_in_ctypes(tmp_path):
    got = c_layout(tmp_path, "gra_config", ["volumetric_decals"], "granite_app.h") + c_layout(tmp_path, "gra_config_ext", ["struct_size", "sky"], "granite_app.h")
    assert got == [C.sizeof(gapp.Config), gapp.Config.volumetric_decals.offset, C.sizeof(gapp.ConfigExt), gapp.ConfigExt.struct_size.offset,
                   gapp.ConfigExt.sky.offset]
    assert gapp.Config.volumetric_decals.offset + 4 == C.sizeof(gapp.Config), "volumetric_decals is still the last member"


def test_the_extension_structure_may_be_absent_or_shorter():
    lib = gapp.load_library()
    plain = gapp.Application(64, 48, device=-1)
    cfg = plain.config
    plain.close()
    err = C.create_string_buffer(512)
    for ext in (None, gapp.ConfigExt(4, gapp.SKY_CUBE)):  # a caller compiled before `sky` existed: the member reads as 0
        handle = lib.gra_create_ext(cfg, ext, err, 512)
        assert handle, err.value
        color = (C.c_float * 3)(1.0, 1.0, 1.0)
        assert lib.gra_set_sky_cube(handle, 1, 1, (C.c_uint16 * 24)(), color) < 0 and b"created without sky = 2" in lib.gra_last_error(handle)
        lib.gra_destroy(handle)
    assert not lib.gra_create_ext(cfg, gapp.ConfigExt(2, 0), err, 512) and b"struct_size" in err.value


@pytest.mark.parametrize("kw", [dict(lighting=False, hdr_bloom=False), dict(aa_bench=True, lighting=False, hdr_bloom=False), dict(strip_count=2)],
                         ids=["no_lighting", "aa_bench", "row_bands"])
@pytest.mark.parametrize("sky", [gapp.SKY_ATMOSPHERE, gapp.SKY_CUBE])
def test_configurations_the_sky_is_not_built_for_are_refused(kw, sky):
    with pytest.raises(capi.GraniteHipError, match="sky needs enable_lighting and is not available with aa_bench or row bands"):
        gapp.Application(64, 48, device=-1, sky=sky, **kw)


def test_a_sky_value_outside_the_three_is_refused():
    for value in (3, -1):
        with pytest.raises(capi.GraniteHipError, match="sky must be 0"):
            gapp.Application(64, 48, device=-1, sky=value)


def test_set_sky_cube_needs_the_cube_mode():
    a = gapp.Application(64, 48, device=-1, sky=gapp.SKY_ATMOSPHERE)
    with pytest.raises(capi.GraniteHipError, match="created without sky = 2"):
        a.set_sky_cube(np.zeros(6 * 4, np.uint16), 1, 1)
    a.close()


@pytest.mark.parametrize("name", list(sc.PROCEDURAL) + list(sc.TEXTURED))
def test_inv_local_view_projection_equals_the_reference_math_library(name):
    view, projection, inv = GOLDEN[f"{name}/view"], GOLDEN[f"{name}/projection"], GOLDEN[f"{name}/inv"]
    assert view[12:15].any(), "the camera is away from the origin: the translation has to be zeroed"
    width, height = (int(v) for v in name.split("/")[1].split("x"))
    a = gapp.Application(width, height, device=-1, sky=gapp.SKY_ATMOSPHERE)
    a.set_camera(projection, view)
    state = a.get_sky_state()
    assert np.array_equal(state["inv_local_view_projection"].view(np.uint32), inv.view(np.uint32)), f"{name}: through set_camera"
    # the hook: the six matrices of a.get_render_parameters() installed verbatim into a fresh application
    params = a.get_render_parameters()
    b = gapp.Application(width, height, device=-1, sky=gapp.SKY_ATMOSPHERE)
    assert not np.array_equal(b.get_sky_state()["inv_local_view_projection"], inv)
    b.set_render_parameters(params)
    assert np.array_equal(b.get_sky_state()["inv_local_view_projection"].view(np.uint32), inv.view(np.uint32)), f"{name}: through set_render_parameters"
    assert np.array_equal(b.get_sky_state()["local_view_projection"], state["local_view_projection"])
    a.close()
    b.close()


def test_the_push_values_without_a_cube():
    name = "mie_peak/136x72"
    a = gapp.Application(136, 72, device=-1, sky=gapp.SKY_ATMOSPHERE)
    a.set_camera(GOLDEN[f"{name}/projection"], GOLDEN[f"{name}/view"])
    a.set_directional((0.0, 3.0, -4.0), (2.0, 3.0, 5.0))
    state = a.get_sky_state()
    assert np.array_equal(state["color"], np.float32([2.0, 3.0, 5.0]))
    assert np.allclose(state["direction"], [0.0, 0.6, -0.8], rtol=1e-6)
    assert state["camera_height"] == a.get_render_parameters()[97] and abs(state["camera_height"] - 1500.0) < 1e-2
    a.close()
