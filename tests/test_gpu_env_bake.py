"""GPU: gr_env_equirect_to_cube, gr_env_specular and gr_env_diffuse against the reference's skybox_latlon.frag, util/ibl_specular.frag
and util/ibl_diffuse.frag executed on the CPU (tests/golden/env_bake_shader_v1.npz), on every recorded case, and
Application.bake_environment through its three files.

Tolerance.  The bound is never taken from the kernels' output.  Measured on the CPU (tests/golden/make_env_bake_golden.py prints it,
tests/test_env_ref_cpu.py asserts it): the distance between the executed shaders (fp32, libm) and tests/env_ref.py (float64), per
case, in fp16 ulps beyond the standing absolute allowance of 1e-4:

    equirect_5 0.000   equirect_16 0.949   specular_24 0.000   specular_16 0.000   diffuse_8 0.987   diffuse_4 0.000

Every figure is below one fp16 ulp: two evaluations that agree to fp32 accuracy land at most one fp16 rounding step apart (the 1024- and
15 876-term sums carry a relative error near 1e-6, three orders below an fp16 step), and no texel of the reference pair is
ill-conditioned.  The standing bound of tests/util.assert_rgba16f_close (2 fp16 ulps + 1e-4) covers that with a whole ulp to spare, so
it is the bound here as well, everywhere, with no allowance for ill-conditioned pixels."""
import os

import numpy as np
import pytest

import env_ref
from granite_amd import app as gapp
from granite_amd import capi, gtx
from util import assert_rgba16f_close

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_bake_shader_v1.npz"))
GUARD = 0xA5


def chain_buffer(gr, size, levels, bits=None):
    """A device buffer holding a chain followed by 64 guard bytes."""
    nbytes = gr.lib.gr_cube_chain_bytes(size, levels)
    assert nbytes == 8 * env_ref.chain_texels(size, levels)
    raw = np.full(nbytes + 64, GUARD, np.uint8)
    if bits is not None:
        raw[:nbytes] = np.ascontiguousarray(bits, np.uint16).reshape(-1).view(np.uint8)
    return capi.DeviceBuffer(gr, raw.size).upload(raw), nbytes


def read_chain(buf, nbytes):
    raw = buf.download()
    assert (raw[nbytes:] == GUARD).all(), "bytes behind the chain were written"
    return raw[:nbytes].view(np.uint16).reshape(-1, 4)


def run_equirect(gr, equirect_bits, size, levels):
    h, w = equirect_bits.shape[:2]
    image = capi.DeviceImage(gr, w, h, capi.FORMAT_R16G16B16A16_SFLOAT).upload(equirect_bits)
    cube, nbytes = chain_buffer(gr, size, levels)
    gr.env_equirect_to_cube(image, cube, size, levels)
    gr.sync()
    return read_chain(cube, nbytes)


def run_specular(gr, src_bits, src_size, src_levels, out_size, out_levels):
    src, _ = chain_buffer(gr, src_size, src_levels, src_bits)
    out, nbytes = chain_buffer(gr, out_size, out_levels)
    gr.env_specular(src, src_size, src_levels, out, out_size, out_levels)
    gr.sync()
    return read_chain(out, nbytes)


def run_diffuse(gr, src_bits, src_size, src_levels, out_size):
    src, _ = chain_buffer(gr, src_size, src_levels, src_bits)
    out, nbytes = chain_buffer(gr, out_size, 1)
    gr.env_diffuse(src, src_size, src_levels, out, out_size)
    gr.sync()
    return read_chain(out, nbytes)


def close(name, got, want):
    want = np.asarray(want, np.uint16).reshape(-1, 4)
    d = env_ref.ulp_distance(got, want)
    print(f"{name}: max {d.max():.3f} fp16 ulps beyond abs 1e-4 from the executed shaders over {want.shape[0]} texels")
    assert_rgba16f_close(got, want, what=name)


@pytest.mark.parametrize("name", ["equirect_5", "equirect_16"])
def test_equirect_to_cube_matches_the_executed_shader(gr, name):
    size, levels = (int(v) for v in GOLDEN[name + "/params"])
    close(name, run_equirect(gr, GOLDEN[name + "/equirect"], size, levels), GOLDEN[name + "/out"])


@pytest.mark.parametrize("name", ["specular_24", "specular_16"])
def test_specular_matches_the_executed_shader(gr, name):
    src_size, src_levels, out_size, out_levels = (int(v) for v in GOLDEN[name + "/params"])
    got = run_specular(gr, GOLDEN[name + "/src"], src_size, src_levels, out_size, out_levels)
    assert (got[:, 3] == 0x3C00).all()
    close(name, got, GOLDEN[name + "/out"])


@pytest.mark.parametrize("name", ["diffuse_8", "diffuse_4"])
def test_diffuse_matches_the_executed_shader(gr, name):
    src_size, src_levels, out_size = (int(v) for v in GOLDEN[name + "/params"])
    got = run_diffuse(gr, GOLDEN[name + "/src"], src_size, src_levels, out_size)
    assert (got[:, 3] == 0x3C00).all()
    close(name, got, GOLDEN[name + "/out"])


def test_specular_lane_and_wave_paths_agree_on_a_constant_cube(gr):
    """64 texels a side puts level 0 (24 576 texels) on the texel-per-lane path and the levels below on the wave-per-texel path: a
    constant cube must come out as that constant on both (the weights divide out exactly up to fp32 rounding)."""
    size, levels = 4, 3
    src = np.zeros((env_ref.chain_texels(size, levels), 4), np.float16)
    src[:] = (3.5, 0.25, 700.0, 1.0)
    got = run_specular(gr, src.view(np.uint16), size, levels, 64, 7)
    assert_rgba16f_close(got, np.broadcast_to(src[0].view(np.uint16), got.shape), what="constant cube")


def test_application_bakes_and_rereads_its_three_files(gr, tmp_path):
    name = "equirect_16"
    equirect = GOLDEN[name + "/equirect"]  # 48 x 24 at scale 1: cube 16 with its full chain of 5, the recorded case
    src = str(tmp_path / "equirect.gtx")
    gtx.write(src, capi.FORMAT_R16G16B16A16_SFLOAT, [equirect])
    paths = {k: str(tmp_path / (k + ".gtx")) for k in ("cube", "reflection", "irradiance")}
    application = gapp.Application(64, 64, lighting=False)
    application.bake_environment(src, cube_scale=1.0, **paths)
    application.close()
    files = {k: gtx.read(p) for k, p in paths.items()}
    for k, (size, levels) in {"cube": (16, 5), "reflection": (128, 8), "irradiance": (32, 1)}.items():
        info = files[k].info
        assert (info.format, info.width, info.height, info.depth, info.layers, info.levels) == (capi.FORMAT_R16G16B16A16_SFLOAT, size, size, 1, 6, levels), k
        assert info.flags & 1, k  # MEMORY_MAPPED_TEXTURE_CUBE_MAP_COMPATIBLE_BIT
        assert info.payload_size == gr.lib.gr_cube_chain_bytes(size, levels)
        assert [files[k].level_offset(l) for l in range(levels)] == [gr.lib.gr_cube_chain_offset(size, l, 0) for l in range(levels)]
    cube_bits = np.asarray(files["cube"].payload).view(np.uint16).reshape(-1, 4)
    close("bake_environment cube", cube_bits, GOLDEN[name + "/out"])
    # the reference's 128 / 8 and 32 sizes have no golden: byte for byte what the entry points give for the same cube
    assert np.array_equal(np.asarray(files["reflection"].payload).view(np.uint16).reshape(-1, 4), run_specular(gr, cube_bits, 16, 5, 128, 8))
    assert np.array_equal(np.asarray(files["irradiance"].payload).view(np.uint16).reshape(-1, 4), run_diffuse(gr, cube_bits, 16, 5, 32))
