"""CPU: tests/ocean_ref.py against the reference's three ocean shaders executed on the CPU (tests/golden/ocean_shader_v1.npz): generate
within the measured distance plus one unit and without a flipped round(), bake_maps and mipmap bit for bit in their fp32 restatement and
to rounding in float64; and the golden's bake and mipmap cases do test the wrap."""
import numpy as np
import pytest

import ocean_ref as ocr
from ocean_cases import BAKE, GENERATE, GOLDEN, MIPMAP, generate_inputs


def test_golden_covers_what_it_should():
    assert len(GENERATE) == 18 and len(BAKE) == 5 and len(MIPMAP) == 18
    shapes = {tuple(GOLDEN[c + "/push"][2:4]) for c in GENERATE}
    assert shapes == {(64, 64), (128, 64), (128, 128)}
    assert {tuple(GOLDEN[c + "/spec"]) for c in GENERATE} == {(v, b) for v in range(3) for b in range(2)}
    assert len(set(GOLDEN["generate/bands"].tolist())) == 8
    # the recorded distance of the executed shader from ocean_ref is the one the bound is built on
    assert round(float(GOLDEN["generate/measured_units"]), 3) == ocr.GENERATE_MEASURED_UNITS


@pytest.mark.parametrize("name", GENERATE)
def test_generate(name):
    d, push, variant, bands = generate_inputs(name)
    spectrum, s = ocr.generate(d, push, variant, bands)
    distance = ocr.generate_distance(GOLDEN[name + "/out"], spectrum, s)
    print(f"{name}: {distance:.3f} units")
    assert distance <= ocr.GENERATE_MEASURED_UNITS + 0.0005  # the measurement itself, no bin exempt: a flipped round() is whole units away


@pytest.mark.parametrize("name", BAKE)
def test_bake_maps(name):
    size, vertex = (int(v) for v in GOLDEN[name + "/spec"])
    height, disp, push = GOLDEN["bake/height"], GOLDEN[f"bake/displacement{size}"], GOLDEN[name + "/push"]
    gj, hd = ocr.bake_maps(height, disp, push)
    assert np.array_equal(gj, GOLDEN[name + "/grad_jacobian"])
    if vertex:
        assert np.array_equal(hd, GOLDEN[name + "/height_displacement"])
    # float64 is the same formula: fp16 neighbours at worst, where no difference of large texels cancels
    gj64, hd64 = ocr.bake_maps(height, disp, push, np.float64)
    a, b = ocr.half_to_float(hd64), ocr.half_to_float(hd)
    assert np.all(np.abs(a - b) <= 2.0 ** -10 * np.maximum(np.abs(a), 2.0 ** -14))
    # a clamping sampler gives other bytes: the case tests the wrap
    gj_clamp, hd_clamp = ocr.bake_maps(height, disp, push, wrap=False)
    assert not np.array_equal(gj_clamp, gj)
    assert np.array_equal(gj_clamp[4:-4, 4:-4], gj[4:-4, 4:-4])  # ... at the border only (the half-size map's offsets reach 4 texels in)


@pytest.mark.parametrize("name", MIPMAP)
def test_mipmap(name):
    w, h, channels = (int(v) for v in GOLDEN[name + "/spec"])
    src, push = GOLDEN[f"mipmap/in_{w}x{h}_c{channels}"], GOLDEN[name + "/push"]
    out = ocr.mipmap(src, push)
    assert np.array_equal(out, GOLDEN[name + "/out"])
    if "zero_first" in name:
        assert not np.any(out[..., 0] & 0x7fff)
    a, b = ocr.half_to_float(ocr.mipmap(src, push, np.float64)), ocr.half_to_float(out)
    assert np.all(np.abs(a - b) <= 2.0 ** -10 * np.maximum(np.abs(a), 2.0 ** -14))


def test_mipmap_taps_do_not_reach_the_border_but_offsets_would():
    """mipmap.comp's taps sit at the centres of 2 x 2 footprints: wrap and clamp agree there (which is why the reference may use the
    clamping single-pass downsampler for the same chain); a tap moved by half a source texel does cross the border and tells them apart."""
    src = GOLDEN["mipmap/in_8x4_c2"]
    push = ocr.mipmap_push((1, 1, 1, 1), (1 / 8, 1 / 4), (4, 2))
    assert np.array_equal(ocr.mipmap(src, push), ocr.mipmap(src, push, wrap=False))
    image = ocr.half_to_float(src, np.float32)
    u, v = np.float32([[0.0]]), np.float32([[0.0]])  # the corner: the four texels around it are the image's four corners
    wrapped = ocr.sample(image, u, v)[0, 0]
    corners = (image[0, 0] + image[0, -1] + image[-1, 0] + image[-1, -1]) / 4
    assert np.allclose(wrapped, corners, rtol=1e-6) and not np.allclose(ocr.sample(image, u, v, wrap=False)[0, 0], corners, rtol=1e-3)


def test_mip_chain_last_level():
    chain = ocr.mip_chain(GOLDEN["mipmap/in_64x64_c4"], 5, (0.0, 1.0, 1.0, 1.0))
    assert [c.shape for c in chain] == [(64 >> i, 64 >> i, 4) for i in range(5)]
    assert not np.any(chain[-1][..., 0] & 0x7fff) and np.any(chain[-2][..., 0] & 0x7fff)
