"""GPU: gr_ocean_generate_fft, gr_ocean_bake_maps and gr_ocean_mipmap on the cases of tests/golden/ocean_shader_v1.npz (the reference's
shaders executed on the CPU; tests/test_ocean_core_cpu.py runs the same cases through the host build of the same code): generate within
ocean_ref.GENERATE_BOUND_UNITS of the float64 reference, bake and mipmap bit for bit.  Then the update chained entry point by entry point
at N = 128 / 64 -- three spectra, three FFT plans as the ocean configures them, bake, three mip chains -- with the FFT outputs held to
numpy's float64 inverse DFT of the fp16 spectra as stored and everything after them to ocean_ref bit for bit; and misuse, which must be
refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import fft_ref
import ocean_chain
import ocean_ref as ocr
from granite_amd import capi
from ocean_cases import BAKE, GENERATE, GOLDEN, MIPMAP, generate_inputs, hermitian_defect
from ocean_chain import FORMATS, PERIOD, POISON, as_struct, poisoned, run_generate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def image(gr, bits, channels):
    bits = np.ascontiguousarray(bits)
    return capi.DeviceImage(gr, bits.shape[1], bits.shape[0], FORMATS[channels]).upload(bits)


@pytest.mark.parametrize("name", GENERATE)
def test_generate(gr, name):
    d, push, variant, bands = generate_inputs(name)
    out = run_generate(gr, d, push, variant, bands)
    spectrum, s = ocr.generate(d, push, variant, bands)
    distance = ocr.generate_distance(out, spectrum, s)
    print(f"{name}: device {distance:.3f} units")
    assert distance <= ocr.GENERATE_BOUND_UNITS
    # with band modulation the amplitude follows max(F.x, F.y) of the aliased frequency, which the mirror does not share
    if variant == ocr.HEIGHT and bands is None and push.view(np.float32)[5] == 0.0:
        assert hermitian_defect(out) == 0


@pytest.mark.parametrize("name", BAKE)
def test_bake_maps(gr, name):
    size, vertex = (int(v) for v in GOLDEN[name + "/spec"])
    height, disp = image(gr, GOLDEN["bake/height"], 1), image(gr, GOLDEN[f"bake/displacement{size}"], 2)
    gj = capi.DeviceImage(gr, 64, 64, FORMATS[4])
    hd = capi.DeviceImage(gr, 64, 64, FORMATS[4]) if vertex else None
    gr.ocean_bake_maps(height, disp, gj, hd, as_struct(capi.PushOceanBake, GOLDEN[name + "/push"]))
    gr.sync()
    assert np.array_equal(gj.download(), GOLDEN[name + "/grad_jacobian"])
    if vertex:
        assert np.array_equal(hd.download(), GOLDEN[name + "/height_displacement"])


@pytest.mark.parametrize("name", MIPMAP)
def test_mipmap(gr, name):
    w, h, channels = (int(v) for v in GOLDEN[name + "/spec"])
    src = image(gr, GOLDEN[f"mipmap/in_{w}x{h}_c{channels}"], channels)
    out = capi.DeviceImage(gr, w // 2, h // 2, FORMATS[channels])
    gr.ocean_mipmap(src, out, as_struct(capi.PushOceanMipmap, GOLDEN[name + "/push"]))
    gr.sync()
    assert np.array_equal(out.download().reshape(h // 2, w // 2, channels), GOLDEN[name + "/out"])


# ---- the update, entry point by entry point ----------------------------------------------------------------------------------------------
N, SHIFT = 128, 1


def spectrum_of(bits):
    return ocr.half_to_float((bits & 0xffff).astype(np.uint16)) + 1j * ocr.half_to_float((bits >> 16).astype(np.uint16))


def run_update(gr, time, spd=False):
    """ocean_size 128 / grid_count 4 / grid_resolution 32 at fft_resolution 128: world size 128, samples 1 apart, 5 vertex levels"""
    height_d = np.ascontiguousarray(GOLDEN["generate/distribution"])
    normal_d = np.ascontiguousarray(np.roll(height_d, (5, 9), (0, 1)) * np.float32(0.01))  # another field; small, as its gradient factor reaches 32
    return ocean_chain.run_update(gr, height_d, ocean_chain.downsample_distribution(height_d, SHIFT), normal_d, time, spd=spd)


@pytest.fixture(scope="module")
def update(gr):
    return run_update(gr, np.float32(44.0))  # fmod(300, 256)


def test_fft_as_the_ocean_uses_it(update):
    m = N >> SHIFT
    height = spectrum_of(update["height-fft-input"])
    want = np.fft.irfft2(height[:, :N // 2 + 1], s=(N, N)) * (N * N)
    ratio = fft_ref.worst_row_ratio(ocr.half_to_float(update["height-fft-output"]), want)
    print(f"height C2R: worst row ratio {ratio:.3g}")
    assert ratio <= 5e-4
    for name, size in (("displacement", m), ("normal", N)):
        want = np.fft.ifft2(spectrum_of(update[name + "-fft-input"])) * (size * size)
        out = ocr.half_to_float(update[name + "-fft-output"])
        ratio = fft_ref.worst_row_ratio(out[..., 0] + 1j * out[..., 1], want)
        print(f"{name} inverse C2C: worst row ratio {ratio:.3g}")
        assert ratio <= 5e-4


def test_bake_and_chains_after_the_fft(update):
    gj, hd = ocr.bake_maps(update["height-fft-output"], update["displacement-fft-output"], update["bake-push"])
    assert np.array_equal(update["gradient-jacobian"][0], gj) and np.array_equal(update["height-displacement"][0], hd)
    for name, level0, levels, mod in (("gradient-jacobian", gj, 8, (1.0, 1.0, 1.0, 1.0)), ("height-displacement", hd, 5, (0.0, 1.0, 1.0, 1.0)),
                                      ("normal", update["normal-fft-output"], 8, (1.0, 1.0, 1.0, 1.0))):
        want = ocr.mip_chain(level0, levels, mod)
        assert len(update[name]) == levels
        for level, (a, b) in enumerate(zip(update[name], want)):
            assert np.array_equal(a, b), (name, level)
    assert not np.any(update["height-displacement"][-1][..., 0] & 0x7fff)
    assert update["normal"][-1].shape == (1, 1, 2)


def test_update_repeats_bit_for_bit(gr, update):
    again = run_update(gr, np.float32(44.0))
    for key, value in update.items():
        for a, b in zip(value if isinstance(value, list) else [value], again[key] if isinstance(value, list) else [again[key]]):
            assert np.array_equal(a, b), key


def test_single_pass_chains_of_the_update(gr, update):
    """The route the pass takes for its two RGBA16F chains: gr_spd_downsample with 3 components, the vertex chain's last level times
    (0, 1, 1, 1).  Level 0 and the normal chain are untouched by the choice; level 1 is one LinearClamp tap at the footprint centre, where
    clamp and wrap agree, so but for the fourth component cut to 0 it is the mipmap shader's level 1 bit for bit; the deeper levels are
    2 x 2 averages with the downsampler's own rounding points, held to fp16 neighbours of the level-by-level chain."""
    spd = run_update(gr, np.float32(44.0), spd=True)
    for key in ("height-fft-input", "normal-fft-input", "displacement-fft-input", "height-fft-output", "displacement-fft-output", "normal-fft-output"):
        assert np.array_equal(spd[key], update[key]), key
    for a, b in zip(spd["normal"], update["normal"]):
        assert np.array_equal(a, b)
    for name in ("gradient-jacobian", "height-displacement"):
        assert len(spd[name]) == len(update[name])
        assert np.array_equal(spd[name][0], update[name][0])
        assert np.array_equal(spd[name][1][..., :3], update[name][1][..., :3]), name
        for level, (a, b) in enumerate(zip(spd[name], update[name])):
            assert a.shape == b.shape and not np.any(a[..., 3] & 0x7fff), (name, level)
    assert not np.any(spd["height-displacement"][-1][..., 0] & 0x7fff)
    assert np.any(spd["height-displacement"][-2][..., 0] & 0x7fff)


# ---- misuse ------------------------------------------------------------------------------------------------------------------------------
def test_generate_refusals(gr):
    d = np.ascontiguousarray(GOLDEN["generate/distribution"][:64, :64])
    src, out = capi.DeviceBuffer(gr, d.nbytes).upload(d), poisoned(gr, 4 * 64 * 64, 0)
    good = ocr.generate_push((0.05, 0.05), (64, 64), 14.0 / 64, 1.0, PERIOD)

    def call(push=good, variant=0, distribution=src.ptr, target=out.ptr, null_push=False):
        p = None if null_push else C.byref(as_struct(capi.PushOceanGenerate, push))
        return gr.lib.gr_ocean_generate_fft(gr.handle, None, distribution, target, p, variant, None)

    def with_n(nx, ny, period=PERIOD):
        return ocr.generate_push((0.05, 0.05), (nx, ny), 14.0 / 64, 1.0, period)

    refused = [call(distribution=None), call(target=None), call(null_push=True), call(target=src.ptr), call(with_n(96, 64)), call(with_n(64, 48)), call(with_n(32, 64)),
               call(with_n(65536, 32768)), call(with_n(64, 64, 0.0)), call(with_n(64, 64, -1.0)), call(variant=3)]
    assert refused == [-1] * len(refused)
    gr.sync()
    assert np.all(out.download(np.uint8) == POISON)
    assert call() == 0
    gr.sync()


def test_bake_and_mipmap_refusals(gr):
    f = FORMATS
    height, disp = capi.DeviceImage(gr, 64, 64, f[1]), capi.DeviceImage(gr, 32, 32, f[2])
    gj, hd = capi.DeviceImage(gr, 64, 64, f[4]), capi.DeviceImage(gr, 64, 64, f[4])
    for img in (gj, hd):
        gr.check(gr.lib.gr_fill_byte(gr.handle, None, img.ptr, POISON, img.pitch * img.height))
    push = as_struct(capi.PushOceanBake, ocr.bake_push((1 / 64,) * 2 + (1 / 32,) * 2, (8.0,) * 4))
    small, odd, wrong = capi.DeviceImage(gr, 32, 32, f[4]), capi.DeviceImage(gr, 48, 32, f[2]), capi.DeviceImage(gr, 64, 64, f[2])
    bake = lambda h, d, g, v, p=C.byref(push): gr.lib.gr_ocean_bake_maps(gr.handle, None, h, d, g, v, p)
    refused = [bake(None, disp.desc, gj.desc, hd.desc), bake(height.desc, None, gj.desc, hd.desc), bake(height.desc, disp.desc, None, hd.desc),
               bake(height.desc, disp.desc, gj.desc, hd.desc, None), bake(height.desc, odd.desc, gj.desc, hd.desc), bake(height.desc, disp.desc, small.desc, hd.desc),
               bake(height.desc, disp.desc, gj.desc, small.desc), bake(wrong.desc, disp.desc, gj.desc, hd.desc), bake(height.desc, disp.desc, wrong.desc, hd.desc),
               bake(height.desc, disp.desc, gj.desc, gj.desc)]
    assert refused == [-1] * len(refused)

    src, dst = capi.DeviceImage(gr, 64, 64, f[4]), hd
    mp = lambda count=(64, 64): as_struct(capi.PushOceanMipmap, ocr.mipmap_push((1, 1, 1, 1), (1 / 64, 1 / 64), count))
    mip = lambda s, d, p: gr.lib.gr_ocean_mipmap(gr.handle, None, s, d, p)
    r32 = capi.DeviceImage(gr, 64, 64, capi.FORMAT_R32_SFLOAT)
    refused = [mip(None, dst.desc, C.byref(mp())), mip(src.desc, None, C.byref(mp())), mip(src.desc, dst.desc, None), mip(src.desc, dst.desc, C.byref(mp((32, 32)))),
               mip(src.desc, wrong.desc, C.byref(mp())), mip(r32.desc, r32.desc, C.byref(mp())), mip(dst.desc, dst.desc, C.byref(mp()))]
    assert refused == [-1] * len(refused)
    gr.sync()
    for img in (gj, hd):
        assert np.all(img.download().view(np.uint8) == POISON)
