"""GPU: gr_ocean_update_lod, gr_ocean_init_counter_buffer and gr_ocean_cull_blocks on the cases of tests/golden/ocean_lod_shader_v1.npz (the
reference's shaders executed on the CPU; tests/test_ocean_lod_core_cpu.py runs the same cases through the host build of the same code).

update_lod: byte-identical to the golden outside the near-tie mask (ocean_lod_ref.near_tie_mask of the stored float64 LOD) and within one
fp16 code inside it; the number of differing texels is printed per case.  init_counter_buffer: exact.  cull_blocks, fed the golden's LOD
image: counters exact, patches exact as sorted sets per bucket, three times over in one process -- the set must not depend on the order
in which waves arrive."""
import numpy as np
import pytest

import ocean_lod_ref as olr
from granite_amd import capi
from ocean_chain import POISON, as_struct
from ocean_lod_cases import CASES, GOLDEN, assert_cull, assert_lods, spec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def download_image(image):
    raw = np.empty(image.pitch * image.height, np.uint8)
    image.ctx.check(image.ctx.lib.gr_download(image.ctx.handle, None, raw.ctypes.data, image.ptr, raw.nbytes))
    image.ctx.sync()
    return raw.view(np.uint16).reshape(image.height, image.pitch // 2)[:, :image.width]


@pytest.mark.parametrize("name", CASES)
def test_update_lod(gr, name):
    gc = spec(name)[0]
    image = capi.DeviceImage(gr, gc, gc, capi.FORMAT_R16_SFLOAT)
    gr.check(gr.lib.gr_fill_byte(gr.handle, None, image.ptr, POISON, image.pitch * image.height))
    gr.ocean_update_lod(image, as_struct(capi.PushOceanUpdateLod, GOLDEN[name + "/update_push"]))
    gr.sync()
    differing = assert_lods(name, download_image(image), "device")
    print(f"{name}: device differs from the golden in {differing} of {gc * gc} texels")


def test_init_counter_buffer(gr):
    counters = capi.DeviceBuffer(gr, 8 * 32 + 64)
    gr.check(gr.lib.gr_fill_byte(gr.handle, None, counters.ptr, POISON, counters.nbytes))
    gr.ocean_init_counter_buffer(counters, GOLDEN["init/counts16"])
    gr.sync()
    raw = counters.download(np.uint8)
    assert np.array_equal(raw[:256].view(np.uint32).reshape(8, 8), GOLDEN["init/draws"])
    assert np.all(raw[256:] == POISON)


@pytest.mark.parametrize("name", CASES)
def test_cull_blocks(gr, name):
    gc, _, _, wrap = spec(name)
    image = capi.DeviceImage(gr, gc, gc, capi.FORMAT_R16_SFLOAT).upload(np.ascontiguousarray(GOLDEN[name + "/lods"]))
    patches, counters = capi.DeviceBuffer(gr, gc * gc * 8 * 32), capi.DeviceBuffer(gr, 8 * 32)
    push = as_struct(capi.PushOceanCull, GOLDEN[name + "/cull_push"])
    for _ in range(3):
        gr.check(gr.lib.gr_fill_byte(gr.handle, None, patches.ptr, POISON, patches.nbytes))
        gr.ocean_init_counter_buffer(counters, GOLDEN["init/counts16"])
        gr.ocean_cull_blocks(image, wrap, patches, counters, push, GOLDEN[name + "/frustum"].reshape(24))
        gr.sync()
        draws, buffer = counters.download(np.uint32), patches.download(np.uint32)
        assert_cull(name, draws, buffer, "device")
        # slots past instance_count are untouched
        flat = buffer.reshape(8, gc * gc, 8)
        for l in range(8):
            assert np.all(flat[l, int(draws.reshape(8, 8)[l, 1]):].view(np.uint8) == POISON), (name, l)
