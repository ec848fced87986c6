"""GPU: gr_fft_* on the shapes of tests/fft_ref.py (the ones tests/test_fft_core_cpu.py runs through the host build of the same code)
against numpy's float64 DFT under the same bounds: 1e-10 of the power in fp32, 5e-4 in fp16, per output row.  Then texture output with an
offset and clipping between guard bytes, repeatability, execute_iteration, and misuse that must be refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import fft_ref
from fft_ref import Case
from granite_amd import app as gapp
from granite_amd import capi, fft

pytestmark = pytest.mark.gpu
CASES = fft_ref.shape_cases()


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def executor(gr, per_iteration=False):
    def execute(options, dst, dst_layout, src, src_layout):
        d_src, d_dst = capi.DeviceBuffer(gr, src.nbytes).upload(src), capi.DeviceBuffer(gr, dst.nbytes).upload(dst)
        plan = fft.Plan(gr, options)
        try:
            r_dst = capi.fft_buffer_resource(d_dst.ptr, d_dst.nbytes, dst_layout.row_stride, dst_layout.layer_stride)
            r_src = capi.fft_buffer_resource(d_src.ptr, d_src.nbytes, src_layout.row_stride, src_layout.layer_stride)
            if per_iteration:
                for i in range(plan.iterations):
                    plan.execute(r_dst, r_src, iteration=i)
            else:
                plan.execute(r_dst, r_src)
            gr.sync()
            dst[:] = d_dst.download(dst.dtype)
            src[:] = d_src.download(src.dtype)
        finally:
            plan.close()
            d_src.free()
            d_dst.free()
    return execute


def cases_of(mode):
    picked = [c for c in CASES if c.mode == fft_ref.MODES[mode]]
    return pytest.mark.parametrize("case", picked, ids=[c.name for c in picked])


@cases_of("forward")
def test_forward_c2c(gr, case):
    fft_ref.check_case(executor(gr), case)


@cases_of("inverse")
def test_inverse_c2c(gr, case):
    fft_ref.check_case(executor(gr), case)


@cases_of("r2c")
def test_r2c(gr, case):
    fft_ref.check_case(executor(gr), case)


@cases_of("c2r")
def test_c2r(gr, case):
    fft_ref.check_case(executor(gr), case)


def run_bytes(gr, case, per_iteration, runs=1):
    rng = np.random.default_rng(11)
    src_layout, dst_layout = case.layouts()
    src = src_layout.store(fft_ref.quantised_input(rng, case.nz, case.ny, case.nx, case.mode, case.data_type))
    results = []
    for _ in range(runs):
        dst = dst_layout.poisoned()
        executor(gr, per_iteration)(case.options(), dst, dst_layout, src, src_layout)
        results.append(dst.tobytes())
    return results


@pytest.mark.parametrize("case", [Case("forward", 8192), Case("c2r", 64, 32, dimensions=2, data_type=capi.FFT_FP16), Case("r2c", 16, 8, 4, 3)],
                         ids=lambda c: c.name)
def test_execute_twice_and_by_iteration_give_identical_bytes(gr, case):
    first, second = run_bytes(gr, case, False, runs=2)
    assert first == second
    assert run_bytes(gr, case, True)[0] == first


def test_app_transform_round_trip(gr):
    x = np.random.default_rng(2).uniform(-1, 1, (3, 16, 32)).astype(np.float32)
    spectrum = fft.transform(gr, x, "r2c", dimensions=2)
    assert fft_ref.worst_row_ratio(spectrum.astype(np.complex128), np.fft.rfftn(x.astype(np.float64), axes=(-2, -1))) <= 1e-10
    back = fft.transform(gr, spectrum, "c2r", dimensions=2)
    assert fft_ref.worst_row_ratio(back.astype(np.float64), x.astype(np.float64) * (16 * 32)) <= 1e-10


@pytest.fixture(scope="module")
def application():
    a = gapp.Application(64, 64, lighting=False)
    yield a
    a.close()


def case_options(case):
    return (case.nx, case.ny, case.nz, case.dimensions, case.mode, case.data_type)


@pytest.mark.parametrize("image,offset", [((80, 70), (3, 2)), ((40, 30), (3, 2)), ((40, 30), (-5, -7))])
def test_c2r_fp16_into_r16_image_with_offset_and_clipping(application, image, offset):
    """Through gra_fft_transform and Granite::FFT: 64 x 64 into an image larger than the transform (the texels around the written
    rectangle keep their bytes) and into a smaller one (stores outside are dropped: the guard bytes on both sides of the image keep
    theirs)."""
    nx = ny = 64
    case = Case("c2r", nx, ny, dimensions=2, data_type=capi.FFT_FP16)
    x = fft_ref.quantised_input(np.random.default_rng(5), 1, ny, nx, case.mode, case.data_type)
    want = fft_ref.dft(x, case.mode, 2, nx)[0]
    src_layout, _ = case.layouts()
    src = src_layout.store(x)
    width, height = image
    guard = 256
    memory = np.full(guard + width * height + guard, 0x7EAD, np.uint16)
    application.fft(case_options(case), src, (src_layout.row_stride, src_layout.layer_stride), memory, image=(width, height, 2 * guard), output_offset=offset)
    assert np.all(memory[:guard] == 0x7EAD) and np.all(memory[guard + width * height:] == 0x7EAD)
    texels = memory[guard:guard + width * height].reshape(height, width)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    inside = (xs >= offset[0]) & (xs < offset[0] + nx) & (ys >= offset[1]) & (ys < offset[1] + ny)
    assert np.all(texels[~inside] == 0x7EAD)
    got = texels.view(np.float16).astype(np.float64)[inside]
    ref = want[ys[inside] - offset[1], xs[inside] - offset[0]]
    assert np.mean((got - ref) ** 2) <= 5e-4 * np.mean(ref ** 2)


@pytest.mark.parametrize("case", [Case("r2c", 16, 8, 3, 2, pad=True), Case("forward", 8192), Case("c2r", 16, 8, 4, 3, capi.FFT_FP16)], ids=lambda c: c.name)
def test_granite_fft_class_on_buffers(application, case):
    """Granite::FFT through gra_fft_transform on buffers, padded strides included: same bound, padding and source untouched."""
    def execute(options, dst, dst_layout, src, src_layout):
        application.fft(case_options(case), src, (src_layout.row_stride, src_layout.layer_stride), dst, (dst_layout.row_stride, dst_layout.layer_stride))
    fft_ref.check_case(execute, case)


def test_granite_fft_class_refuses(application):
    case = Case("forward", 16, 8, dimensions=2)
    src_layout, dst_layout = case.layouts()
    src, dst = src_layout.store(np.zeros((1, 8, 16), np.complex128)), dst_layout.poisoned()
    before = dst.tobytes()
    # a plan the library refuses; a destination too small for its strides; an image outside the output block
    with pytest.raises(RuntimeError):
        application.fft((12, 8, 1, 2, case.mode, case.data_type), src, (16, 128), dst, (16, 128))
    with pytest.raises(RuntimeError):
        application.fft(case_options(case), src, (16, 128), dst, (20, 160))
    with pytest.raises(RuntimeError):
        application.fft(case_options(case), src, (16, 128), dst, image=(16, 8, 64))
    assert dst.tobytes() == before


def test_c2c_into_rg32_image(gr):
    case = Case("forward", 16, 8, dimensions=2)
    x = fft_ref.quantised_input(np.random.default_rng(6), 1, 8, 16, case.mode, case.data_type)
    src_layout, _ = case.layouts()
    src = src_layout.store(x)
    d_src = capi.DeviceBuffer(gr, src.nbytes).upload(src)
    out = capi.DeviceImage(gr, 16, 8, capi.FORMAT_R32G32_SFLOAT)
    plan = fft.Plan(gr, case.options(output_resource=capi.FFT_RESOURCE_TEXTURE))
    try:
        plan.execute(capi.fft_image_resource(out.desc), capi.fft_buffer_resource(d_src.ptr, d_src.nbytes, 16, 128))
        gr.sync()
        got = out.download().view(np.float32).reshape(8, 16, 2).astype(np.float64)
    finally:
        plan.close()
        d_src.free()
    assert fft_ref.worst_row_ratio(got[..., 0] + 1j * got[..., 1], fft_ref.dft(x, case.mode, 2, 16)[0]) <= 1e-10


def test_misuse_is_refused_and_nothing_is_launched(gr):
    nx, ny = 16, 8
    poison = np.full(4096, 0x7EAD, np.uint16)

    def refused(options, make):
        """make(src buffer, dst buffer) -> (dst resource, src resource); the destination keeps its poison."""
        d_src, d_dst = capi.DeviceBuffer(gr, poison.nbytes).upload(poison), capi.DeviceBuffer(gr, poison.nbytes).upload(poison)
        plan = fft.Plan(gr, options)
        try:
            dst, src = make(d_src, d_dst)
            with pytest.raises(capi.GraniteHipError):
                plan.execute(dst, src)
            gr.sync()
            assert np.all(d_dst.download(np.uint16) == 0x7EAD) and np.all(d_src.download(np.uint16) == 0x7EAD)
        finally:
            plan.close()
            d_src.free()
            d_dst.free()

    c2c = capi.fft_options(nx, ny, 1, 2)
    full = nx * ny * 8
    refused(c2c, lambda s, d: (capi.fft_buffer_resource(None, full, nx, nx * ny), capi.fft_buffer_resource(s.ptr, full, nx, nx * ny)))
    refused(c2c, lambda s, d: (capi.fft_buffer_resource(d.ptr, full, nx, nx * ny), capi.fft_buffer_resource(None, full, nx, nx * ny)))
    # a byte size too small for the strides, on either side
    refused(c2c, lambda s, d: (capi.fft_buffer_resource(d.ptr, full, nx + 2, 0), capi.fft_buffer_resource(s.ptr, full, nx, nx * ny)))
    refused(c2c, lambda s, d: (capi.fft_buffer_resource(d.ptr, full, nx, nx * ny), capi.fft_buffer_resource(s.ptr, full - 8, nx, nx * ny)))
    # a row stride below the row
    refused(c2c, lambda s, d: (capi.fft_buffer_resource(d.ptr, full, nx - 1, 0), capi.fft_buffer_resource(s.ptr, full, nx, nx * ny)))
    # an odd stride on an fp16 real side
    r2c16 = capi.fft_options(nx, ny, 1, 1, capi.FFT_R2C, capi.FFT_FP16)
    refused(r2c16, lambda s, d: (capi.fft_buffer_resource(d.ptr, d.nbytes, nx // 2 + 1, 0), capi.fft_buffer_resource(s.ptr, s.nbytes, nx + 1, 0)))
    c2r16 = capi.fft_options(nx, ny, 1, 1, capi.FFT_C2R, capi.FFT_FP16)
    refused(c2r16, lambda s, d: (capi.fft_buffer_resource(d.ptr, d.nbytes, nx + 1, 0), capi.fft_buffer_resource(s.ptr, s.nbytes, nx // 2 + 1, 0)))
    # overlapping ranges: in place, and a destination that starts inside the source
    refused(c2c, lambda s, d: (capi.fft_buffer_resource(d.ptr, full, nx, nx * ny), capi.fft_buffer_resource(d.ptr, full, nx, nx * ny)))
    refused(c2c, lambda s, d: (capi.fft_buffer_resource(d.ptr + full - 64, full, nx, nx * ny), capi.fft_buffer_resource(d.ptr, full, nx, nx * ny)))
    # a resource of the other type, and an image of the wrong format
    refused(c2c, lambda s, d: (capi.fft_image_resource(capi.Image(d.ptr, nx, ny, nx * 8, capi.FORMAT_R32G32_SFLOAT)),
                               capi.fft_buffer_resource(s.ptr, full, nx, nx * ny)))
    tex = capi.fft_options(nx, ny, 1, 2, output_resource=capi.FFT_RESOURCE_TEXTURE)
    refused(tex, lambda s, d: (capi.fft_image_resource(capi.Image(d.ptr, nx, ny, nx * 4, capi.FORMAT_R16G16_SFLOAT)),
                               capi.fft_buffer_resource(s.ptr, full, nx, nx * ny)))
    # options the plan refuses
    for bad in (capi.fft_options(12), capi.fft_options(4, mode=capi.FFT_R2C), capi.fft_options(16, 16, 1, 2, input_resource=capi.FFT_RESOURCE_TEXTURE),
                capi.fft_options(16, 16, 2, 2, output_resource=capi.FFT_RESOURCE_TEXTURE)):
        with pytest.raises(capi.GraniteHipError):
            fft.Plan(gr, bad)
