"""CPU: granite_amd/csrc/fft_core.hpp built for the host (tests/cpp/fft_core_host.cpp), running the plan the host code makes pass by pass and
lane by lane as the kernels of fft.hip do, held to numpy's float64 DFT under the bounds of tests/fft_ref.py (1e-10 of the power in fp32,
5e-4 in fp16, per output row), plus exact probes and the image store's clipping."""
import ctypes as C
import numpy as np
import pytest

import fft_ref
from fft_ref import Case, ptr
from granite_amd import capi
from host_program import build_library

CASES = fft_ref.shape_cases()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    # -O2: the cases run every pass lane by lane, and the suite's time is this library's speed
    return C.CDLL(build_library(tmp_path_factory.mktemp("fft_core"), "libfft_core_host.so", "fft_core_host.cpp", extra=["-O2"]))


def executor(host):
    def execute(options, dst, dst_layout, src, src_layout):
        n = host.fft_host_execute(C.byref(options), ptr(dst), dst_layout.row_stride, dst_layout.layer_stride, ptr(src), src_layout.row_stride,
                                  src_layout.layer_stride, None)
        assert n > 0, "the plan was refused"
    return execute


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_shapes_against_float64_dft(host, case):
    fft_ref.check_case(executor(host), case)


def run(host, case, x):
    src_layout, dst_layout = case.layouts()
    src, dst = src_layout.store(x), dst_layout.poisoned()
    executor(host)(case.options(), dst, dst_layout, src, src_layout)
    return dst_layout.load(dst)


@pytest.mark.parametrize("mode", ["forward", "r2c"])
@pytest.mark.parametrize("n", [8, 16, 64, 8192, 16384])
def test_unit_impulse_gives_all_ones(host, mode, n):
    x = np.zeros((1, 1, n), np.float64 if mode == "r2c" else np.complex128)
    x[0, 0, 0] = 1.0
    got = run(host, Case(mode, n), x)
    assert np.array_equal(got, np.ones_like(got))


@pytest.mark.parametrize("n", [4, 8, 16, 32, 64])
def test_constant_gives_n_in_bin_zero_and_exact_zeros(host, n):
    got = run(host, Case("forward", n), np.ones((1, 1, n), np.complex128))
    want = np.zeros(n, np.complex128)
    want[0] = n
    assert np.array_equal(got[0, 0], want)


@pytest.mark.parametrize("data_type", [capi.FFT_FP32, capi.FFT_FP16])
@pytest.mark.parametrize("shape", [(64, 1, 1), (8192, 1, 1), (16, 8, 2)])
def test_inverse_of_forward_is_n_times_input(host, shape, data_type):
    nx, ny, dims = shape
    x = fft_ref.quantised_input(np.random.default_rng(3), 1, ny, nx, capi.FFT_FORWARD_C2C, data_type)
    # fp16: scaled so that the spectrum and N x stay far inside the half range
    scale = 1.0 / 64.0 if data_type == capi.FFT_FP16 else 1.0
    x = (x * scale).astype(np.complex64).astype(np.complex128) if data_type == capi.FFT_FP32 else \
        (x.real * scale).astype(np.float16).astype(np.float64) + 1j * (x.imag * scale).astype(np.float16).astype(np.float64)
    forward = run(host, Case("forward", nx, ny, dimensions=dims, data_type=data_type), x)
    back = run(host, Case("inverse", nx, ny, dimensions=dims, data_type=data_type), forward)
    ratio = fft_ref.worst_row_ratio(back, x * (nx * (ny if dims == 2 else 1)))
    assert ratio <= fft_ref.BOUND[data_type], ratio


@pytest.mark.parametrize("image,offset", [((80, 70), (3, 2)), ((40, 30), (3, 2)), ((40, 30), (-5, -7))])
def test_c2r_image_store_clips_and_leaves_the_rest(host, image, offset):
    """2-D C2R fp16 64 x 64 into an R16 image: texels outside the written rectangle keep their bytes, stores outside the image are dropped
    (the image lies between guard bytes)."""
    nx = ny = 64
    case = Case("c2r", nx, ny, dimensions=2, data_type=capi.FFT_FP16)
    x = fft_ref.quantised_input(np.random.default_rng(5), 1, ny, nx, case.mode, case.data_type)
    want = fft_ref.dft(x, case.mode, 2, nx)[0]
    src_layout, _ = case.layouts()
    src = src_layout.store(x)
    width, height = image
    guard = 256
    memory = np.full(guard + width * height + guard, 0x7EAD, np.uint16)
    desc = (C.c_int32 * 5)(width, height, width * 2, offset[0], offset[1])
    options = case.options(output_resource=capi.FFT_RESOURCE_TEXTURE)
    assert host.fft_host_execute(C.byref(options), ptr(memory[guard:]), 0, 0, ptr(src), src_layout.row_stride, src_layout.layer_stride, desc) > 0
    assert np.all(memory[:guard] == 0x7EAD) and np.all(memory[guard + width * height:] == 0x7EAD)
    texels = memory[guard:guard + width * height].reshape(height, width)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    inside = (xs >= offset[0]) & (xs < offset[0] + nx) & (ys >= offset[1]) & (ys < offset[1] + ny)
    assert np.all(texels[~inside] == 0x7EAD)
    got = texels.view(np.float16).astype(np.float64)[inside]
    ref = want[ys[inside] - offset[1], xs[inside] - offset[0]]
    assert np.mean((got - ref) ** 2) <= 5e-4 * np.mean(ref ** 2)
