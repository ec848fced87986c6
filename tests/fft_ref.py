"""The yardstick of the FFT tests: numpy's float64 DFT (fft, ifft * N, rfft, irfft * N and their n-dimensional forms) applied to the inputs
as stored, i.e. after quantising to fp32 or fp16, and the criterion of the reference's own test (renderer/fft/test/fft_test.cpp:56-125):
per output row, over the columns that carry information,

    mean squared error <= 1e-10 * mean power (fp32),   <= 5e-4 * mean power (fp16),   NaN fails.

Also the buffer layouts (strides in elements, poisoned padding) and the list of shapes the CPU emulation and the GPU are both held to."""
import ctypes as C

import numpy as np

from granite_amd import capi

BOUND = {capi.FFT_FP32: 1e-10, capi.FFT_FP16: 5e-4}
MODES = {"forward": capi.FFT_FORWARD_C2C, "inverse": capi.FFT_INVERSE_C2C, "r2c": capi.FFT_R2C, "c2r": capi.FFT_C2R}
POISON = {np.dtype(np.float32): 0x7FC0BEEF, np.dtype(np.float16): 0x7EAD}


def scalar_type(data_type):
    return np.dtype(np.float16 if data_type == capi.FFT_FP16 else np.float32)


def real_side(mode, output):
    return mode == (capi.FFT_C2R if output else capi.FFT_R2C)


def row_units(nx, mode, output):
    """Elements of a row the transform touches: scalars on a real side, nx / 2 + 1 complex numbers opposite it, else nx."""
    if real_side(mode, output):
        return nx
    return nx // 2 + 1 if mode in (capi.FFT_R2C, capi.FFT_C2R) else nx


class Layout:
    """A buffer side: logical shape (nz, ny, row units), strides in elements, scalars or complex pairs of `dtype`."""

    def __init__(self, nz, ny, units, real, dtype, row_stride=None, layer_stride=None):
        self.nz, self.ny, self.units, self.real, self.dtype = nz, ny, units, real, np.dtype(dtype)
        self.row_stride = units if row_stride is None else row_stride
        self.layer_stride = self.row_stride * ny if layer_stride is None else layer_stride
        self.per = 1 if real else 2
        self.elements = (nz - 1) * self.layer_stride + (ny - 1) * self.row_stride + units
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(units), indexing="ij")
        self.index = z * self.layer_stride + y * self.row_stride + x

    @property
    def nbytes(self):
        return self.elements * self.per * self.dtype.itemsize

    def poisoned(self):
        bits = np.full(self.elements * self.per, POISON[self.dtype], np.uint32 if self.dtype.itemsize == 4 else np.uint16)
        return bits.view(self.dtype)

    def store(self, logical):
        """The buffer holding `logical` (float64 / complex128, shape nz x ny x units), padding poisoned."""
        buf = self.poisoned()
        if self.real:
            buf[self.index] = logical.astype(self.dtype)
        else:
            buf[2 * self.index] = logical.real.astype(self.dtype)
            buf[2 * self.index + 1] = logical.imag.astype(self.dtype)
        return buf

    def load(self, buf):
        buf = buf.view(self.dtype)
        if self.real:
            return buf[self.index].astype(np.float64)
        return buf[2 * self.index].astype(np.float64) + 1j * buf[2 * self.index + 1].astype(np.float64)

    def padding_untouched(self, buf):
        mask = np.ones(self.elements * self.per, bool)
        for k in range(self.per):
            mask[self.per * self.index + k] = False
        raw = buf.view(np.uint32 if self.dtype.itemsize == 4 else np.uint16)
        return bool(np.all(raw[mask] == POISON[self.dtype]))


def quantised_input(rng, nz, ny, nx, mode, data_type):
    """Uniform in (-1, 1) as the reference's test draws it, rounded to the memory type; a C2R input has real DC and Nyquist columns."""
    dtype = scalar_type(data_type)
    if mode == capi.FFT_R2C:
        return rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(dtype).astype(np.float64)
    cols = row_units(nx, mode, False)
    x = rng.uniform(-1.0, 1.0, (nz, ny, cols)).astype(dtype).astype(np.float64) + 1j * rng.uniform(-1.0, 1.0, (nz, ny, cols)).astype(dtype).astype(np.float64)
    if mode == capi.FFT_C2R:
        x[..., 0] = x[..., 0].real
        x[..., nx // 2] = x[..., nx // 2].real
    return x


def dft(x, mode, dimensions, nx):
    """float64: x is (nz, ny, row units); the last `dimensions` axes are transformed, nothing is normalised."""
    axes = tuple(range(-dimensions, 0))
    shape = x.shape[:2] + (nx,)
    count = int(np.prod([shape[a] for a in axes]))
    if mode == capi.FFT_FORWARD_C2C:
        return np.fft.fftn(x, axes=axes)
    if mode == capi.FFT_INVERSE_C2C:
        return np.fft.ifftn(x, axes=axes) * count
    if mode == capi.FFT_R2C:
        return np.fft.rfftn(x, axes=axes)
    return np.fft.irfftn(x, s=[shape[a] for a in axes], axes=axes) * count


def worst_row_ratio(got, want):
    """max over rows of (mean squared error / mean power); inf when anything is NaN.  Rows without power must be exact."""
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    if np.isnan(got.view(np.float64)).any():
        return np.inf
    error = np.mean(np.abs(got - want) ** 2, axis=1)
    power = np.mean(np.abs(want) ** 2, axis=1)
    ratio = np.where(power > 0, error / np.where(power > 0, power, 1.0), np.where(error > 0, np.inf, 0.0))
    return float(ratio.max())


class Case:
    def __init__(self, mode, nx, ny=1, nz=1, dimensions=1, data_type=capi.FFT_FP32, pad=False):
        self.mode, self.nx, self.ny, self.nz, self.dimensions, self.data_type, self.pad = MODES[mode], nx, ny, nz, dimensions, data_type, pad
        self.name = f"{mode}-{nx}x{ny}x{nz}-{dimensions}d-{'fp16' if data_type else 'fp32'}{'-padded' if pad else ''}"

    def options(self, output_resource=capi.FFT_RESOURCE_BUFFER):
        return capi.fft_options(self.nx, self.ny, self.nz, self.dimensions, self.mode, self.data_type, output_resource=output_resource)

    def layouts(self):
        dtype = scalar_type(self.data_type)
        sides = []
        for output in (False, True):
            units, real = row_units(self.nx, self.mode, output), real_side(self.mode, output)
            if self.pad:  # even, so that an fp16 real side is legal; different on the two sides
                row = units + (6 if output else 2)
                sides.append(Layout(self.nz, self.ny, units, real, dtype, row, row * self.ny + (4 if output else 10)))
            else:
                sides.append(Layout(self.nz, self.ny, units, real, dtype))
        return sides


def first_length_with_passes(passes, mode, data_type, limit=1 << 20):
    """The smallest 1-D length gr_fft_describe plans as `passes` C2C passes, or None up to `limit`."""
    n = 8
    while n <= limit:
        listed = capi.fft_describe(capi.fft_options(n, mode=MODES[mode], data_type=data_type))
        if listed is not None and sum(1 for p in listed if p.kind == capi.FFT_PASS_C2C) == passes:
            return n
        n *= 2
    return None


def shape_cases():
    """The shapes of the issue: the smallest at which a pass boundary, a tile edge or a resolve can go wrong."""
    cases = []
    for data_type in (capi.FFT_FP32, capi.FFT_FP16):
        for mode in ("forward", "inverse"):
            lengths = [4, 8, 16, 32, 64, 512] + [n for n in (first_length_with_passes(k, mode, data_type) for k in (2, 3)) if n]
            cases += [Case(mode, n, data_type=data_type) for n in lengths]
        for mode in ("r2c", "c2r"):
            for n in (8, 16, 1024, first_length_with_passes(2, mode, data_type)):
                cases += [Case(mode, n, ny=batch, data_type=data_type) for batch in (1, 15, 16)]
        for mode in ("forward", "inverse", "r2c", "c2r"):
            # a real Nx of 4 is refused: the real modes start at 8 x 4
            shapes = [(8, 4), (8, 8), (64, 32)] if mode in ("r2c", "c2r") else [(4, 4), (8, 4), (4, 8), (64, 32)]
            cases += [Case(mode, nx, ny, dimensions=2, data_type=data_type) for nx, ny in shapes]
            cases += [Case(mode, nx, ny, nz, 3, data_type) for nx, ny, nz in ((4 if mode in ("forward", "inverse") else 8, 4, 4), (16, 8, 4))]
            cases.append(Case(mode, 16, 8, 3, 2, data_type))
            cases.append(Case(mode, 16, 8, 3, 2, data_type, pad=True))
            cases.append(Case(mode, 64, 5, 1, 1, data_type, pad=True))
    return cases


def check_case(execute, case, seed=7):
    """execute(options, dst buffer, dst layout, src buffer, src layout) fills dst.  Returns the worst row ratio after asserting the bound
    and that the padding of the destination and the whole source are byte-identical afterwards."""
    rng = np.random.default_rng(seed)
    src_layout, dst_layout = case.layouts()
    x = quantised_input(rng, case.nz, case.ny, case.nx, case.mode, case.data_type)
    src, dst = src_layout.store(x), dst_layout.poisoned()
    before = src.copy()
    execute(case.options(), dst, dst_layout, src, src_layout)
    assert src.tobytes() == before.tobytes(), f"{case.name}: the source was written"
    assert dst_layout.padding_untouched(dst), f"{case.name}: padding of the destination was written"
    ratio = worst_row_ratio(dst_layout.load(dst), dft(x, case.mode, case.dimensions, case.nx))
    print(f"{case.name}: worst row mse / power = {ratio:.3e} (bound {BOUND[case.data_type]:.0e})")
    assert ratio <= BOUND[case.data_type], f"{case.name}: mse / power {ratio:.3e} above {BOUND[case.data_type]:.0e}"
    return ratio


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
