"""FFT on numpy arrays: upload, plan, execute, download (gr_fft_* of include/granite_hip.h).

    spectrum = fft.transform(ctx, field, "r2c", dimensions=2)            # (ny, nx) float32 -> (ny, nx / 2 + 1) complex64
    heights = fft.transform(ctx, spectrum, "c2r", dimensions=2, fp16=True)

Nothing is normalised: inverse of forward gives N x.  A leading axis beyond `dimensions` is a batch."""
from typing import Optional

import numpy as np

from . import capi

MODES = {"forward": capi.FFT_FORWARD_C2C, "inverse": capi.FFT_INVERSE_C2C, "r2c": capi.FFT_R2C, "c2r": capi.FFT_C2R}


class Plan:
    """gr_fft_plan with its options.  A plan owns its scratch and twiddles and may be in flight on one stream at a time."""

    def __init__(self, ctx: capi.Context, options: capi.FftOptions):
        self.ctx, self.options = ctx, options
        self.handle = ctx.fft_plan(options)
        self.iterations = int(ctx.lib.gr_fft_plan_iterations(self.handle))

    def execute(self, dst: capi.FftResource, src: capi.FftResource, stream=None, iteration: Optional[int] = None):
        self.ctx.fft_execute(self.handle, dst, src, stream, iteration)

    def close(self):
        if self.handle is not None:
            self.ctx.fft_plan_destroy(self.handle)
            self.handle = None


def _split(array, fp16):
    """complex array -> interleaved (re, im) scalars of the memory type."""
    scalar = np.float16 if fp16 else np.float32
    out = np.empty(array.shape + (2,), scalar)
    out[..., 0], out[..., 1] = array.real, array.imag
    return out


def transform(ctx: capi.Context, array: np.ndarray, mode: str, dimensions: int = 1, fp16: bool = False, stream=None) -> np.ndarray:
    """One transform of `array` over its last `dimensions` axes (up to three axes in all; the leading ones are batches).  "c2r" takes the
    nx / 2 + 1 columns numpy's rfft gives and returns nx = 2 (columns - 1) reals a row."""
    m = MODES[mode]
    a = np.asarray(array)
    assert 1 <= a.ndim <= 3 and 1 <= dimensions <= a.ndim
    shape = (1,) * (3 - a.ndim) + a.shape
    nz, ny, units = shape
    nx = 2 * (units - 1) if m == capi.FFT_C2R else units
    scalar = np.float16 if fp16 else np.float32
    host = a.astype(scalar) if m == capi.FFT_R2C else _split(a, fp16)
    out_units = nx if m == capi.FFT_C2R else (nx // 2 + 1 if m == capi.FFT_R2C else nx)
    out_scalars = nz * ny * out_units * (1 if m == capi.FFT_C2R else 2)
    plan = Plan(ctx, capi.fft_options(nx, ny, nz, dimensions, m, capi.FFT_FP16 if fp16 else capi.FFT_FP32))
    src = capi.DeviceBuffer(ctx, host.nbytes).upload(host)
    dst = capi.DeviceBuffer(ctx, out_scalars * np.dtype(scalar).itemsize)
    try:
        plan.execute(capi.fft_buffer_resource(dst.ptr, dst.nbytes, out_units, out_units * ny), capi.fft_buffer_resource(src.ptr, src.nbytes, units, units * ny),
                     stream)
        ctx.sync(stream)
        raw = dst.download(scalar)
    finally:
        plan.close()
        src.free()
        dst.free()
    if m == capi.FFT_C2R:
        return raw.reshape(a.shape[:-1] + (nx,))
    pairs = raw.reshape(a.shape[:-1] + (out_units, 2)).astype(np.float32)
    return (pairs[..., 0] + 1j * pairs[..., 1]).astype(np.complex64)
