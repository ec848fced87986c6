"""GPU: gr_video_yuv_to_rgb (init_yuv_to_rgb / dispatch_conversion + yuv_to_rgb.comp) through the C ABI against tests/yuv_ref.py.

Bounds, per channel:
  * R8G8B8A8: 1 code.  yuv_ref evaluates the shader's expression in float64, the kernel in fp32; a difference of 1e-6 can still fall
    on either side of a rounding midpoint.
  * A2B10G10R10: 1 of 1023, for the same reason.
  * R16G16B16A16_SFLOAT (PQ): the project's standing 2 fp16 ulp + 1e-4 (tests/util.py) plus yuv_ref.pq_fp32_allowance, a first-order
    bound on the error of any fp32 evaluation of the PQ branch.  Reason and figures: before the bound was fixed, yuv_ref was evaluated
    once in float32 (every operation rounded, pow as exp2(y * log2 x), GLSL's definition) against float64 on the PQ inputs of this
    file, on the CPU.  That alone left the standing bound: up to 37.1 times the bound at 4K P010 / BT.2020 (11009 of 33 million
    channels), 31.0 times for yuv444p16 / BT.2020, 2.7 times for BT.601-625; none for BT.709 or gray, where primary_conversion is the
    identity or r = g = b.  Every such channel is one where the terms of primary_conversion cancel (a saturated colour outside the
    BT.709 gamut: terms of up to 200, a result near 0, so an error of 1e-5 relative to the terms is many fp16 ulps of the result).  So
    the standing bound is wrong for fp32 there, not the kernel, and it is widened by exactly that mechanism instead of by a flat
    factor: the allowance follows one fp32 ulp (2^-23) per operation through the EOTF's two pow calls -- x^(1/78.84) lands in
    [0.84, 1], subtracting c1 = 0.8359 cancels most of it, the second pow multiplies the relative error by 6.28 -- and sums
    |coefficient| x error over the conversion's terms.  It is at most 5.3e-2 (at values of 100 to 200, where 2 fp16 ulp are 0.125 to
    0.25) and vanishes with the value.  The float32 evaluation uses at most 0.29 of the allowance where it needs any, and 0.47 of the
    whole bound everywhere.

yuv_ref's chroma fetch is the project's sampler model; the 16-bit fetch is v / 65535 (the executed-shader golden of
tests/test_yuv_ref_cpu.py covers 8-bit planes only).  Every output lies in a buffer with a padded row pitch and guards before, between
and after its rows: no byte outside the image's extent may change, and a refused call changes none at all.
"""
import ctypes as C

import numpy as np
import pytest

import yuv_ref as yr
from granite_amd import capi
from util import rgba16f_mismatch, ulp_fp16
from video_planes import EDGE_SIZES, GuardedImage

pytestmark = pytest.mark.gpu

# name -> (number of planes, 16-bit planes, 4:2:0)
LAYOUTS = {
    "gray": (1, False, False), "gray16": (1, True, False),
    "nv12": (2, False, True), "yuv420p": (3, False, True), "yuv444p": (3, False, False),
    "p010": (2, True, True), "yuv420p16": (3, True, True), "yuv444p16": (3, True, False),
}


def make_planes(layout, w, h, seed, bits=None):
    """Random stored planes with a smooth band on top (ramps: the chroma filter between neighbouring values, not only noise).  bits:
    significant bits of a 16-bit sample: 16, (10, 'msb') for P010's high bits, (10, 'lsb') for a software decoder's low bits."""
    n, wide, sub = LAYOUTS[layout]
    rng = np.random.default_rng(seed)
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub else (w, h)
    top = 65536 if wide else 256

    def plane(pw, ph, channels, phase):
        shape = (ph, pw, channels) if channels > 1 else (ph, pw)
        v = rng.integers(0, top, shape, dtype=np.int64)
        band = max(1, ph // 4)
        ramp = (np.arange(pw)[None, :] * (top - 1) // max(1, pw - 1) + phase * top // 3) % top
        v[:band] = ramp[..., None] if channels > 1 else ramp
        if wide and bits and bits[0] == 10:
            v = (v >> 6) << 6 if bits[1] == "msb" else v >> 6
        return v.astype(np.uint16 if wide else np.uint8)

    planes = [plane(w, h, 1, 0)]
    if n == 2:
        planes.append(plane(cw, ch, 2, 1))
    elif n == 3:
        planes += [plane(cw, ch, 1, 1), plane(cw, ch, 1, 2)]
    return planes


def plane_format(p):
    return {(1, 2): yr.R8, (2, 2): yr.R16, (1, 3): yr.R8G8, (2, 3): yr.R16G16}[(p.dtype.itemsize, p.ndim)]


def upload_planes(gr, planes, offset=0, pad=None):
    return [GuardedImage(gr, p.shape[1], p.shape[0], plane_format(p), p, offset, pad) for p in planes]


def compare(got_rows, ref, out_fmt, w, h, what="", allowance=None):
    """Print the worst figure, then hold it to the bound.  allowance: yuv_ref.pq_fp32_allowance of the case (RGBA16F only)."""
    if out_fmt == yr.RGBA16F:
        got = got_rows.view(np.uint16).reshape(h, w, 4)
        a, b = got.view(np.float16).astype(np.float64), ref.view(np.float16).astype(np.float64)
        tol = 2.0 * ulp_fp16(np.maximum(np.abs(a), np.abs(b))) + 1e-4
        tol[..., :3] += allowance
        with np.errstate(invalid="ignore"):
            bad = ~(np.abs(a - b) <= tol)
        standing = rgba16f_mismatch(got, ref, 2.0, 1e-4)
        print(f"{what}: worst share of the bound {np.nanmax(np.abs(a - b) / tol):.3f}; {int(standing.sum())} channels beyond 2 fp16 ulp + 1e-4 alone")
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} channels beyond the bound; first at {tuple(np.argwhere(bad)[0])}: {a[tuple(np.argwhere(bad)[0])]} vs {b[tuple(np.argwhere(bad)[0])]}"
        return
    got = yr.unpack_a2b10g10r10(got_rows.view(np.uint32).reshape(h, w)) if out_fmt == yr.A2B10G10R10 else got_rows.reshape(h, w, 4).astype(np.int64)
    err = np.abs(got - ref)
    print(f"{what}: worst {err.max()} code(s), {float((err == 0).mean()) * 100:.3f} % exact")
    assert (got[..., 3] == ref[..., 3]).all(), f"{what}: alpha is not 1"
    assert err.max() <= 1, f"{what}: {int((err > 1).sum())} channels beyond 1 code, worst {err.max()} at {tuple(np.argwhere(err > 1)[0])}"


def run_case(gr, layout, size, out_fmt, inf, seed=1, bits=None, offset=0, pad=None, out_offset=0, out_pad=None):
    w, h = size
    planes = make_planes(layout, w, h, seed, bits)
    src = upload_planes(gr, planes, offset, pad)
    out = GuardedImage(gr, w, h, out_fmt, None, out_offset, out_pad)
    gr.video_yuv_to_rgb([s.desc for s in src], out.desc, capi.video_yuv_info(**inf))
    gr.sync()
    p = yr.plan([(q.shape[1], q.shape[0], plane_format(q)) for q in planes], (w, h, out_fmt), yr.info(**inf))
    ref = yr.store(yr.shade(planes, p), out_fmt)
    allowance = yr.pq_fp32_allowance(planes, p) if out_fmt == yr.RGBA16F else None
    compare(out.read(), ref, out_fmt, w, h, f"{layout} {w}x{h} -> {out_fmt}", allowance)


def stream_info(layout, **kw):
    inf = dict(bit_depth=16 if LAYOUTS[layout][1] else 8, full_range=1)
    inf.update(kw)
    return inf


# ---- every layout recording can emit, plus gray, at 4K and at an odd size ---------------------------------------------------------
@pytest.mark.parametrize("layout", ["nv12", "yuv420p", "yuv444p", "p010", "yuv420p16", "yuv444p16", "gray"])
def test_recorded_layouts_odd_size(gr, layout):
    run_case(gr, layout, (1277, 719), yr.RGBA8, stream_info(layout))


@pytest.mark.parametrize("layout,out_fmt,kw", [("nv12", yr.RGBA8, {}), ("yuv420p", yr.RGBA8_SRGB, dict(full_range=0, matrix=yr.M_UNSPECIFIED)),
                                               ("p010", yr.RGBA16F, dict(pq=1, matrix=yr.M_BT2020)),
                                               ("p010", yr.A2B10G10R10, dict(pq=1, matrix=yr.M_BT2020, full_range=0))],
                         ids=["nv12", "yuv420p_limited", "p010_pq_rgba16f", "p010_pq_a2b10g10r10"])
def test_4k(gr, layout, out_fmt, kw):
    run_case(gr, layout, (3840, 2160), out_fmt, stream_info(layout, **kw))


# ---- stream descriptions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("location", range(6))
@pytest.mark.parametrize("layout", ["nv12", "yuv444p"])
def test_sitings(gr, layout, location):
    run_case(gr, layout, (333, 127), yr.RGBA8, stream_info(layout, chroma_location=location, full_range=0), seed=3 + location)


@pytest.mark.parametrize("matrix", range(6))
@pytest.mark.parametrize("full_range", [0, 1])
def test_matrices_and_ranges(gr, matrix, full_range):
    run_case(gr, "yuv420p", (322, 242), yr.RGBA8, stream_info("yuv420p", matrix=matrix, full_range=full_range), seed=11)


def test_nv21_swaps_the_chroma_channels(gr):
    run_case(gr, "nv12", (641, 361), yr.RGBA8, stream_info("nv12", nv21=1, full_range=0), seed=5)


def test_p010_msb_aligned(gr):
    run_case(gr, "p010", (641, 361), yr.RGBA8, stream_info("p010", bit_depth=10, msb_aligned=1, full_range=0), seed=6, bits=(10, "msb"))


def test_yuv420p10_low_bits(gr):
    run_case(gr, "yuv420p16", (641, 361), yr.RGBA8, stream_info("yuv420p16", bit_depth=10, msb_aligned=0, full_range=0), seed=7, bits=(10, "lsb"))


@pytest.mark.parametrize("matrix", [yr.M_BT2020, yr.M_BT601_625, yr.M_BT709])
@pytest.mark.parametrize("layout,bits,kw", [("p010", (10, "msb"), dict(bit_depth=10, msb_aligned=1)), ("yuv444p16", None, {}), ("gray16", None, {})],
                         ids=["p010", "yuv444p16", "gray16"])
def test_pq_into_rgba16f(gr, layout, bits, kw, matrix):
    run_case(gr, layout, (1277, 719), yr.RGBA16F, stream_info(layout, pq=1, matrix=matrix, full_range=0, **kw), seed=8, bits=bits)


@pytest.mark.parametrize("layout,bits,kw", [("p010", (10, "msb"), dict(bit_depth=10, msb_aligned=1)), ("yuv420p16", None, {})], ids=["p010", "yuv420p16"])
def test_pq_left_encoded_into_a2b10g10r10(gr, layout, bits, kw):
    run_case(gr, layout, (1277, 719), yr.A2B10G10R10, stream_info(layout, pq=1, matrix=yr.M_BT2020, full_range=0, **kw), seed=9, bits=bits)


# ---- shapes and placement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", EDGE_SIZES, ids=[f"{w}x{h}" for w, h in EDGE_SIZES])
@pytest.mark.parametrize("layout,out_fmt,kw", [("nv12", yr.RGBA8, {}), ("yuv420p", yr.RGBA8, dict(chroma_location=yr.C_TOPLEFT)), ("yuv444p", yr.RGBA8, {}),
                                               ("gray", yr.RGBA8, {}), ("p010", yr.RGBA16F, dict(pq=1, matrix=yr.M_BT2020))],
                         ids=["nv12", "yuv420p", "yuv444p", "gray", "p010_pq"])
def test_edge_sizes(gr, size, layout, out_fmt, kw):
    run_case(gr, layout, size, out_fmt, stream_info(layout, **kw), seed=20)


@pytest.mark.parametrize("layout,out_fmt,kw", [("nv12", yr.RGBA8, {}), ("yuv420p", yr.RGBA8, {}), ("yuv444p16", yr.RGBA8, {}),
                                               ("p010", yr.RGBA16F, dict(pq=1, matrix=yr.M_BT2020)), ("p010", yr.A2B10G10R10, dict(pq=1))],
                         ids=["nv12", "yuv420p", "yuv444p16", "p010_pq_rgba16f", "p010_a2b10g10r10"])
@pytest.mark.parametrize("where", ["planes", "output", "both"])
def test_unaligned(gr, layout, out_fmt, kw, where):
    # pointers 4 bytes into their buffers and pitches of row + 4: vector loads / stores are off on that side
    src = dict(offset=4, pad=4) if where != "output" else {}
    dst = dict(out_offset=4, out_pad=4) if where != "planes" else {}
    run_case(gr, layout, (1277, 719), out_fmt, stream_info(layout, **kw), seed=30, **src, **dst)


# ---- exact probes, as in tests/test_yuv_ref_cpu.py ---------------------------------------------------------------------------------
def test_dither_probe_exact(gr):
    plane, c8, c10 = yr.dither_probe()
    h, w = plane.shape
    for out_fmt, want, pq in ((yr.RGBA8, c8, 0), (yr.A2B10G10R10, c10, 1)):
        src = upload_planes(gr, [plane])
        out = GuardedImage(gr, w, h, out_fmt)
        gr.video_yuv_to_rgb([src[0].desc], out.desc, capi.video_yuv_info(full_range=0, pq=pq))
        gr.sync()
        rows = out.read()
        got = yr.unpack_a2b10g10r10(rows.view(np.uint32).reshape(h, w)) if pq else rows.reshape(h, w, 4).astype(np.int64)
        assert (got == want).all(), f"{int((got != want).sum())} channels differ from the dither table's codes"


@pytest.mark.parametrize("location", range(6))
@pytest.mark.parametrize("sub", [True, False], ids=["420", "444"])
@pytest.mark.parametrize("size", [(67, 35), (34, 18)], ids=["67x35", "34x18"])
def test_coordinate_probe(gr, size, sub, location):
    """Chroma texels encode their own coordinates (tests/test_yuv_ref_cpu.py holds yuv_ref's taps to the exact positions).  Full range
    BT.709: b = y + 1.8556 (cb - 128 / 255), r = y + 1.5748 (cr - 128 / 255), and neighbouring texels differ by PROBE_STEP codes, so a
    tap off by one texel, or a clamp that does not bite, moves a stored code by 4 or more where the channel is not saturated: the
    1-code bound against yuv_ref decides."""
    w, h = size
    planes, _, _ = yr.coordinate_probe(w, h, sub, location)
    src = upload_planes(gr, planes)
    out = GuardedImage(gr, w, h, yr.RGBA8)
    inf = dict(full_range=1, chroma_location=location)
    gr.video_yuv_to_rgb([s.desc for s in src], out.desc, capi.video_yuv_info(**inf))
    gr.sync()
    compare(out.read(), yr.yuv_to_rgb(planes, yr.RGBA8, yr.info(**inf)), yr.RGBA8, w, h, f"coordinate probe {w}x{h}")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(gr):
    w, h = 64, 32
    planes = make_planes("nv12", w, h, 1)
    src = upload_planes(gr, planes)
    wide = upload_planes(gr, make_planes("p010", w, h, 1))
    bgra = 44

    def refused(descs, out_fmt, what, out_size=(w, h), **inf):
        out = GuardedImage(gr, out_size[0], out_size[1], out_fmt)
        arr = (capi.Image * len(descs))(*descs)
        i = capi.video_yuv_info(**inf)
        rc = gr.lib.gr_video_yuv_to_rgb(gr.handle, None, arr, len(descs), C.byref(out.desc), C.byref(i))
        gr.sync()
        assert rc == -1 and gr.lib.gr_last_error(gr.handle), what
        assert out.untouched(), what + ": the refused call wrote"

    d = [s.desc for s in src]
    refused(d, bgra, "BGRA output", full_range=1)
    refused(d, yr.RGBA16F, "RGBA16F without PQ", full_range=1)
    refused(d, yr.A2B10G10R10, "A2B10G10R10 without PQ", full_range=1)
    refused(d, yr.RGBA8, "RGBA8 with PQ", pq=1)
    refused(d, yr.RGBA8, "8-bit planes declared 10-bit", bit_depth=10)
    refused([s.desc for s in wide], yr.RGBA8, "16-bit planes declared 8-bit", bit_depth=8)
    refused(d, yr.RGBA8, "unknown matrix", matrix=6)
    refused(d, yr.RGBA8, "unknown chroma location", chroma_location=6)
    refused(d[:1], yr.RGBA8, "nv21 with one plane", nv21=1)
    refused(d, yr.RGBA8, "output of another size", out_size=(w, h - 1))
    refused([d[0], wide[1].desc], yr.RGBA8, "R8 luma with R16G16 chroma")
    third = capi.Image(d[1].ptr, w // 3, h // 2, d[1].pitch_bytes, yr.R8G8)
    refused([d[0], third], yr.RGBA8, "chroma plane neither full nor half size")
    short = capi.Image(d[0].ptr, w, h, w - 1, yr.R8)
    refused([short, d[1]], yr.RGBA8, "luma pitch smaller than a row")
    null = capi.Image(None, w, h, w, yr.R8)
    refused([null, d[1]], yr.RGBA8, "null plane pointer")
