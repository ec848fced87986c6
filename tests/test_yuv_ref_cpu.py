"""CPU: tests/yuv_ref.py, the reference gr_video_yuv_to_rgb is held to, against three things of its own.

1. The reference's util/yuv_to_rgb.comp, executed on the CPU and recorded in tests/golden/yuv_to_rgb_shader_v1.npz (generator and
   runner: tests/golden/make_yuv_to_rgb_golden.py, yuv_to_rgb_runner.cpp).  The shader computes in fp32, yuv_ref in float64, so they
   can only part at a rounding midpoint:
     * R8G8B8A8: at most 1 code, and at least 99 % of every colour plane's samples exact -- a misread constant, siting, clamp or dither
       index moves whole codes on many samples and fails the share first.  The share is a condition, not a measurement; when the
       golden was generated the minimum over its 32 UNORM cases was 99.837 % (one sample of 612), most cases 100 %.
     * R16G16B16A16_SFLOAT (PQ): 2 fp16 ulp + 1e-4, the project's standing bound, plus yuv_ref.pq_fp32_allowance -- the shader is an
       fp32 evaluation, and tests/test_gpu_yuv_to_rgb.py's docstring says why that alone leaves the standing bound where the terms of
       primary_conversion cancel.
   The CPU GLSL environment samples R8 and R8G8 textures but no 16-bit UNORM ones, so the golden covers 8-bit planes only; the
   16-bit fetch is v / 65535 and is covered by yuv_ref alone.
2. Exact answers: a dither probe (codes decided by the dither term alone, no tolerance) and a coordinate probe (chroma texels encode
   their own coordinates: tap indices with no tolerance) for every siting, 4:2:0 and 4:4:4, at odd sizes where chroma_clamp bites on
   the last column and row.
3. gr_video_yuv_plan (no device) against yuv_ref.plan: every float of the UBO equal as fp32 bits -- both restate the same operations
   in the same order, in fp32 -- except the translation column of yuv_to_rgb and primary_conversion, which are sums of products
   whose order a compiler may change: 1 ulp there (0 observed).  Specialization constants equal; refusals negative.
"""
import os

import numpy as np
import pytest

import yuv_ref as yr
from granite_amd import capi
from util import ulp_fp16

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "yuv_to_rgb_shader_v1.npz")
INFO_KEYS = ("bit_depth", "msb_aligned", "full_range", "matrix", "chroma_location", "pq", "nv21")


def golden_cases():
    z = np.load(GOLDEN)
    return z, sorted({k.split("/")[0] for k in z.files})


def load_case(z, name):
    planes = [z[f"{name}/plane{i}"] for i in range(3) if f"{name}/plane{i}" in z.files]
    inf = dict(zip(INFO_KEYS, (int(v) for v in z[f"{name}/info"])))
    return planes, inf, z[f"{name}/ubo"], z[f"{name}/spec"], z[f"{name}/out"]


def plan_of(planes, inf, out_fmt):
    dims = [(q.shape[1], q.shape[0], {(1, 2): yr.R8, (2, 2): yr.R16, (1, 3): yr.R8G8, (2, 3): yr.R16G16}[(q.dtype.itemsize, q.ndim)]) for q in planes]
    return dims, yr.plan(dims, (dims[0][0], dims[0][1], out_fmt), inf)


def ubo_floats(p):
    return np.concatenate([p["yuv_to_rgb"].ravel(), p["primary_conversion"].ravel(), np.float32(p["inv_resolution"]), np.float32(p["chroma_siting"]),
                           np.float32(p["chroma_clamp"]), np.float32([p["unorm_rescale"]])]).astype(np.float32)


def test_golden_covers_what_it_should():
    z, names = golden_cases()
    seen = {"planes": set(), "nv21": set(), "sub": set(), "siting": set(), "range": set(), "matrix": set(), "pq": set()}
    for name in names:
        planes, inf, _, spec, out = load_case(z, name)
        seen["planes"].add(len(planes))
        seen["nv21"].add(inf["nv21"])
        if len(planes) > 1:
            seen["sub"].add(planes[1].shape[1] < planes[0].shape[1])
            seen["siting"].add(inf["chroma_location"])
        seen["range"].add(inf["full_range"])
        seen["matrix"].add(inf["matrix"])
        seen["pq"].add((inf["pq"], out.dtype.name))
        assert planes[0].dtype == np.uint8
    assert seen == {"planes": {1, 2, 3}, "nv21": {0, 1}, "sub": {False, True}, "siting": set(range(6)), "range": {0, 1},
                    "matrix": set(range(6)), "pq": {(0, "uint8"), (1, "uint16")}}
    assert os.path.getsize(GOLDEN) < 256 * 1024


@pytest.mark.parametrize("name", golden_cases()[1])
def test_yuv_ref_matches_the_executed_shader(name):
    z, _ = golden_cases()
    planes, inf, ubo, spec, out = load_case(z, name)
    out_fmt = yr.RGBA16F if inf["pq"] else yr.RGBA8
    _, p = plan_of(planes, inf, out_fmt)
    # the recorded push block is the plan's, bit for bit, and so are the specialization constants
    assert np.array_equal(ubo_floats(p).view(np.uint32), ubo.view(np.uint32))
    assert list(spec) == [p["spec_pq"], p["spec_num_planes"], p["spec_nv21"]]
    ref = yr.store(yr.shade(planes, p), out_fmt)
    if inf["pq"]:
        a, b = out.view(np.float16).astype(np.float64), ref.view(np.float16).astype(np.float64)
        tol = 2.0 * ulp_fp16(np.maximum(np.abs(a), np.abs(b))) + 1e-4
        tol[..., :3] += yr.pq_fp32_allowance(planes, p)
        share = np.abs(a - b) / tol
        print(f"{name}: worst share of the bound {share.max():.3f}")
        assert (share <= 1.0).all(), f"{int((share > 1).sum())} channels beyond the bound, worst {share.max():.2f} times"
        return
    err = np.abs(out.astype(np.int64) - ref)
    shares = [float((err[..., c] == 0).mean()) for c in range(3)]
    print(f"{name}: worst {err.max()} code(s), exact on {100 * min(shares):.3f} % of the worst plane")
    assert err.max() <= 1
    assert (out[..., 3] == 255).all() and (ref[..., 3] == 255).all()
    assert min(shares) >= 0.99, shares


def test_dither_probe_exact():
    plane, c8, c10 = yr.dither_probe()
    assert len(np.unique(plane)) == 64
    for dtype in (np.float64, np.float32):
        assert np.array_equal(yr.yuv_to_rgb([plane], yr.RGBA8, yr.info(full_range=0), dtype), c8)
        assert np.array_equal(yr.yuv_to_rgb([plane], yr.A2B10G10R10, yr.info(full_range=0, pq=1), dtype), c10)
    # the term is the table's: every 4 x 4 block of one luma code holds at most two codes, and differs from its neighbour blocks
    assert all(len(np.unique(c8[y:y + 4, x:x + 4, 0])) <= 2 for y in range(0, 16, 4) for x in range(0, 64, 4))


@pytest.mark.parametrize("location", range(6))
@pytest.mark.parametrize("sub", [True, False], ids=["420", "444"])
@pytest.mark.parametrize("size", [(67, 35), (34, 18), (35, 19), (5, 3), (2, 1), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_coordinate_probe_exact(size, sub, location):
    """The taps yuv_ref resolves to against the position computed in exact rational arithmetic: the first tap's index is equal (no
    tolerance) wherever the exact position is not itself on a texel centre, and the position t0 + weight is equal to 1e-4 texel -- the
    normalised fp32 coordinate (x + siting) / w * cw carries a few roundings of 2^-24 * cw texel, which is all that separates the two.
    On a texel centre the 2^-8 snap decides for that texel alone."""
    w, h = size
    planes, ex, ey = yr.coordinate_probe(w, h, sub, location)
    dims, p = plan_of(planes, yr.info(full_range=1, chroma_location=location), yr.RGBA8)
    (x0, x1, a), (y0, y1, b) = yr.chroma_taps(p, dims[1][0], dims[1][1])
    for t0, t1, wt, want in ((x0, x1, a, ex), (y0, y1, b, ey)):
        centre = np.abs(want - np.round(want)) < 1e-3
        assert np.array_equal(t0[~centre], np.floor(want[~centre]).astype(np.int64))
        # on a centre (the plane's edge included, where both taps are clamped onto the edge texel) that texel alone is read
        alone = (wt[centre] == 0.0) | (t0[centre] == t1[centre])
        assert alone.all() and np.array_equal(t0[centre], np.round(want[centre]).astype(np.int64))
        assert np.abs(t0 + (t1 - t0) * wt.astype(np.float64) - want).max() <= 1e-4
    if sub and w > 2 and w & 1:
        # the clamp does bite: without it the last column would sit beyond the last chroma texel's centre for sitings left of centre
        assert ex[-1] <= (w + 1) // 2 - 1
    # and the sampled chroma is the probe's own ramp at those positions: the stored planes read back through the fetch
    c = yr._sample_chroma(np.stack([planes[1], planes[2]], axis=-1).astype(np.float64), p, np.float64)
    assert np.abs(c[..., 0] - yr.PROBE_STEP * ex[None, :]).max() <= yr.PROBE_STEP * 1e-4
    assert np.abs(c[..., 1] - yr.PROBE_STEP * ey[:, None]).max() <= yr.PROBE_STEP * 1e-4


def layouts(w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    for wide in (False, True):
        y, c2 = (yr.R16, yr.R16G16) if wide else (yr.R8, yr.R8G8)
        yield wide, [(w, h, y)]
        for cs in ((cw, ch), (w, h)):
            yield wide, [(w, h, y), (*cs, c2)]
            yield wide, [(w, h, y), (*cs, y), (*cs, y)]


@pytest.mark.parametrize("size", [(67, 35), (34, 18), (1280, 576), (1280, 700), (1920, 1080), (3840, 2160), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_plan_matches_yuv_ref(size):
    w, h = size
    checked = 0
    for wide, planes in layouts(w, h):
        for depth, msb in (((10, 1), (10, 0), (16, 0)) if wide else ((8, 0),)):
            for matrix in range(6):
                for full in (0, 1):
                    for loc in range(6):
                        for out_fmt, pq in ((yr.RGBA8, 0), (yr.RGBA8_SRGB, 0), (yr.RGBA16F, 1), (yr.A2B10G10R10, 1)):
                            nv21 = int(len(planes) == 2 and loc & 1)
                            want = yr.plan(planes, (w, h, out_fmt), yr.info(depth, msb, full, matrix, loc, pq, nv21))
                            got = capi.video_yuv_plan(planes, (w, h, out_fmt), capi.video_yuv_info(depth, msb, full, matrix, loc, pq, nv21))
                            assert want is not None and got is not None
                            for k in ("spec_pq", "spec_num_planes", "spec_nv21", "matrix"):
                                assert int(got[k]) == int(want[k]), k
                            assert tuple(got["resolution"]) == (w, h)
                            for k in ("inv_resolution", "chroma_siting", "chroma_clamp", "unorm_rescale"):
                                assert np.array_equal(np.float32(got[k]).view(np.uint32), np.float32(want[k]).view(np.uint32)), k
                            a, b = got["yuv_to_rgb"], want["yuv_to_rgb"]
                            assert np.array_equal(a[:3].view(np.uint32), b[:3].view(np.uint32)), "yuv_to_rgb"
                            for x, y in ((a[3], b[3]), (got["primary_conversion"], want["primary_conversion"])):
                                d = np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64))
                                assert d.max() <= 1, (x, y)
                            checked += 1
    assert checked > 1000


def test_unspecified_matrix_goes_by_height():
    for h, want in ((480, yr.M_BT601_525), (624, yr.M_BT601_525), (625, yr.M_BT601_625), (719, yr.M_BT601_625), (720, yr.M_BT709),
                    (2159, yr.M_BT709), (2160, yr.M_BT2020)):
        got = capi.video_yuv_plan([(64, h, yr.R8)], (64, h, yr.RGBA8), capi.video_yuv_info(matrix=capi.VIDEO_MATRIX_UNSPECIFIED))
        assert got["matrix"] == want == yr.plan([(64, h, yr.R8)], (64, h, yr.RGBA8), yr.info(matrix=yr.M_UNSPECIFIED))["matrix"]


def test_push_block_values():
    """A few values by hand: BT.709 limited range 8 bits."""
    p = capi.video_yuv_plan([(64, 32, yr.R8), (32, 16, yr.R8G8)], (64, 32, yr.RGBA8), capi.video_yuv_info(full_range=0))
    m = p["yuv_to_rgb"].astype(np.float64)
    assert abs(m[0][0] - 255.0 / 219.0) < 1e-6 and abs(m[2][0] - 1.5748 * 255.0 / 224.0) < 1e-6
    # black (16, 128, 128) and white (235, 128, 128) map to 0 and 1
    for code, want in ((16, 0.0), (235, 1.0)):
        rgb = m[0][:3] * code / 255 + (m[1][:3] + m[2][:3]) * 128 / 255 + m[3][:3]
        assert np.abs(rgb - want).max() < 1e-6
    assert p["chroma_clamp"] == (np.float32(63.0) * np.float32(1.0 / 64.0), np.float32(31.0) * np.float32(1.0 / 32.0))
    assert np.array_equal(p["primary_conversion"], np.eye(4, dtype=np.float32))
    for depth, msb, want in ((10, 1, 65535.0 / (1023 << 6)), (10, 0, 65535.0 / 1023.0), (16, 0, 1.0)):
        q = capi.video_yuv_plan([(64, 32, yr.R16)], (64, 32, yr.RGBA8), capi.video_yuv_info(bit_depth=depth, msb_aligned=msb))
        assert q["unorm_rescale"] == np.float32(want)
    # BT.2020 -> BT.709 primaries: the well-known matrix
    q = capi.video_yuv_plan([(64, 32, yr.R8)], (64, 32, yr.RGBA8), capi.video_yuv_info(matrix=capi.VIDEO_MATRIX_BT2020))
    pc = q["primary_conversion"][:3, :3].T.astype(np.float64)  # rows
    assert np.abs(pc - np.array([[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]])).max() < 2e-4


def test_refusals_return_negative():
    ok = [(64, 32, yr.R8), (32, 16, yr.R8G8)]
    i = capi.video_yuv_info
    assert capi.video_yuv_plan(ok, (64, 32, yr.RGBA8), i()) is not None
    refused = [
        (ok, (64, 32, 44), i()),                                   # BGRA output
        (ok, (64, 32, yr.RGBA16F), i()),                           # RGBA16F without PQ
        (ok, (64, 32, yr.A2B10G10R10), i()),                       # A2B10G10R10 without PQ
        (ok, (64, 32, yr.RGBA8), i(pq=1)),                         # RGBA8 with PQ
        (ok, (64, 31, yr.RGBA8), i()),                             # output of another size
        (ok, (64, 32, yr.RGBA8), i(bit_depth=10)),                 # 8-bit planes, 10-bit stream
        (ok, (64, 32, yr.RGBA8), i(bit_depth=12)),
        ([(64, 32, yr.R16)], (64, 32, yr.RGBA8), i(bit_depth=8)),  # 16-bit planes, 8-bit stream
        (ok, (64, 32, yr.RGBA8), i(matrix=6)),
        (ok, (64, 32, yr.RGBA8), i(chroma_location=6)),
        (ok[:1], (64, 32, yr.RGBA8), i(nv21=1)),
        ([(64, 32, yr.R8), (32, 16, yr.R16G16)], (64, 32, yr.RGBA8), i()),
        ([(64, 32, yr.R8), (32, 16, yr.R8)], (64, 32, yr.RGBA8), i()),                  # two planes need interleaved chroma
        ([(64, 32, yr.R8), (32, 16, yr.R8G8), (32, 16, yr.R8G8)], (64, 32, yr.RGBA8), i()),
        ([(64, 32, yr.R8), (21, 16, yr.R8G8)], (64, 32, yr.RGBA8), i()),                # neither full nor half size
        ([(64, 32, yr.R8), (32, 32, yr.R8G8)], (64, 32, yr.RGBA8), i()),                # 4:2:2
        ([(64, 32, yr.R8), (32, 16, yr.R8), (32, 15, yr.R8)], (64, 32, yr.RGBA8), i()),
        ([(64, 32, yr.RGBA8)], (64, 32, yr.RGBA8), i()),
        ([(0, 32, yr.R8)], (0, 32, yr.RGBA8), i()),
        ([], (64, 32, yr.RGBA8), i()),
    ]
    for planes, out, inf in refused:
        assert capi.video_yuv_plan(planes, out, inf) is None, (planes, out)
        d = {k: int(getattr(inf, k)) for k in INFO_KEYS}
        assert yr.plan(planes, out, d) is None, (planes, out)
    lib = capi.load_library()
    assert lib.gr_video_yuv_plan(None, 1, None, None, None) < 0


@pytest.mark.parametrize("planes", [[(1, 2, yr.R8), (1, 1, yr.R8G8)], [(1, 2, yr.R8), (1, 1, yr.R8), (1, 1, yr.R8)]], ids=["nv12", "three_planes"])
def test_plan_accepts_one_pixel_wide_420(planes):
    """A 4:2:0 frame one pixel wide has chroma as wide as its luma.  Playback tells subsampling by the width or the height and takes
    it; gr_video_scale_plan, by the width alone, refuses the same planes (tests/test_video_scaler_cpu.py)."""
    q = capi.video_yuv_plan(planes, (1, 2, yr.RGBA8), capi.video_yuv_info())
    assert q is not None
    assert capi.video_scale_plan((1, 2), yr.RGBA8, planes, capi.COLOR_SPACE_SRGB_NONLINEAR, capi.COLOR_SPACE_SRGB_NONLINEAR) is None


def test_golden_regenerates_identically(tmp_path):
    """Needs the reference's sources: re-spells and re-runs the shader, and must reproduce the committed file's every array."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_yuv_to_rgb_golden", os.path.join(HERE, "golden", "make_yuv_to_rgb_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if not os.path.exists(gen.SHADER):
        pytest.skip("the reference's sources are not here")
    path = str(tmp_path / "regenerated.npz")
    gen.generate(path)
    new, old = np.load(path), np.load(GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k
