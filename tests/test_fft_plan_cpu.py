"""CPU: the pass list of an FFT plan as gr_fft_describe (host-only) reports it: radices, cumulative p, LDS, the place of the real-mode
resolve, the ping-pong between the buffers, and every refusal of gr_fft_plan_create's option check."""
import pytest

from granite_amd import capi

LDS_LIMIT = 80 * 1024  # two workgroups share a CU's 160 KiB (fft_core.hpp: LDS_LIMIT)
MODES = [capi.FFT_FORWARD_C2C, capi.FFT_INVERSE_C2C, capi.FFT_R2C, capi.FFT_C2R]
REAL = (capi.FFT_R2C, capi.FFT_C2R)


def describe(nx, ny=1, nz=1, dimensions=1, mode=capi.FFT_FORWARD_C2C, data_type=capi.FFT_FP32, **kw):
    return capi.fft_describe(capi.fft_options(nx, ny, nz, dimensions, mode, data_type, **kw))


def check_plan(nx, ny, nz, dimensions, mode, data_type):
    passes = describe(nx, ny, nz, dimensions, mode, data_type)
    assert passes, (nx, ny, nz, dimensions, mode, data_type)
    extents = [nx // 2 if mode in REAL else nx, ny, nz]
    c2c = [p for p in passes if p.kind == capi.FFT_PASS_C2C]
    for dim in range(3):
        own = [p for p in c2c if p.dimension == dim]
        if dim >= dimensions:
            assert not own
            continue
        product = 1
        for p in own:
            assert p.p == product, "p runs 1, r1, r1 r2, ..."
            assert p.points >= 4 and p.points & (p.points - 1) == 0
            product *= p.points
        assert product == extents[dim]
    for p in passes:
        assert p.lds_bytes <= LDS_LIMIT
        assert p.grid_size >= 1 and p.workgroup_size in (256, 512)
        if p.kind == capi.FFT_PASS_C2C:
            assert p.columns * p.points <= 8192 and p.lds_bytes >= p.columns * p.points * 8
    # the dimensions in order, reversed for C2R, each dimension's passes together
    order = [p.dimension for p in c2c]
    assert order == sorted(order, reverse=mode == capi.FFT_C2R)
    # exactly one resolve in a real mode, none otherwise
    resolves = [i for i, p in enumerate(passes) if p.kind != capi.FFT_PASS_C2C]
    if mode in REAL:
        assert len(resolves) == 1
        at = resolves[0]
        x_passes = [i for i, p in enumerate(passes) if p.kind == capi.FFT_PASS_C2C and p.dimension == 0]
        if mode == capi.FFT_R2C:
            # after the last pass of dimension 0 and before the other dimensions (last of all in one dimension)
            assert passes[at].kind == capi.FFT_PASS_R2C_RESOLVE and at == x_passes[-1] + 1 and x_passes[0] == 0
            if dimensions == 1:
                assert at == len(passes) - 1
        else:
            # first of dimension 0, which comes last
            assert passes[at].kind == capi.FFT_PASS_C2R_RESOLVE and at == x_passes[0] - 1 and x_passes[-1] == len(passes) - 1
    else:
        assert not resolves
    # the ping-pong: the first pass reads the source, every pass reads what the one before wrote, never the buffer it writes, the last
    # writes the destination, and neither user buffer is used in between
    assert passes[0].reads == capi.FFT_BUFFER_SRC and passes[-1].writes == capi.FFT_BUFFER_DST
    for i, p in enumerate(passes):
        assert p.reads != p.writes
        if i:
            assert p.reads == passes[i - 1].writes and p.reads in (capi.FFT_BUFFER_SCRATCH_A, capi.FFT_BUFFER_SCRATCH_B)
        if i + 1 < len(passes):
            assert p.writes in (capi.FFT_BUFFER_SCRATCH_A, capi.FFT_BUFFER_SCRATCH_B)
    return passes


@pytest.mark.parametrize("data_type", [capi.FFT_FP32, capi.FFT_FP16])
@pytest.mark.parametrize("mode", MODES)
def test_every_power_of_two_in_each_dimension(mode, data_type):
    for log2 in range(2, 25):
        n = 1 << log2
        if not (mode in REAL and n < 8):
            check_plan(n, 1, 1, 1, mode, data_type)
            check_plan(n, 3, 1, 1, mode, data_type)  # batched
        check_plan(8, n, 1, 2, mode, data_type)
        check_plan(8, 4, n, 3, mode, data_type)


@pytest.mark.parametrize("data_type", [capi.FFT_FP32, capi.FFT_FP16])
@pytest.mark.parametrize("mode", MODES)
def test_shapes_in_two_and_three_dimensions(mode, data_type):
    for nx, ny, nz, dims in ((8, 4, 1, 2), (64, 32, 1, 2), (1024, 1024, 1, 2), (2048, 1024, 1, 2), (256, 256, 3, 2), (8192, 16384, 1, 2), (16384, 4096, 5, 2),
                             (8, 4, 4, 3), (16, 8, 4, 3), (128, 64, 32, 3), (8, 8192, 2048, 3), (1 << 16, 16, 1, 1)):
        check_plan(nx, ny, nz, dims, mode, data_type)


def test_one_pass_up_to_4096_points_in_a_row_and_two_above():
    assert len(describe(4096)) == 1 and len(describe(8192)) == 2
    assert [p.points for p in describe(1 << 20)] == [1024, 1024]
    # a column pass keeps a 64-byte run of columns: 8 in fp32, 16 in fp16
    assert all(p.columns >= 8 for p in describe(1024, 1024, 1, 2) if p.dimension == 1)
    assert all(p.columns >= 16 for p in describe(1024, 1024, 1, 2, data_type=capi.FFT_FP16) if p.dimension == 1)


def test_refusals():
    T, B = capi.FFT_RESOURCE_TEXTURE, capi.FFT_RESOURCE_BUFFER
    assert describe(8, mode=capi.FFT_R2C) is not None
    for mode in REAL:
        assert describe(4, mode=mode) is None  # the real length is halved before the >= 4 rule
        assert describe(4, 8, 1, 2, mode=mode) is None
    for n in (0, 1, 2, 3, 6, 12, 100, 1000, (1 << 20) + 1):
        assert describe(n) is None, n
        assert describe(8, n, 1, 2) is None, n
        assert describe(8, 8, n, 3) is None, n
    assert describe(8, 6, 1, 1) is not None and describe(8, 8, 6, 2) is not None  # batches need no power of two
    assert describe(8, 0) is None and describe(8, 1, 0) is None
    for dims in (0, 4):
        assert describe(8, 8, 8, dims) is None
    assert describe(8, mode=4) is None and describe(8, data_type=2) is None
    assert describe(8, output_resource=2) is None and describe(8, input_resource=2) is None
    # texture input, in every mode
    for mode in MODES:
        assert describe(16, 16, 1, 2, mode, input_resource=T) is None
    # texture output: not with Nz > 1, not with a real mode in one dimension, not wider than an image
    assert describe(16, 16, 1, 2, output_resource=T) is not None
    assert describe(16, 16, 2, 2, output_resource=T) is None
    assert describe(16, 16, 4, 3, output_resource=T) is None
    assert describe(16, 1, 1, 1, output_resource=T) is not None
    for mode in REAL:
        assert describe(16, 16, 1, 1, mode, output_resource=T) is None
        assert describe(16, 16, 1, 2, mode, output_resource=T) is not None
    assert describe(1 << 17, 4, 1, 2, output_resource=T) is None
    # 2^31 elements or more
    assert describe(1 << 16, 1 << 15, 1, 2) is None
    assert describe(1 << 11, 1 << 10, 1 << 10, 3) is None
    assert describe(1 << 16, 1 << 14, 1, 2) is not None
    assert describe(1 << 24, 1 << 7, 1, 1) is None
    # batch extents need no power of two and may be anything: the product must not wrap 64 bits (2^64, 2^32 + ..., 2^63 elements)
    assert describe(1 << 16, 1 << 24, 1 << 24, 1) is None
    assert describe(1 << 16, (1 << 32) - 1, (1 << 32) - 1, 1) is None
    assert describe(8, (1 << 32) - 1, 1, 1) is None and describe(8, 1, (1 << 32) - 1, 1) is None
    assert describe(1 << 31, 1, 1, 1) is None
    assert describe(8, 1 << 14, 1 << 14, 1) is None and describe(8, 1 << 14, (1 << 13) - 1, 1) is not None
