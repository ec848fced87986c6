"""GPU: every gr_cacao_* entry point, each stage fed the stored inputs of tests/cacao_ref.py's float32 chain, at the four sizes of
tests/cacao_cases.py, both qualities, with guard bytes around the workspace and the output and padded pitches on every gr_image
(tests/cacao_chain.py states the bounds; tests/test_cacao_core_cpu.py runs the same cases through the host build of the same kernel text).
Then the whole pass through Context.cacao against the reference chain, and the sequence called twice, which must give the same bytes."""
import ctypes as C

import numpy as np
import pytest

import cacao_cases as cc
import cacao_chain as chain
import cacao_ref as cr
from granite_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gr():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def constants_array(records):
    out = (capi.CacaoConstants * 4)()
    C.memmove(out, np.ascontiguousarray(records).ctypes.data, 4 * 384)
    return out


class PitchedImage:
    """a gr_image whose rows carry `extra` more elements than its width, filled with a pattern"""

    def __init__(self, gr, array, fmt, extra, fill):
        self.rows = chain.padded(array, extra, fill)
        self.buffer = capi.DeviceBuffer(gr, self.rows.nbytes).upload(self.rows)
        self.desc = capi.Image(self.buffer.ptr, array.shape[1], array.shape[0], self.rows.strides[0], fmt)

    def download(self):
        return self.buffer.download(self.rows.dtype).reshape(self.rows.shape)


class DeviceBackend:
    def __init__(self, gr):
        self.gr = gr

    def layout(self, w, h):
        d = capi.cacao_workspace_describe(w, h)
        offsets = d[0]["mip_offset"] + [d[i]["mip_offset"][0] for i in range(1, 7)] + [self.gr.lib.gr_cacao_workspace_bytes(w, h)]
        return chain.Layout(w, h, offsets)

    def run(self, stage, guarded, constants, width, height, **a):
        gr, lib, h = self.gr, self.gr.lib, self.gr.handle
        buffer = capi.DeviceBuffer(gr, guarded.size).upload(guarded)
        ws = buffer.ptr + chain.GUARD
        c = constants_array(constants)
        out = None
        if stage == "prepare_depths":
            image = PitchedImage(gr, a["depth"], capi.FORMAT_D32_SFLOAT, 3, np.float32(7.0))
            gr.check(lib.gr_cacao_prepare_depths(h, None, image.desc, ws, c))
        elif stage == "prepare_normals":
            image = PitchedImage(gr, a["normal"], capi.FORMAT_A2B10G10R10_UNORM_PACK32, 5, np.uint32(0xffffffff))
            gr.check(lib.gr_cacao_prepare_normals(h, None, image.desc, ws, c))
        elif stage == "generate_base":
            gr.check(lib.gr_cacao_generate_base(h, None, ws, width, height, c))
        elif stage == "generate":
            gr.check(lib.gr_cacao_generate(h, None, ws, width, height, c, a["quality"]))
        elif stage.startswith("importance_"):
            gr.check(getattr(lib, "gr_cacao_" + stage)(h, None, ws, width, height, c))
        elif stage == "blur":
            gr.check(lib.gr_cacao_blur(h, None, ws, width, height, c, a["blur_passes"]))
        elif stage == "apply":
            out = PitchedImage(gr, np.full((height, width), chain.FILL, np.uint8), capi.FORMAT_R8_UNORM, 7, np.uint8(chain.FILL))
            gr.check(lib.gr_cacao_apply(h, None, ws, out.desc, c, a["from_pong"]))
        else:
            raise KeyError(stage)
        gr.sync()
        result = buffer.download()
        return (result, out.download()) if out is not None else result


@pytest.mark.parametrize("quality", cc.QUALITIES, ids=lambda q: f"q{q}")
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_stages_against_reference(gr, case, quality):
    chain.check_stages(DeviceBackend(gr), case, quality)


def run_pass(gr, case, quality, blur_passes, workspace=None):
    w, h, cam_name, variant, _ = case
    ref = chain.reference(case, quality)
    depth = capi.DeviceImage(gr, w, h, capi.FORMAT_D32_SFLOAT).upload(ref["depth"])
    normal = capi.DeviceImage(gr, w, h, capi.FORMAT_A2B10G10R10_UNORM_PACK32).upload(ref["normal"])
    out = capi.DeviceImage(gr, w, h, capi.FORMAT_R8_UNORM)
    workspace = workspace or gr.cacao_workspace(w, h)
    gr.cacao(depth, normal, out, workspace, constants_array(cc.constants(w, h, cam_name, variant, quality)), quality, blur_passes)
    gr.sync()
    return out.download(), workspace


@pytest.mark.parametrize("quality", cc.QUALITIES, ids=lambda q: f"q{q}")
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_whole_pass_against_reference_chain(gr, case, quality):
    got, workspace = run_pass(gr, case, quality, 2)
    want = chain.reference(case, quality)["output"]
    distance = chain.codes(got, want)
    print(f"{cc.case_id(case)} q{quality}: whole pass largest difference {int(distance.max())} code(s), mean {float(distance.mean()):.5f}")
    largest, mean = chain.whole_pass_bound(case, quality)  # the float32-against-float64 measurement + 1 code, and twice its mean
    assert distance.max() <= largest, (int(distance.max()), largest)
    assert distance.mean() <= mean, (float(distance.mean()), mean)
    # the same sequence on the workspace the first run left behind: the counter is cleared, nothing else is carried over
    again, _ = run_pass(gr, case, quality, 2, workspace)
    assert np.array_equal(got, again)


def test_constants_from_the_library_are_the_references(gr):
    """capi.cacao_constants -- gr_cacao_update_buffer_sizes and gr_cacao_update_constants -- on one case, against the recorded bytes"""
    w, h = 130, 98
    g = cc.golden()
    k = cc.key(w, h, "survey", "reference", cr.QUALITY_HIGHEST)
    got = np.frombuffer(bytes(capi.cacao_constants(w, h, g[k + "/proj"], g[k + "/view"], ctx=gr)), cr.CONSTANTS_DTYPE)
    want = g[k + "/constants"].view(cr.CONSTANTS_DTYPE).reshape(4)
    for name in cr.CONSTANTS_DTYPE.names:
        if name == "PatternRotScaleMatrices":
            assert np.abs(got[name].view(np.int32).astype(np.int64) - want[name].view(np.int32).astype(np.int64)).max() <= 1
        else:
            assert got[name].tobytes() == want[name].tobytes(), name
