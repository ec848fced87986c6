"""What the CPU test of cacao_core.hpp and the GPU test of the gr_cacao_* entry points share: the reference chain per case (computed once),
the workspace as numpy sees it, and check_stages(), which feeds every stage the REFERENCE's stored inputs and holds its output to the
bounds below.  A backend runs one stage on a workspace: tests/test_cacao_core_cpu.py's is the host build of the kernels, tests/
test_gpu_cacao.py's is the device.

Bounds, per stage:
  - byte-identical to cacao_ref in float32, no texel exempt: prepare depths with all four mips, prepare normals, importance A and B and
    the counter word, blur at 1, 2 and 8 passes, apply (after 0, 1, 2 and 8 blur passes).  These stages contain no library function.
  - at most ONE_CODE per channel at every unflagged texel: generate base, generate Q2 / Q3, importance map.  pow and log2 differ between
    math libraries by a few ulps, <= 1e-6 before a quantisation step of 1 / 255: more than one code is a bug.  Texels the reference flags
    (a tap's lod within 2^-10 of a mip switch, where the last bit of log2 selects another depth) are left out; their share must be
    <= FLAG_SHARE_LIMIT in every case.
  - every byte of the workspace outside the stage's outputs, and the guard bytes around the workspace and the output image, unchanged.
"""
import functools

import numpy as np

import cacao_cases as cc
import cacao_ref as cr

ONE_CODE = 1
FLAG_SHARE_LIMIT = 0.005
GUARD = 256
FILL = 0xA5
BLUR_PASSES = (1, 2, 8)
# The whole pass is not derivable: a one-code change upstream moves discrete sample counts downstream.  Measured on the CPU, per case and
# quality: the distance of the final image between cacao_ref in float32 and in float64 -- largest difference in R8 codes, mean absolute
# difference (tests/test_cacao_ref_cpu.py::test_float32_against_float64 measures them again, prints them and holds them to the same bound).
# The device gets the largest + 1 code, for its own pow / log2, and twice the mean: whole_pass_bound().
WHOLE_PASS_MEASURED = {
    ("64x48-survey-reference-synthetic", 4): (3, 0.00423),
    ("64x48-survey-reference-synthetic", 3): (1, 0.00065),
    ("64x48-survey-wide-box", 4): (1, 0.00065),
    ("64x48-survey-wide-box", 3): (1, 0.00033),
    ("64x48-oblique-reference-box", 4): (1, 0.00391),
    ("64x48-oblique-reference-box", 3): (1, 0.0026),
    ("61x45-survey-reference-synthetic", 4): (4, 0.01202),
    ("61x45-survey-reference-synthetic", 3): (0, 0.0),
    ("61x45-survey-wide-box", 4): (1, 0.00146),
    ("61x45-survey-wide-box", 3): (1, 0.00146),
    ("61x45-oblique-reference-box", 4): (1, 0.00073),
    ("61x45-oblique-reference-box", 3): (1, 0.00073),
    ("130x98-survey-reference-synthetic", 4): (1, 0.00479),
    ("130x98-survey-reference-synthetic", 3): (1, 0.00024),
    ("130x98-survey-wide-box", 4): (1, 0.00173),
    ("130x98-survey-wide-box", 3): (1, 0.00118),
    ("130x98-oblique-reference-box", 4): (1, 0.00267),
    ("130x98-oblique-reference-box", 3): (1, 0.00078),
    ("16x16-survey-reference-synthetic", 4): (0, 0.0),
    ("16x16-survey-reference-synthetic", 3): (0, 0.0),
    ("16x16-survey-wide-box", 4): (0, 0.0),
    ("16x16-survey-wide-box", 3): (0, 0.0),
    ("16x16-oblique-reference-box", 4): (0, 0.0),
    ("16x16-oblique-reference-box", 3): (0, 0.0),
}


def whole_pass_bound(case, quality):
    largest, mean = WHOLE_PASS_MEASURED[(cc.case_id(case), quality)]
    return largest + 1, 2.0 * mean
INTERMEDIATES = ("depth_mips", "normals", "ping", "pong", "importance", "importance_pong", "load_counter")


class Layout:
    """offsets: depth_mip[4], normals, ssao ping, ssao pong, importance, importance pong, load counter, bytes"""

    def __init__(self, width, height, offsets):
        self.width, self.height = width, height
        self.hw, self.hh = cr.half_size(width, height)
        self.iw, self.ih = cr.half_size(self.hw, self.hh)
        o = [int(v) for v in offsets]
        self.depth_mip, self.normals, self.ping, self.pong, self.importance, self.importance_pong, self.load_counter, self.bytes = o[0:4], *o[4:11]

    def mip_shape(self, k):
        return cr.PASSES, cr.mip_extent(self.hh, k), cr.mip_extent(self.hw, k)

    def ranges(self, name):
        """[(offset, bytes)] of one intermediate"""
        if name == "depth_mips":
            return [(self.depth_mip[k], int(np.prod(self.mip_shape(k))) * 2) for k in range(cr.DEPTH_MIPS)]
        half = self.hw * self.hh * cr.PASSES
        return [{"normals": (self.normals, half * 4), "ping": (self.ping, half * 2), "pong": (self.pong, half * 2),
                 "importance": (self.importance, self.iw * self.ih), "importance_pong": (self.importance_pong, self.iw * self.ih),
                 "load_counter": (self.load_counter, 4)}[name]]

    def put(self, buf, name, value):
        if name == "depth_mips":
            for k, (offset, n) in enumerate(self.ranges(name)):
                assert value[k].shape == self.mip_shape(k) and value[k].dtype == np.uint16
                buf[offset:offset + n] = np.ascontiguousarray(value[k]).view(np.uint8).reshape(-1)
            return
        (offset, n), = self.ranges(name)
        value = np.ascontiguousarray(np.uint32(value) if name == "load_counter" else value).view(np.uint8).reshape(-1)
        assert value.size == n, (name, value.size, n)
        buf[offset:offset + n] = value

    def get(self, buf, name):
        if name == "depth_mips":
            return [buf[offset:offset + n].view(np.uint16).reshape(self.mip_shape(k)).copy() for k, (offset, n) in enumerate(self.ranges(name))]
        (offset, n), = self.ranges(name)
        raw = buf[offset:offset + n].copy()
        if name == "normals":
            return raw.reshape(cr.PASSES, self.hh, self.hw, 4)
        if name in ("ping", "pong"):
            return raw.reshape(cr.PASSES, self.hh, self.hw, 2)
        if name == "load_counter":
            return int(raw.view(np.uint32)[0])
        return raw.reshape(self.ih, self.iw)


@functools.lru_cache(maxsize=None)
def reference(case, quality, blur_passes=2, dtype="float32"):
    """cacao_ref.chain of one case, computed once and shared; nobody changes it"""
    w, h, cam_name, variant, _ = case
    depth, normal = cc.case_inputs(case)
    r = cr.chain(depth, normal, cc.constants(w, h, cam_name, variant, quality), quality, blur_passes, getattr(np, dtype))
    r["depth"], r["normal"] = depth, normal
    return r


@functools.lru_cache(maxsize=None)
def reference_blur(case, quality, passes):
    w, h, cam_name, variant, _ = case
    return cr.blur(reference(case, quality)["ping"], cc.constants(w, h, cam_name, variant, quality)[0], passes)


@functools.lru_cache(maxsize=None)
def reference_apply(case, quality, passes):
    w, h, cam_name, variant, _ = case
    source = reference_blur(case, quality, passes) if passes else reference(case, quality)["ping"]
    return cr.apply(source, cc.constants(w, h, cam_name, variant, quality)[0], w, h)


def padded(image, extra_elements, fill):
    """(rows with `extra_elements` more elements, view of the image inside them)"""
    h, w = image.shape
    rows = np.full((h, w + extra_elements), fill, image.dtype)
    rows[:, :w] = image
    return rows


def codes(a, b):
    return np.abs(a.astype(np.int32) - b.astype(np.int32))


def check_stages(backend, case, quality):
    """backend: .layout(w, h) -> Layout; .run(stage, workspace bytes, **arguments) -> workspace bytes afterwards (and, for "apply", the
    output rows with their padding).  Returns the figures it printed, for the caller's docstring-grade record."""
    w, h, cam_name, variant, _ = case
    constants = cc.constants(w, h, cam_name, variant, quality)
    ref = reference(case, quality)
    layout = backend.layout(w, h)
    figures = {}

    def stage(name, inputs, outputs, **arguments):
        before = np.full(layout.bytes + 2 * GUARD, FILL, np.uint8)
        inner = before[GUARD:GUARD + layout.bytes]
        for key, value in inputs.items():
            layout.put(inner, key, value)
        after = backend.run(name, before.copy(), constants=constants, width=w, height=h, **arguments)
        result = after[0] if isinstance(after, tuple) else after
        changed = np.flatnonzero(result != before)
        allowed = np.zeros(before.size, bool)
        for key in outputs:
            for offset, n in layout.ranges(key):
                allowed[GUARD + offset:GUARD + offset + n] = True
        stray = changed[~allowed[changed]]
        assert stray.size == 0, f"{name}: {stray.size} bytes outside its outputs changed, first at workspace offset {int(stray[0]) - GUARD}"
        got = {key: layout.get(result[GUARD:GUARD + layout.bytes], key) for key in outputs}
        return (got, after[1]) if isinstance(after, tuple) else got

    def exact(name, got, want):
        assert np.array_equal(got, want), f"{name}: {int(np.count_nonzero(np.asarray(got) != np.asarray(want)))} elements differ from the fp32 reference"

    def within_one_code(name, got, want, flag=None):
        distance = codes(got, want)
        if flag is not None:
            share = float(flag.mean())
            figures[name + " flagged share"] = share
            assert share <= FLAG_SHARE_LIMIT, f"{name}: the reference flags {100 * share:.3f} % of the texels"
            distance = distance[~flag]
        worst = int(distance.max()) if distance.size else 0
        figures[name + " largest difference in codes"] = worst
        figures[name + " texels one code off"] = int(np.count_nonzero(distance))
        print(f"{cc.case_id(case)} q{quality} {name}: largest difference {worst} code(s), {int(np.count_nonzero(distance))} of {distance.size} values differ")
        assert worst <= ONE_CODE, f"{name}: {worst} codes from the fp32 reference at an unflagged texel"

    # prepare: the counter is cleared with the depths
    got = stage("prepare_depths", {"load_counter": 0xdeadbeef}, ("depth_mips", "load_counter"), depth=ref["depth"])
    for k in range(cr.DEPTH_MIPS):
        exact(f"prepare depths mip {k}", got["depth_mips"][k], ref["depth_mips"][k])
    assert got["load_counter"] == 0
    got = stage("prepare_normals", {}, ("normals",), normal=ref["normal"])
    exact("prepare normals", got["normals"], ref["normals"])

    prepared = {"depth_mips": ref["depth_mips"], "normals": ref["normals"]}
    if quality == cr.QUALITY_HIGHEST:
        got = stage("generate_base", prepared, ("pong",))
        within_one_code("generate base", got["pong"], ref["base"], ref["base_info"]["flag"][..., None].repeat(2, axis=-1))
        got = stage("importance_generate", {"pong": ref["base"]}, ("importance",))
        within_one_code("importance map", got["importance"], ref["importance_0"])
        got = stage("importance_postprocess_a", {"importance": ref["importance_0"]}, ("importance_pong",))
        exact("importance A", got["importance_pong"], ref["importance_a"])
        got = stage("importance_postprocess_b", {"importance_pong": ref["importance_a"], "load_counter": 0}, ("importance", "load_counter"))
        exact("importance B", got["importance"], ref["importance"])
        assert got["load_counter"] == ref["load_counter"], f"load counter {got['load_counter']}, reference {ref['load_counter']}"
        got = stage("generate", dict(prepared, pong=ref["base"], importance=ref["importance"], load_counter=ref["load_counter"]), ("ping",), quality=quality)
        within_one_code("generate Q3", got["ping"], ref["ping"], ref["info"]["flag"][..., None].repeat(2, axis=-1))
    else:
        got = stage("generate", prepared, ("ping",), quality=quality)
        within_one_code("generate Q2", got["ping"], ref["ping"], ref["info"]["flag"][..., None].repeat(2, axis=-1))

    for passes in BLUR_PASSES:
        got = stage("blur", {"ping": ref["ping"]}, ("pong",), blur_passes=passes)
        exact(f"blur {passes}", got["pong"], reference_blur(case, quality, passes))
    for passes in (0,) + BLUR_PASSES:
        source = {"pong": reference_blur(case, quality, passes)} if passes else {"ping": ref["ping"]}
        _, rows = stage("apply", source, (), from_pong=1 if passes else 0)
        exact(f"apply after {passes} blur passes", rows[:, :w], reference_apply(case, quality, passes))
        assert np.all(rows[:, w:] == FILL), "apply wrote into the padding of its output's rows"
    return figures
