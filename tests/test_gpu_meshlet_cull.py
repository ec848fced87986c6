"""GPU: gr_meshlet_cull.  Every case of tests/golden/meshlet_cull_shader_v1.npz (the reference's meshlet_cull.comp executed on the CPU) in
every specialisation set -- phase 0 / 1 / 2 x ORTHO x SKINNED, FORCE_VISIBLE for phase 2 -- with no tolerance: the count word exact,
the records exact as a set sorted by (task_index, first_index), each task's records contiguous and in lane order, occluder words exact,
other lists' count words untouched, every dword past the last record still the poison byte.  Each case runs three times in one process,
so that the result cannot depend on the order in which waves arrive at the count word.

Beyond the golden, against tests/meshlet_cull_ref.py (which the generator holds to the executed shader): an output too small for its
records, device data that points outside its buffers, a depth hierarchy written by gr_hiz on the device, and every refusal of the
launcher."""
import ctypes as C

import numpy as np
import pytest

import meshlet_cull_cases as mc
import meshlet_cull_ref as ref
from granite_amd import capi, meshlet

pytestmark = pytest.mark.gpu
GOLDEN = mc.load_golden()


def upload(gr, scene, chain=None):
    return meshlet.CullScene(gr, scene["tasks"], scene["aabbs"], scene["transforms"], scene["bounds"], scene["draws"], scene["occluders"], scene["output"],
                             scene["chain"] if chain is None else chain, scene["chain_width"], scene["chain_height"], scene["chain_levels"])


def device_cull(device, scene, phase, flags):
    device.reset(scene["occluders"], scene["output"])
    for offset, count, mdi, draw in scene["dispatches"]:
        meshlet.cull(device, scene["frustum"], scene["camera"], phase, flags, int(offset), int(count), int(mdi), int(draw))
    return device.download()


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_golden_case_equals_the_executed_shader(gr, name):
    devices = {ortho: upload(gr, mc.golden_scene(GOLDEN, name, ortho)) for ortho in (False, True)}
    for phase, flags in mc.sets():
        ortho = bool(flags & ref.ORTHO)
        scene = mc.golden_scene(GOLDEN, name, ortho)
        want_output, want_occluders = mc.golden_result(GOLDEN, name, phase, flags)
        for run in range(3):
            output, occluders = device_cull(devices[ortho], scene, phase, flags)
            mc.assert_same(scene, output, occluders, want_output, want_occluders, f"{name} {mc.set_name(phase, flags)} run {run}")


def test_an_output_too_small_still_counts_every_survivor_and_writes_nothing_past_its_end(gr):
    for phase, flags in ((0, 0), (2, ref.ORTHO | ref.FORCE_VISIBLE), (1, ref.SKINNED)):
        scene = mc.random_scene(11, bool(flags & ref.ORTHO), tasks=70)
        full_output, _, _ = mc.run_reference(scene, phase, flags)
        survivors = int(full_output[0])
        assert survivors > 20
        # the device buffer is longer than output_dwords says: what lies past output_dwords must stay poison
        short = mc.COUNT_WORDS + 5 * (survivors // 2) + 3
        device = upload(gr, scene)
        device.reset(scene["occluders"], scene["output"])
        args = device.args(scene["frustum"], scene["camera"], phase, flags)
        args.output_dwords = short
        offset, count, mdi, draw = (int(v) for v in scene["dispatches"][0])
        gr.meshlet_cull(args, offset, count, mdi, draw)
        output, occluders = device.download()
        assert int(output[0]) == survivors, "the count includes the records that did not fit"
        assert np.all(output[short:] == ref.POISON_WORD), "dwords past output_dwords were written"
        assert np.all(output[mc.COUNT_WORDS + 5 * (survivors // 2):short] == ref.POISON_WORD), "a record that would end past output_dwords was written in part"
        fit = output[mc.COUNT_WORDS:mc.COUNT_WORDS + 5 * (survivors // 2)].reshape(-1, 5)
        every = {tuple(r) for r in ref.records(full_output, 0, mc.COUNT_WORDS)[1]}
        assert all(tuple(r) in every for r in fit) and len({tuple(r) for r in fit}) == len(fit), "the records that fit are survivors, each once"


def test_device_data_pointing_outside_its_buffers_is_not_visible_and_not_read(gr):
    for phase, flags in mc.sets():
        scene = mc.hostile_scene(bool(flags & ref.ORTHO))
        want_output, want_occluders, _ = mc.run_reference(scene, phase, flags)
        device = upload(gr, scene)
        output, occluders = device_cull(device, scene, phase, flags)
        mc.assert_same(scene, output, occluders, want_output, want_occluders, f"hostile {mc.set_name(phase, flags)}")


@pytest.mark.parametrize("ortho", [False, True])
def test_phase_2_over_a_hierarchy_written_by_gr_hiz(gr, ortho):
    """synthetic depth -> gr_hiz (output_downsample = 1) -> gr_meshlet_cull phase 2, against the restatement fed the downloaded chain"""
    width, height = mc.SCREENS["a"]
    depth = mc.synthetic_depth(width, height)
    image = capi.DeviceImage(gr, width, height, capi.FORMAT_R32_SFLOAT)
    image.upload(depth)
    chain, _, layout = gr.hiz(image, (1.0, 0.0, 0.0, 1.0), output_downsample=True)  # (num, den) = (depth, 1): the stored value is the depth
    gr.sync()
    assert (layout["chain_w"], layout["chain_h"], layout["levels"]) == mc.chain_shape(width, height)
    texels = sum(w * h for w, h in ref.level_sizes(layout["chain_w"], layout["chain_h"], layout["levels"]))
    flat = chain.download(np.float32, texels)
    scene = mc.random_scene(23, ortho, tasks=70, chain=(flat, layout["chain_w"], layout["chain_h"], layout["levels"]))
    flags = ref.ORTHO if ortho else 0
    want_output, want_occluders, info = mc.run_reference(scene, 2, flags)
    assert info["chunk_hiz_reject"] > 0 and info["chunk_hiz_accept"] > 0 and info["aabb_hiz_reject"] > 0
    device = upload(gr, scene, chain=chain)
    output, occluders = device_cull(device, scene, 2, flags)
    mc.assert_same(scene, output, occluders, want_output, want_occluders, "chained")


REFUSALS = [
    ("phase", lambda a, p: setattr(a, "phase", 3), "phase 3"),
    ("flags", lambda a, p: setattr(a, "flags", 8), "flags 0x8"),
    ("tasks null", lambda a, p: setattr(a, "tasks", None), "tasks is null"),
    ("aabbs misaligned", lambda a, p: setattr(a, "aabbs", a.aabbs + 4), "aabbs is not 16-byte aligned"),
    ("bounds misaligned", lambda a, p: setattr(a, "bounds", a.bounds + 8), "bounds is not 16-byte aligned"),
    ("transforms null", lambda a, p: setattr(a, "transforms", None), "transforms is null"),
    ("draws misaligned", lambda a, p: setattr(a, "draws", a.draws + 2), "draws is not 4-byte aligned"),
    ("output null", lambda a, p: setattr(a, "output", None), "output is null"),
    ("occluders missing", lambda a, p: setattr(a, "occluders", None), "occluders is null"),
    ("chain missing", lambda a, p: setattr(a, "chain", None), "chain is null"),
    ("hiz_resolution", lambda a, p: a.frustum.hiz_resolution.__setitem__(0, a.frustum.hiz_resolution[0] * 2), "frustum.hiz_resolution"),
    ("hiz_max_lod", lambda a, p: setattr(a.frustum, "hiz_max_lod", a.frustum.hiz_max_lod + 1), "frustum.hiz_max_lod"),
    ("hiz_min_lod", lambda a, p: setattr(a.frustum, "hiz_min_lod", -1), "frustum.hiz_min_lod"),
    ("mdi_count_offset", lambda a, p: setattr(p, "mdi_count_offset", a.output_dwords), "mdi_count_offset"),
    ("draw_indirect_offset", lambda a, p: setattr(p, "draw_indirect_offset", a.output_dwords), "draw_indirect_offset"),
]


@pytest.mark.parametrize("what,spoil,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_launcher_refuses_before_any_launch(gr, what, spoil, message):
    scene = mc.random_scene(5, False, tasks=8)
    device = upload(gr, scene)
    device.reset(scene["occluders"], scene["output"])
    args = device.args(scene["frustum"], scene["camera"], 2, 0)
    push = capi.PushMeshletCull(0, len(scene["tasks"]), 0, mc.COUNT_WORDS)
    spoil(args, push)
    code = gr.lib.gr_meshlet_cull(gr.handle, None, C.byref(args), C.byref(push))
    assert code == -1, (what, code)  # GR_ERR_INVALID_ARGUMENT
    text = gr.lib.gr_last_error(gr.handle).decode()
    assert text.startswith("gr_meshlet_cull: ") and message in text, text
    output, occluders = device.download()
    assert np.array_equal(output, scene["output"]) and np.array_equal(occluders, scene["occluders"]), "a refused call wrote something"


def test_count_zero_returns_ok_without_a_launch(gr):
    scene = mc.random_scene(5, False, tasks=8)
    device = upload(gr, scene)
    device.reset(scene["occluders"], scene["output"])
    args = device.args(scene["frustum"], scene["camera"], 2, 0)
    args.tasks = None  # not looked at: nothing is launched
    gr.meshlet_cull(args, 0, 0, 0, mc.COUNT_WORDS)
    output, _ = device.download()
    assert np.array_equal(output, scene["output"])
