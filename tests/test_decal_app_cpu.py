"""CPU: volumetric decals in the application, under the device-less HIP stand-in of tests/hip_stub (tests/decal_app_worker.py).
With volumetric_decals = 1 the baked graph has three new edges into the G-buffer pass and a frame's launch list gains exactly the upload,
the decal binning (only with decals present), the decal z-range and the apply; with 0, graph and launch list are those of a configuration
that never names the field.  gra_set_decals refuses a decal that names a missing texture, gra_create the configurations decals are not
built for.  The host's packing -- sort order, slice intervals, mvps, world_to_texture -- equals tests/decal_ref.py bit for bit on two scenes of
tests/decal_cases.py handed over back to front."""
import re

import numpy as np
import pytest

import decal_cases as dc
import decal_ref as ref
from granite_amd import synth
from test_decal_abi_cpu import run_worker


@pytest.fixture(scope="module")
def worker():
    return run_worker("app", trace=True)


def launches(stderr, name):
    body = stderr.split(f"=== frame {name}\n")[1].split("=== end")[0]
    return [re.sub(r".*?(k_[a-z_0-9]+).*", r"\1", line.split(" ", 2)[2]) for line in body.splitlines() if line.startswith("L ")]


def test_off_is_the_configuration_without_the_field(worker):
    got, stderr = worker
    assert got["graphs"]["off"] == got["graphs"]["without_field"]
    assert launches(stderr, "off") == launches(stderr, "without_field")
    assert not any("decal" in k for k in launches(stderr, "off"))


def test_on_adds_three_edges_into_the_gbuffer_pass(worker):
    got, _ = worker
    off, on = got["graphs"]["off"], got["graphs"]["on_decals"]
    assert [p["name"] for p in on["passes"]] == [p["name"] for p in off["passes"]]
    for before, after in zip(off["passes"], on["passes"]):
        reads = lambda p: {r["name"] for r in p["reads"]}
        writes = lambda p: {r["name"] for r in p["writes"]}
        assert writes(after) == writes(before), after["name"]
        extra = reads(after) - reads(before)
        assert extra == ({"cluster-bitmask-decal", "cluster-range-decal", "cluster-transforms"} if after["name"] == "gbuffer-main" else set()), after["name"]
        assert reads(before) <= reads(after)
    order = [p["name"] for p in on["passes"]]
    assert order.index("clustering-bindless") < order.index("gbuffer-main") < order.index("lighting-main")
    assert got["graphs"]["on_no_decals"] == on, "the graph does not depend on how many decals are set"


def test_a_frame_gains_exactly_the_decal_launches(worker):
    _, stderr = worker
    base = launches(stderr, "off")
    with_decals, without = launches(stderr, "on_decals"), launches(stderr, "on_no_decals")

    def added(longer):
        rest = list(longer)
        for k in base:  # the frame's own launches are all there, in order
            assert k in rest, k
            del rest[:rest.index(k) + 1]
        extra = list(longer)
        for k in base:
            extra.remove(k)
        return extra

    assert added(with_decals) == ["k_upload_batch", "k_cluster_binning_decal", "k_cluster_z_range", "k_decal_apply"]
    assert added(without) == ["k_upload_batch", "k_cluster_z_range"], "no decals: the ranges are still cleared, nothing is binned or applied"
    assert with_decals.index("k_cluster_binning") < with_decals.index("k_cluster_binning_decal") < with_decals.index("k_decal_apply") < with_decals.index("k_lighting")


def test_refusals(worker):
    got, _ = worker
    assert re.search(r"decal 2 names texture 7, but only 1 are set", got["missing_texture"])
    for name in ("no_lighting", "row_bands", "aa_bench"):
        assert "volumetric_decals needs enable_lighting" in got["refused"][name], name


@pytest.mark.parametrize("name", ["three_overlap_odd", "many"])
def test_host_packing_equals_the_reference(worker, name):
    got, _ = worker
    state = {k: np.array(v) for k, v in got["state"][name].items()}
    case = dc.apply_case(name)
    cam = synth.Camera(case["width"], case["height"])
    rp = cam.render_params()
    handed = case["world_rows"][::-1]  # the worker hands the decals over back to front
    order = ref.host_sort_order(handed, rp[99:102])
    assert np.array_equal(state["order"], order)
    assert len(set(order.tolist())) == len(handed) and not np.array_equal(order, np.arange(len(handed))), "the hand-over order is not the sorted one"
    rows = handed[order]
    extent = ref.z_slice_extent(rp[103], dc.RES_Z)
    want_ranges = np.array([ref.compute_uint_range(*ref.decal_z_range(r, rp[96:99], rp[99:102]), extent, dc.RES_Z) for r in rows], np.uint32)
    assert np.array_equal(state["ranges"].astype(np.uint32), want_ranges)
    assert np.array_equal(state["mvps"].astype(np.float32), np.stack([ref.host_mvp(rp[32:48], r) for r in rows]))
    want = np.stack([ref.host_world_to_texture(r) for r in rows])
    assert np.array_equal(state["world_to_texture"].astype(np.float32).view(np.uint32), want.view(np.uint32))
