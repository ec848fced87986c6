"""GPU: the cluster-build kernels on lights around, behind and beside the camera (tests/cluster_cases.py) -- against the oracle
bit for bit (a NaN for a NaN in the set-up records), against float64 geometry, through the lighting kernel and through the host
layer's packing.  tests/test_cluster_cases_cpu.py holds the oracle to the reference's executed shaders on the same cases."""
import os

import numpy as np
import pytest

from granite_amd import app as gapp, capi, synth
from oracle import oracle as orc
import cluster_cases as cc
from gpu_scene import Scene
from util import assert_rgba16f_close, assert_words_equal_or_both_nan

pytestmark = pytest.mark.gpu

os.environ.setdefault("GRANITE_LIGHT_PREFETCH_MIN", "0")  # as tests/test_gpu_app.py: read once per process

NAMES = [n for n in cc.CASES if n != "box_dim"]
FULL = ("box_around_camera",) + tuple(f"counts_{n}" for n in cc.COUNTS)
BUILDS = [(name, res) for name in NAMES for res in (cc.RES, cc.RES_SMALL) + ((cc.RES_FULL,) if name in FULL else ())]


def download(sc, dev):
    n32 = (sc.n + 31) // 32
    return {"spots": dev["spots"].download(np.uint32), "setup": dev["setup"].download(np.uint32),
            "range": dev["range"].download(np.uint32).reshape(-1, 2), "bitmask": dev["bitmask"].download(np.uint32)[:sc.res[0] * sc.res[1] * n32]}


@pytest.mark.parametrize("name,res", BUILDS, ids=[f"{n}-{r[0]}x{r[1]}x{r[2]}" for n, r in BUILDS])
def test_kernels_equal_the_oracle(gr, name, res):
    """The launch-by-launch build and gr_cluster_front in its buffer and its pinned form: ranges and bitmask exactly, spots and set-up
    as words with NaN == NaN (cluster_cases.compare_cluster_build)."""
    cam, descs = cc.case(name)
    ref = cc.built(name, res)
    sc = Scene.from_camera(cam, descs, res)
    assert sc.n == ref["n"]
    for what, dev in (("launch by launch", sc.build_clusters_gpu(gr)), ("front, buffers", sc.build_clusters_gpu_fused(gr, False)),
                      ("front, pinned", sc.build_clusters_gpu_fused(gr, True))):
        got = download(sc, dev)
        excepted = cc.compare_cluster_build(got, ref, sc.n, what=f"{name} {res} {what}")
        nan = got["setup"].reshape(-1, 128)[:sc.n]
        nan = nan[np.isnan(nan.view(np.float32)) & (np.arange(128)[None, :] % 128 != 3)]
        print(f"{name} {res} {what}: {excepted} words equal only as NaN; NaN patterns written: {sorted({hex(v) for v in nan.tolist()})}")


@pytest.mark.parametrize("name", ["box_around_camera", "camera_oblique"])
def test_gpu_masks_and_ranges_are_conservative_against_float64_geometry(gr, name):
    """cluster_cases.conservativeness (shrink 0.98, zero misses) on what the kernels wrote."""
    cam, descs = cc.case(name)
    sc = Scene.from_camera(cam, descs, cc.RES)
    got = download(sc, sc.build_clusters_gpu(gr))
    c = cc.conservativeness(cc.built(name), got["bitmask"], got["range"])
    print(name, c)
    assert c["point"][0] > 1000 and c["spot"][0] > 1000
    assert c["point"][1] == 0 and c["spot"][1] == 0, c


def test_lighting_through_the_clusters_of_lights_around_the_camera(gr):
    """box_dim under the far = 20 camera at 256 x 128: gr_lighting's clustered sum against the oracle's brute-force sum over all lights
    (2 ulp fp16, as test_lighting_equals_bruteforce_sum) and against the oracle's clustered result (2 ulp + 1e-4); on the CPU the two
    oracle results are equal bit for bit (test_cluster_cases_cpu.py)."""
    cam, descs = cc.case("box_dim")
    sc = Scene.from_camera(cam, descs)
    dev = sc.build_clusters_gpu(gr)
    ref_c = orc.cluster_build(sc.rp, sc.prm, sc.lights, sc.model, sc.type_mask, sc.n, sc.res[2])
    args = (sc.gbuf, sc.rp, sc.prm, sc.lights, sc.type_mask)
    brute = orc.lighting(*args, np.zeros(1, np.uint32), np.zeros((1, 2), np.uint32), synth.DIRECTIONAL_COLOR, synth.DIRECTIONAL_DIRECTION,
                         directional=False, bruteforce=True)
    clustered = orc.lighting(*args, ref_c["bitmask"], ref_c["range"], synth.DIRECTIONAL_COLOR, synth.DIRECTIONAL_DIRECTION, directional=False)
    largs, imgs = sc.lighting_args(gr, dev, capi.LIGHTING_CLUSTERED_BIT)
    gr.check(gr.lib.gr_lighting(gr.handle, None, largs))
    gr.sync()
    got = imgs["hdr"].download()
    assert_rgba16f_close(got, brute, ulps=2.0, what="clustered vs brute force")
    assert_rgba16f_close(got, clustered, ulps=2.0, abs_tol=1e-4, what="clustered vs the oracle's clustered result")


def test_host_packing_and_cluster_build_of_lights_around_the_camera():
    """gapp.Application with box_around_camera's camera and lights, one frame: lights.cpp / clusterer.cpp packing and slice intervals
    (lights behind the camera included), the kernels' bitmask, ranges and set-up records, against the oracle."""
    cam, descs = cc.case("box_around_camera")
    ref = cc.built("box_around_camera", cc.RES_FULL)
    a = gapp.Application(cam.width, cam.height)
    a.set_render_parameters(cam.render_params())
    a.set_lights(descs)
    a.upload_gbuffer(synth.make_gbuffer(cam))
    a.render_frames(1)
    st = a.cluster_state()
    n = ref["n"]
    assert st["count"] == n
    np.testing.assert_array_equal(st["lights"][:n * 48], ref["lights"].view(np.uint8)[:n * 48])
    np.testing.assert_array_equal(st["models"][:n].view(np.uint32), ref["model"][:n].view(np.uint32))
    np.testing.assert_array_equal(st["type_mask"], ref["type_mask"])
    np.testing.assert_array_equal(st["params"], ref["prm"].view(np.uint8).reshape(-1))
    np.testing.assert_array_equal(st["light_ranges"], ref["light_ranges"])
    n32 = (n + 31) // 32
    np.testing.assert_array_equal(a.read("cluster-bitmask").view(np.uint32)[:128 * 64 * n32], ref["bitmask"])
    np.testing.assert_array_equal(a.read("cluster-range").view(np.uint32).reshape(-1, 2), ref["range"])
    integer = np.zeros((n, 128), bool)
    integer[:, 3] = True
    setup = a.read("cluster-cull-setup").view(np.uint32).reshape(-1)[:n * 128].reshape(n, 128)
    excepted = assert_words_equal_or_both_nan(setup, ref["setup"][:n], integer_words=integer, what="cluster-cull-setup")
    assert excepted <= int(np.isnan(ref["setup"][:n]).sum())
    a.close()
