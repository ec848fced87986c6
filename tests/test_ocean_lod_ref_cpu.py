"""CPU: tests/ocean_lod_ref.py -- the numpy restatement of update_lod.comp, init_counter_buffer.comp and cull_blocks.comp and of the mesh
builders -- against the golden of the executed shaders (tests/golden/ocean_lod_shader_v1.npz): LOD images byte for byte, counters exactly,
patches exactly after sorting each bucket's first instance_count entries by offsets (slots past instance_count are never read).  Then the
meshes: counts from the loops, restart placement, the weight rule, and a hand-written known answer for grid_count = grid_resolution = 4."""
import numpy as np
import pytest

import ocean_lod_ref as olr
from ocean_lod_cases import CASES, GOLDEN, golden_buckets, spec


def test_the_golden_has_the_cases_the_generator_promises():
    assert len(CASES) == 3 * (4 * 3 - 1) * 2 + 1
    for gc in (4, 8, 16):
        for camera in ("origin", "negative", "up", "far"):
            for frustum in ("all", "perspective", "none"):
                for mode in ("moving", "fixed"):
                    assert (f"lod_g{gc}_{camera}_{frustum}_{mode}" in CASES) == ((camera, frustum) != ("far", "perspective"))
    assert "lod_g64_default_origin_all_moving" in CASES
    # the kinds: a negative image_offset, every LOD at max_lod, a frustum that keeps about half, one that keeps nothing, several waves into a bucket
    assert np.all(GOLDEN["lod_g16_negative_all_moving/update_push"][4:6].view(np.int32) < 0)
    up = GOLDEN["lod_g16_up_all_moving/lods"]
    assert np.all(up.view(np.float16) == 6.0)
    kept = int(GOLDEN["lod_g16_origin_perspective_fixed/draws"][:, 1].sum())
    assert 256 // 4 <= kept <= 3 * 256 // 4
    assert GOLDEN["lod_g16_origin_none_moving/draws"][:, 1].sum() == 0
    assert GOLDEN["lod_g16_origin_all_moving/draws"][:, 1].max() > 64


@pytest.mark.parametrize("name", CASES)
def test_update_lod(name):
    image, _ = olr.update_lod(GOLDEN[name + "/update_push"])
    assert np.array_equal(image, GOLDEN[name + "/lods"])
    _, lod64 = olr.update_lod(GOLDEN[name + "/update_push"], np.float64)
    assert np.array_equal(lod64, GOLDEN[name + "/lod64"])
    assert olr.near_tie_mask(lod64).mean() <= 0.02


def test_init_counters():
    assert np.array_equal(olr.init_counters(GOLDEN["init/counts16"]), GOLDEN["init/draws"])
    assert np.all(GOLDEN["init/draws"][:, 1:] == 0) and np.array_equal(GOLDEN["init/draws"][:, 0], GOLDEN["init/counts16"][:8])


@pytest.mark.parametrize("name", CASES)
def test_cull_blocks(name):
    _, _, _, wrap = spec(name)
    draws, patches = olr.cull_blocks(GOLDEN[name + "/lods"], GOLDEN[name + "/cull_push"], GOLDEN[name + "/frustum"], wrap, GOLDEN["init/draws"])
    assert np.array_equal(draws, GOLDEN[name + "/draws"])
    for l, (a, b) in enumerate(zip(patches, golden_buckets(name))):
        assert np.array_equal(olr.sorted_bucket(a).view(np.uint32), b.view(np.uint32)), l
    # every patch's bucket is at most each of its edge LODs and its inner LOD
    for l, b in enumerate(golden_buckets(name)):
        assert np.all(b[:, 4:8] >= l) and np.all(b[:, 2] >= l) and np.all(b[:, 3] == 0)


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("lod_g16")])
def test_pushes_are_the_hosts_derivation(name):
    gc, gr, fixed, wrap = spec(name)
    cfg = GOLDEN[name + "/config"]
    pushes = olr.pass_pushes(gc, gr, cfg[0:2], cfg[2], cfg[3:6], bool(fixed), cfg[6:9])
    assert np.array_equal(pushes["update"], GOLDEN[name + "/update_push"]) and np.array_equal(pushes["cull"], GOLDEN[name + "/cull_push"])
    assert pushes["wrap"] == wrap == (0 if fixed else 1)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_resolution", [4, 32, 128])
def test_lod_meshes(grid_resolution):
    meshes = olr.lod_meshes(grid_resolution)
    assert len(meshes) == olr.lod_count(grid_resolution) <= olr.MAX_LOD_INDIRECT
    for level, (vertices, indices) in enumerate(meshes):
        size, stride = grid_resolution >> level, 1 << level
        assert vertices.shape == ((size + 1) ** 2, 8) and indices.shape == (size * (2 * (size + 1) + 1),)
        # one restart after every strip of 2 (size + 1) indices, and nowhere else
        rows = indices.reshape(size, 2 * (size + 1) + 1)
        assert np.all(rows[:, -1] == olr.RESTART) and np.all(rows[:, :-1] < len(vertices))
        assert np.array_equal(rows[:, 0:-1:2], np.arange(size * (size + 1)).reshape(size, size + 1))
        assert np.array_equal(rows[:, 1:-1:2], rows[:, 0:-1:2] + size + 1)
        x, y = vertices[:, 0].astype(int), vertices[:, 1].astype(int)
        assert np.array_equal(x, np.tile(np.arange(size + 1) * stride, size + 1)) and np.array_equal(y, np.repeat(np.arange(size + 1) * stride, size + 1))
        assert np.array_equal(vertices[:, 2], x < grid_resolution // 2) and np.array_equal(vertices[:, 3], y < grid_resolution // 2)
        # the weight rule: x edges win over y edges, so a corner belongs to its x edge; at most one weight is set
        w = vertices[:, 4:8]
        assert np.array_equal(w[:, 0] == 255, x == 0) and np.array_equal(w[:, 1] == 255, x == grid_resolution)
        assert np.array_equal(w[:, 2] == 255, (y == 0) & (x != 0) & (x != grid_resolution))
        assert np.array_equal(w[:, 3] == 255, (y == grid_resolution) & (x != 0) & (x != grid_resolution))
        assert set(np.unique(w)) <= {0, 255} and np.all((w == 255).sum(1) <= 1)


@pytest.mark.parametrize("gc,gr", [(4, 4), (16, 32), (64, 128)])
def test_border_mesh_counts(gc, gr):
    positions, indices = olr.border_mesh(gc, gr)
    assert len(positions) == 4 * (2 * gc + 1) * 2 + 16 + 4 * (2 * gc + 3) * 2
    assert len(indices) == len(positions) + 12 and np.count_nonzero(indices == olr.RESTART) == 12
    used = indices[indices != olr.RESTART]
    assert np.array_equal(used, np.arange(len(positions)))  # every position once, in order
    restarts = np.flatnonzero(indices == olr.RESTART)
    assert np.array_equal(np.diff(np.concatenate([[-1], restarts])) - 1, [(2 * gc + 1) * 2] * 4 + [4] * 4 + [(2 * gc + 3) * 2] * 4)
    assert olr.border_mesh(gc, gr, fixed_position=True)[0].shape == (0, 3)
    plane, plane_indices = olr.border_mesh(8, 1024, heightmap=False, fixed_position=True)
    assert plane.shape == (17 * 17, 3) and len(plane_indices) == 16 * (2 * 17 + 1) and np.all(plane[:, 2] == 1.0)
    assert plane[:, 0].max() == 16 * 512


def test_known_answer_grid_4_by_4():
    (v0, i0), (v1, i1) = olr.lod_meshes(4)
    # LOD 1: a 2 x 2 quad mesh of stride 2 over 0 .. 4
    assert v1.tolist() == [[0, 0, 1, 1, 255, 0, 0, 0], [2, 0, 0, 1, 0, 0, 255, 0], [4, 0, 0, 1, 0, 255, 0, 0],
                           [0, 2, 1, 0, 255, 0, 0, 0], [2, 2, 0, 0, 0, 0, 0, 0], [4, 2, 0, 0, 0, 255, 0, 0],
                           [0, 4, 1, 0, 255, 0, 0, 0], [2, 4, 0, 0, 0, 0, 0, 255], [4, 4, 0, 0, 0, 255, 0, 0]]
    assert i1.tolist() == [0, 3, 1, 4, 2, 5, 0xffff, 3, 6, 4, 7, 5, 8, 0xffff]
    assert v0[:6].tolist() == [[0, 0, 1, 1, 255, 0, 0, 0], [1, 0, 1, 1, 0, 0, 255, 0], [2, 0, 0, 1, 0, 0, 255, 0], [3, 0, 0, 1, 0, 0, 255, 0],
                               [4, 0, 0, 1, 0, 255, 0, 0], [0, 1, 1, 1, 255, 0, 0, 0]]
    assert i0[:11].tolist() == [0, 5, 1, 6, 2, 7, 3, 8, 4, 9, 0xffff]
    positions, indices = olr.border_mesh(4, 4)
    # top border: from (16, 0) leftwards in steps of 2, each with its outer partner 2 (= 16 >> 3) above; the inner vertex carries z = 1
    assert positions[:4].tolist() == [[16, 0, 1], [16, -2, 0], [14, 0, 1], [14, -2, 0]]
    assert positions[16:18].tolist() == [[0, 0, 1], [0, -2, 0]] and indices[:18].tolist() == list(range(18)) and indices[18] == 0xffff
    # left border starts at the origin and runs down
    assert positions[18:22].tolist() == [[0, 0, 1], [-2, 0, 0], [0, 2, 1], [-2, 2, 0]]
    # top-left corner
    corner = 4 * 18
    assert positions[corner:corner + 4].tolist() == [[0, 0, 1], [0, -2, 0], [-2, 0, 0], [-2, -2, 0]]
    # top outer ring: the first inner vertex steps out by the corner delta, its partner is the far corner of the +-32768 square
    ring = corner + 16
    assert positions[ring:ring + 4].tolist() == [[18, -2, 0], [32784, -32768, 0], [16, -2, 0], [26229, -32768, 0]]  # 32784 * 0.9 - 32768 * 0.1 = 26228.8
    assert positions[ring + 20:ring + 22].tolist() == [[-2, -2, 0], [-32768, -32768, 0]]
    assert olr.draw_data(128, 4, 4, (64.0, 64.0), 7.3, (0, 0, 0), (-8, 12)).tolist() == pytest.approx(
        [0, 0, 0, 0, -8, 12, 1 / 128, 1 / 128, 1 / 16, 1 / 16, 7.3, 7.3, 4, 4, -10, 10])
