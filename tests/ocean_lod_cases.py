"""What the LOD update's test modules share: the golden of the reference's shaders executed on the CPU
(tests/golden/ocean_lod_shader_v1.npz), its case list, and the comparisons every layer is held to."""
import os

import numpy as np

import ocean_lod_ref as olr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ocean_lod_shader_v1.npz"))
CASES = sorted({k.split("/")[0] for k in GOLDEN.files if k.startswith("lod_")})
SMALL = [c for c in CASES if not c.startswith("lod_g64")]


def spec(name):
    gc, gr, fixed, wrap = (int(v) for v in GOLDEN[name + "/spec"])
    return gc, gr, fixed, wrap


def golden_buckets(name):
    """the golden's patches split back into its eight sorted buckets"""
    counts = GOLDEN[name + "/draws"][:, 1]
    flat, out, at = GOLDEN[name + "/patches"], [], 0
    for c in counts:
        out.append(flat[at:at + int(c)])
        at += int(c)
    return out


def assert_lods(name, image, what):
    """byte-identical to the golden outside the near-tie mask, at most one fp16 code inside it; -> number of differing texels"""
    golden = GOLDEN[name + "/lods"]
    mask = olr.near_tie_mask(GOLDEN[name + "/lod64"])
    image = np.asarray(image, np.uint16).reshape(golden.shape)
    differ = image != golden
    assert not np.any(differ & ~mask), (what, name, np.argwhere(differ & ~mask)[:4])
    assert np.all(np.abs(image.astype(np.int32) - golden.astype(np.int32)) <= 1), (what, name)
    return int(differ.sum())


def assert_cull(name, draws, patch_buffer, what):
    """counters exact, patches exact as sorted sets per bucket"""
    gc = spec(name)[0]
    draws = np.asarray(draws, np.uint32).reshape(8, 8)
    assert np.array_equal(draws, GOLDEN[name + "/draws"]), (what, name, draws[:, 1], GOLDEN[name + "/draws"][:, 1])
    got = olr.buckets_of(patch_buffer, draws, gc * gc)
    for l, (a, b) in enumerate(zip(got, golden_buckets(name))):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, name, l)
