"""CPU: which frames the fused bloom launches are offered for, pinned.

gr_bloom_down_mid_supported, gr_bloom_down_head_supported, gr_bloom_tail_supported, gr_bloom_up_all_supported and gr_bloom_pyramid_supported
take no context and touch no device.  tests/golden/bloom_supported.json holds their answers over a sweep of frames -- the five BASELINE
configs, every size tests/test_gpu_post.py runs, odd and even sizes around each size limit (65536 texels of downsample-1, 960 x 540 of
upsample-0, a 640 x 384 frame), both HDR formats, with and without the luminance reduction, and descriptors that break one rule each
(misaligned HDR pointer / pitch, equal pointers, no history, levels that are not half of their input) -- as the library answered before
the rules were gathered into one predicate each (tests/golden/make_bloom_supported_golden.py).  A frame that changes its answer changes
the launches it gets."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_bloom_supported_golden", os.path.join(GOLDEN, "make_bloom_supported_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_supported_queries_answer_as_pinned():
    # the queries' measurement switches are read from the environment on first use: the table is the product's behaviour
    for name in ("GR_NO_STENCIL", "GR_NO_MID_FUSION", "GR_MID_FUSION_ANY_SIZE", "GR_NO_HEAD_FUSION", "GR_NO_TAIL_FUSION", "GR_NO_UP_FUSION",
                 "GR_NO_PYRAMID_FUSION", "GR_PYRAMID_ANY_SIZE"):
        os.environ.pop(name, None)
    gen = _generator()
    doc = json.load(open(os.path.join(GOLDEN, "bloom_supported.json")))
    assert tuple(doc["functions"]) == gen.FUNCTIONS
    table = doc["answers"]
    # a table that only ever says "1" (or "0") for a query pins nothing
    for i, function in enumerate(gen.FUNCTIONS):
        assert {v[i] for v in table.values()} == {"0", "1"}, function
    from granite_amd import capi
    lib = capi.load_library()
    seen = 0
    wrong = []
    for name, images, lum in gen.cases():
        got = gen.answers(lib, images, lum)
        if got != table[name]:
            wrong.append((name, dict(zip(gen.FUNCTIONS, zip(table[name], got)))))
        seen += 1
    assert seen == len(table), (seen, len(table))
    assert not wrong, (len(wrong), wrong[:10])
