"""CPU: the executor hands the HIP runtime the calls it handed it before stream planning and cross-stream hazard tracking moved out of
render_graph.cpp (granite_amd/csrc/host/frame_schedule.cpp) -- every launch run, event record, stream wait, event query and host wait, in
order, on the same streams and events, and under GRANITE_SYNC_DEBUG=1 the same "[sync]" lines.

tests/golden/executor_call_stream_parent.json was recorded under tests/hip_stub with the library of the commit before the move
(tests/golden/make_executor_call_stream_golden.py: the cases, the normal form, and how it was recorded twice and compared).  The comparison
is exact.  It also holds what every graph of the cases bakes to: stream per pass, hand-over rings, aliases."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

spec = importlib.util.spec_from_file_location("make_executor_call_stream_golden", os.path.join(GOLDEN, "make_executor_call_stream_golden.py"))
recorder = importlib.util.module_from_spec(spec)
spec.loader.exec_module(recorder)


@pytest.fixture(scope="module")
def parent():
    with open(recorder.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def graph_cases(tmp_path_factory):
    return recorder.build_tools("lib", str(tmp_path_factory.mktemp("executor_call_stream")))


def test_the_fixture_holds_every_case(parent):
    assert sorted(parent) == sorted(recorder.CASES)
    # 40 and 12 random graphs, each pipelined and serial; one graph per application process
    assert len(parent["execute40_pending"]) == 80 and len(parent["execute_blit12_pending"]) == 24
    assert all(len(sections) == 1 for name, sections in parent.items() if not name.startswith("execute"))
    # the cases do reach the paths they are there for
    assert any(s["graph"]["streams"][-1] == ["final", "async"] for s in parent["execute_blit12_pending"].values())
    debug = parent["taa_smaa_pending_granite_sync_debug"]["taa_smaa frames"]["calls"]
    assert sum(l.startswith("[sync]") for l in debug) >= 20
    assert any(l.startswith("G ") for l in parent["taa_smaa_pending_granite_launch_graphs"]["taa_smaa frames"]["calls"])
    assert sum(l.startswith("W ") for s in parent["execute40_pending"].values() for l in s["calls"]) >= 400


@pytest.mark.parametrize("name", sorted(recorder.CASES))
def test_call_stream_is_the_parents(name, parent, graph_cases):
    got = recorder.record(name, graph_cases)
    assert sorted(got) == sorted(parent[name])
    for section in parent[name]:
        assert got[section]["graph"] == parent[name][section]["graph"], section
        want, have = parent[name][section]["calls"], got[section]["calls"]
        first = next((i for i, (a, b) in enumerate(zip(want, have)) if a != b), min(len(want), len(have)))
        assert have == want, (section, "first difference at line %d of %d / %d" % (first, len(want), len(have)), want[max(first - 5, 0):first + 5], have[max(first - 5, 0):first + 5])
