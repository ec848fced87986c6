"""Random frame graphs EXECUTED on the three-stream executor (tests/cpp/graph_cases.cpp --execute): every pass hashes its inputs
into its outputs (gr_debug_mix), four frames are enqueued back to back with no host synchronisation, and the swapchain images
must equal those of a serial run of the same graph (every pass on the graphics queue, nothing hoisted, nothing aliased).  A pass
that ran before a producer, a recycled allocation still in use, or a wrong copy of a hand-over ring changes the hash.
(Sensitivity, measured once: with the executor's cross-stream waits switched off -- GRANITE_UNSAFE_NO_CROSS_SYNC=1 -- 33 of the
40 graphs produce different frames.)"""
import json

import pytest

from host_program import PRODUCT, build_program, run_program

pytestmark = pytest.mark.gpu


def test_pipelined_execution_of_random_graphs_equals_serial_execution(tmp_path):
    exe = build_program(tmp_path, "graph_cases", "graph_cases.cpp", extra=PRODUCT)
    cases = list(map(json.loads, run_program(exe, "--execute", 40, timeout=300).splitlines()))
    assert len(cases) == 40
    seen = set()
    for c in cases:
        assert c["pipelined"] == c["serial"], c["case"]
        assert len(set(c["pipelined"])) == 4, c["case"]   # the frame number is part of every pass's salt
        seen.update(c["pipelined"])
    assert len(seen) == 160
