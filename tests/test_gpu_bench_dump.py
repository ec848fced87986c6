"""bench.py --dump-outputs: what the last timed frame delivered, written as float32 .npy, the same from run to run with the same
arguments (seeded inputs, a fixed number of frames in front of the dump), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3",
                        "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("workload,shape", [("config3_4k_4096lights", (1 << 20, 4)), ("config3_4k_4096lights_b10g11r11", (1 << 20, 4)),
                                            ("config1_256_post_only", (256, 256, 4))])
def test_two_runs_dump_the_same_outputs(tmp_path, workload, shape):
    docs = [run_bench(tmp_path / f"run{i}", "--workload", workload) for i in range(2)]
    for doc in docs:
        assert doc["steps"] == 10 and doc["ms_per_step"] > 0 and doc["roofline"] is None
    names = sorted(os.listdir(tmp_path / "run0"))
    assert names == ["average_luminance.npy", "backbuffer.npy", "hdr_main.npy"]
    assert sum(os.path.getsize(tmp_path / "run0" / n) for n in names) <= 64 << 20
    for name in names:
        a, b = np.load(tmp_path / "run0" / name), np.load(tmp_path / "run1" / name)
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        if name != "average_luminance.npy":
            assert a.shape == shape, (name, a.shape)
        np.testing.assert_array_equal(a, b, err_msg=f"{workload}: {name} differs between two runs")
    bb = np.load(tmp_path / "run0" / "backbuffer.npy")
    assert bb.min() >= 0 and bb.max() <= 255 and bb.max() > bb.min()
