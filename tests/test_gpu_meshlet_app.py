"""GPU: gra_meshlet_decode and granite_amd.meshlet.decode on a written file equal the kernel-level result (gr_meshlet_decode on the same
streams, itself held to the executed shader by tests/test_gpu_meshlet_decode.py), and their indirect records equal the host arithmetic
of tests/test_meshlet_ref_cpu.py for both runtime styles; guard bytes in front of the push offsets come back as they went in."""
import numpy as np
import pytest

import meshlet_cases as mc
import meshlet_ref as mr
from granite_amd import app as gapp
from granite_amd import meshlet
from meshlet_device import device_decode

pytestmark = pytest.mark.gpu
COUNTS = [(i % 3 + 1, i % 4 + 2) for i in range(17)] + [(32, 32), (0, 0), (31, 1)]


def test_app_decode_equals_the_kernel_and_the_host_arithmetic(gr, tmp_path):
    path = str(tmp_path / "mesh.msh4")
    data = mc.random_file(2026, 2, COUNTS, padding=False)
    open(path, "wb").write(data)
    mesh = mr.parse(data)
    counts = mr.counts_of(mesh["streams"])
    a = gapp.Application(64, 64, lighting=False)
    try:
        for target, flags, runtime, po, vo in ((2, 0, meshlet.RUNTIME_MDI, 0, 0), (2, mr.INDEX_16, meshlet.RUNTIME_MESHLET, 11, 5),
                                               (1, mr.UNROLLED_MESH, meshlet.RUNTIME_MDI, 11, 5), (0, mr.INDEX_16, meshlet.RUNTIME_MDI, 0, 3)):
            got = meshlet.decode(a, path, target, flags, runtime, po, vo, guard=mr.GUARD)
            caps = (po + int(counts[:, 0].sum()), vo + int(counts[:, 1].sum()))
            offs = mr.offsets(counts, runtime, flags)
            want, _ = device_decode(gr, mesh["streams"], mesh["payload"], offs, po, vo, target, flags, caps)
            ref = mr.decode(mesh["streams"], mesh["payload"], offs, po, vo, target, flags, caps)
            for key in ("indices", "positions", "attributes", "skin"):
                assert np.array_equal(want[key], ref[key]), (target, flags, key)
                if key in got:
                    assert np.array_equal(got[key].reshape(-1).view(np.uint8), want[key]), (target, flags, runtime, key)
            assert set(got) == {"indices", "positions", "indirect"} | ({"attributes"} if target >= 1 else set()) | ({"skin"} if target >= 2 else set())
            assert np.all(got["indices"][:po].view(np.uint8) == mr.GUARD) and np.all(got["positions"][:vo].view(np.uint8) == mr.GUARD)
            assert np.array_equal(got["indirect"], mr.indirect(counts, runtime, po, vo)), (runtime, po, vo)
        info = meshlet.describe(path)
        assert (info.meshlet_count, info.chunk_count, info.total_primitives, info.total_vertices) == (20, 3, int(counts[:, 0].sum()), int(counts[:, 1].sum()))
        with pytest.raises(Exception, match="target_style"):
            open(path, "wb").write(mc.random_file(1, 0, [(2, 3)]))
            meshlet.decode(a, path, target_style=1)
    finally:
        a.close()
