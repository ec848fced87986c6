"""What the ocean's test modules share: the golden of the reference's shaders executed on the CPU (tests/golden/ocean_shader_v1.npz), its
case lists, the inputs of a generate case and the Hermitian check."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ocean_shader_v1.npz"))
CASES = sorted({k.split("/")[0] for k in GOLDEN.files})
GENERATE = [c for c in CASES if c.startswith("generate_")]
BAKE = [c for c in CASES if c.startswith("bake_")]
MIPMAP = [c for c in CASES if c.startswith("mipmap_")]


def generate_inputs(name):
    push = GOLDEN[name + "/push"]
    nx, ny = int(push[2]), int(push[3])
    variant, bands = (int(v) for v in GOLDEN[name + "/spec"])
    return np.ascontiguousarray(GOLDEN["generate/distribution"][:ny, :nx]), push, variant, GOLDEN["generate/bands"] if bands else None


def hermitian_defect(out):
    """bins whose mirror is not their conjugate.  Bit for bit, except that an imaginary part of zero has the same sign on both sides
    (y - y is +0 whichever way round): zeros compare as values."""
    ny, nx = out.shape
    mirror = out[(ny - np.arange(ny)) & (ny - 1)][:, (nx - np.arange(nx)) & (nx - 1)]
    re, im, mre, mim = out & 0xffff, out >> 16, mirror & 0xffff, mirror >> 16
    zero = ((im & 0x7fff) == 0) & ((mim & 0x7fff) == 0)
    return int(np.count_nonzero((re != mre) | ((im != (mim ^ 0x8000)) & ~zero)))
