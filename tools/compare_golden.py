"""python tools/compare_golden.py a.npz b.npz: the same keys, and per key the same dtype, shape and bytes (so that NaNs count)."""
import sys

import numpy as np

a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
for key in a.files:
    x, y = a[key], b[key]
    assert (x.dtype, x.shape) == (y.dtype, y.shape) and x.tobytes() == y.tobytes(), key
print(f"{sys.argv[1]} == {sys.argv[2]}: {len(a.files)} arrays")
