"""Bitwise comparison of bench.py --dump-outputs directories: every array of the first directory must be
np.array_equal to the array of the same name in each of the others.

    python tools/same_dumps.py DIR DIR [DIR ...]
"""
import os
import sys

import numpy as np

ref, bad = sys.argv[1], 0
names = sorted(f for f in os.listdir(ref) if f.endswith(".npy"))
assert names, ref
for other in sys.argv[2:]:
    assert sorted(f for f in os.listdir(other) if f.endswith(".npy")) == names, (ref, other)
    for f in names:
        a, b = np.load(os.path.join(ref, f)), np.load(os.path.join(other, f))
        same = a.shape == b.shape and np.array_equal(a, b)
        bad += not same
        print(f"{'equal' if same else 'DIFFERENT':>9}  {f:<20} {a.shape}  {ref}  {other}")
sys.exit(1 if bad else 0)
