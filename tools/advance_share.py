"""The advance overlap on the bench's C4 workload, one process, one library: alternating rounds of the timed
region (warm state reset, start states, 2 warm-up steps, 10 timed steps in one dat_closed_loop call) with the
overlap off and on -- ms per step, k_cadmm ms per launch, and the early share of the scenario-steps
(dat_get_advance_counts); the states the two leave must be bitwise equal.

    python tools/advance_share.py [rounds] [batch]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from distributed_aerial_transportation_amd import BatchedController, scenarios  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
n, steps, warmup = 6, 10, 2
scen_forest, states, forests = bench.bench_states(n, B, 0, 1, 64, "path", B)
eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
eng.set_forests(forests, scen_forest)
last = {}
for r in range(rounds):
    for on in (False, True):
        eng.set_advance_overlap(on)
        eng.reset_warm_start()
        eng.set_state(states, np.zeros(B, dtype=np.int32))
        eng.closed_loop(warmup)
        eng.reset_counters()
        eng.synchronize()
        t0 = time.perf_counter()
        eng.closed_loop(steps)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        per = np.diff(eng.step_marks())
        early, late = eng.advance_counts()
        st, cnt = eng.get_state()
        if on in last:
            assert np.array_equal(last[on][0], st) and np.array_equal(last[on][1], cnt), "run-to-run difference"
        last[on] = (st, cnt)
        print(f"round {r} overlap {'on ' if on else 'off'}: {ms:.4f} ms/step  p50 {np.median(per):.3f}  max {per.max():.3f}  "
              f"k_cadmm {eng.kernel_ms() / steps:.4f} ms/launch  early {early}  late {late}  "
              f"early share {early / max(early + late, 1):.3f}", flush=True)
assert np.array_equal(last[False][0], last[True][0]) and np.array_equal(last[False][1], last[True][1]), "on != off"
print("states and rotation counters after the timed steps: overlap on == off, bitwise, every round")
