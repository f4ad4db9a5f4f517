"""Fixture ref_track.npz: the oracle's controllers flying the reference's circle (the trajectory-tracking law of
test/control/test_rqpcontrollers.py:24-48) in closed loop from the rest state, without a forest -- the loop of
tests/_track.py, which uses the oracle alone (oracle/controllers.py, oracle/model.py).  Read by
tests/test_track_fixture.py and tests/test_gpu_tracking.py.

Cases (tests/_track.py CASES): C-ADMM n = 3 and n = 6, DD n = 3, centralized n = 3; 40 HL steps at n = 3, 20 at n = 6.
Per HL step acc_des, f_des, iters and err_seq, and the state after each HL period, at IPM tolerance 1e-11 (the
fixture's) and 1e-10 (`*_1e10`); the difference between the two gives sens_f and count_moves per step and the
loop's state_spread, as make_dd_long.py does.

    python tests/golden/make_track.py [case ...]       (about 2 s per loop)
"""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "ref_track.npz")


def _job(job):
    from tests import _track

    return _track.run(*job)


def main():
    from tests import _track

    names = sys.argv[1:] or list(_track.CASES)
    old = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    with mp.Pool(min(8, os.cpu_count() or 1)) as workers:
        res = workers.map(_job, [(name, tol) for name in names for tol in (1e-11, 1e-10)])
    for j, name in enumerate(names):
        r11, r10 = res[2 * j], res[2 * j + 1]
        sf, cm, spread = _track.sensitivities(r11, r10)
        d = dict(r11)
        d.update({k + "_1e10": r10[k] for k in ("f_des", "iters", "state")})
        d.update(sens_f=sf, count_moves=cm, state_spread=np.float64(spread))
        old = {k: v for k, v in old.items() if not k.startswith(name + "_")}
        old.update({f"{name}_{k}": v for k, v in d.items()})
        it = r11["iters"]
        print(f"{name}: passes first step {int(it[0])}, afterwards {int(it[1:].min())}-{int(it[1:].max())}; sens_f max "
              f"{np.nanmax(sf):.3g}, count moves {int(cm.sum())}, state spread {spread:.3g}", flush=True)
    np.savez_compressed(OUT, **old)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
