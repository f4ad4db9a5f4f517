"""Does the host build of the QP solvers give the same bits in two builds?  Runs the agent-QP checks of
tests/test_hostsim.py -- the C-ADMM, DD and centralized QPs against the oracle, the C4 stall stretches of
ref_c4_hard.npz (whole C-ADMM steps: cold, tuned and warm solves through the tail rule), the captured loose QPs of
ref_loose_caps.npz and the host DD steps -- once with each of two builds of tests/hostsim/hostsim.hip,

    hipcc -O2 -std=c++17 -fPIC -shared --offload-arch=gfx950 tests/hostsim/hostsim.hip -o X.so

and compares everything every solve returned, bit for bit: the solution, status, iterations, the in-band flag,
last_diag(), last_work(), last_stiff() and the warm-start record.

    python tools/same_hostsim.py A.so B.so

One line per entry point; exit status 1 on any difference.  (Each build runs in a process of its own:
`same_hostsim.py --record X.so OUT` writes the record.)
"""
import os
import pickle
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("qp_cadmm", "qp_cadmm_ex", "qp_cadmm_warm", "qp_dd", "qp_cent", "dd_step", "cadmm_step")
TESTS = ("test_reduced_cadmm_qp_matches_oracle", "test_reduced_dd_qp_matches_oracle",
         "test_reduced_centralized_qp_matches_oracle", "test_c4_stall_stretch_matches_oracle",
         "test_c4_tail_record_rule_at_the_handover_pass", "test_loose_caps_solved_within_clarabel_tol",
         "test_host_dd_step_golden", "test_host_dd_step_matches_oracle",
         "test_host_dd_long_chains_match_oracle")


def bits(x):
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return np.float64(x).tobytes()
    if isinstance(x, (tuple, list)):
        return tuple(bits(v) for v in x)
    if hasattr(x, "__dict__"):
        return tuple((k, bits(v)) for k, v in sorted(vars(x).items()))
    return x


def record(lib, out):
    sys.path.insert(0, ROOT)
    import pytest

    import tests.hostsim as hs
    import tests.test_hostsim as th

    hs.LIB = lib
    hs.build = lambda force=False: lib
    log = {e: [] for e in ENTRY}
    for e in ENTRY:
        def wrap(*a, _f=getattr(hs, e), _e=e, **kw):
            r = _f(*a, **kw)
            # not OPTIMAL: the solution is not written (the callers hold theirs), so it is not compared
            kept = r[1:] if isinstance(r, tuple) and r[1] != 0 else r
            wrec = [bits(v) for v in list(a) + list(kw.values())
                    if isinstance(v, np.ndarray) and v.size == hs.WREC_SIZE and _e == "qp_cadmm_warm"]
            log[_e].append((bits(kept), bits(hs.last_diag()), bits(hs.last_work()), hs.last_stiff(), wrec))
            return r
        setattr(hs, e, wrap)
    for t in TESTS:
        fn = getattr(th, t)
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        cases = [(v,) if not isinstance(v, (tuple, list)) else tuple(v) for m in marks for v in m.args[1]] or [()]
        for c in cases:
            try:
                fn(*c)
            except AssertionError as ex:  # the comparison is of the solves, whatever the test makes of them
                print(f"  ({t}{c}: assertion {ex})")
            except AttributeError as ex:  # a build from before an entry point existed: its entry stays empty
                print(f"  ({t}{c}: {ex})")
            except pytest.skip.Exception:
                pass
    with open(out, "wb") as f:
        pickle.dump(log, f)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--record":
        record(os.path.abspath(sys.argv[2]), sys.argv[3])
        sys.exit(0)
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    logs = []
    for k, lib in enumerate(sys.argv[1:]):
        out = f"/tmp/same_hostsim_{os.getpid()}_{k}.pkl"
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--record", lib, out], cwd=ROOT)
        with open(out, "rb") as f:
            logs.append(pickle.load(f))
        os.remove(out)
    bad = 0
    for e in ENTRY:
        a, b = logs[0][e], logs[1][e]
        diff = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
        bad += diff
        print(f"{'equal' if not diff else 'DIFFERENT':>9}  {e}: {len(a)} / {len(b)} solves, {diff} differ")
    print(f"{sum(len(v) for v in logs[0].values())} solves, {bad} not equal")
    sys.exit(1 if bad else 0)
