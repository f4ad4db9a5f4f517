"""The IPM's batched LDS reads (dat_ipm.hpp "How the IPM reads LDS": records read once per phase, row loops one
slot ahead) in every instantiation the launchers can select.

k_cadmm compiles one IPM loop per (env class, row mode) pair; which pair a scenario runs follows from its env
class and from the launch geometry: G scenario slots per wavefront (dat_cadmm_slots) and the row-state placement
of the class at that G (dat_cadmm_row_mode: 0 registers, 1 LDS rows, 2 LDS rows + aux slots).  The pairs, computed
on the host from the library's own rule (test_reachable_pairs asserts this table):

    n = 3    G <= 12: (0, 2) (1, 2) (2, 2) (3, 0)      G >= 13: (0, 2) (1, 2) (2, 1) (3, 0)
    n = 6    every G: (0, 2) (1, 2) (2, 2) (3, 0)
    n = 16   every G: (0, 2) (1, 2) (2, 2) (3, 0)

so four cases reach them all: n = 3 at G = 1 and at G = 21, n = 6 at G = 10, n = 16 at G = 4 (G = 64 // n with
four resident workgroups, G = 1 with the default grid).  Each case is one forest control step of 128 scenarios
from scenarios.forest_path_states; the last 8 fly towards an arc of extra trees, which fills the 10 env row slots
of some agent (env class 3), and every env class must have run.  Checks:

  * outputs bitwise equal on 1 and on 4 sub-batches: the scenarios then sit in other slots and lanes, and a read
    from a wrong lane's column or a stale record depends on the lane position;
  * a sample against the oracle at test_gpu_c4.py's bounds: ADMM counts exact, f_des within 1e-5 relative.

One DD step (n = 3) and one centralized step (n = 4: W = 4 lane groups) against the oracle at test_gpu_parity.py's
bounds: both kernels run the same ipm_attempt.  The tail kernel (one scenario per wavefront, the other lanes idle
or clones, so its LDS columns differ from the batch kernel's): at n = 6 the two stall scenarios of
tests/golden/ref_c4_hard.npz through their first stalled steps (step 1 is handed to the tail at pass 16, step 2 is
routed to it before its first pass) at test_gpu_c4_hard.py's bound; the golden file holds n = 6 only, so the
n = 3 routed case is test_gpu_tail_team_sizes.py's (forced 21-pass steps, step 2 routed) against its oracle."""

import functools

import numpy as np
import pytest

from oracle import controllers as oc
from oracle import scenarios as osc
from tests._golden import load
from tests.test_gpu_c4 import _ambiguous, _oforest, _ostate, _rel
from tests.test_gpu_tail_team_sizes import MAX_ITER, _engine, _inputs, _oracle, _with_arc

pytestmark = pytest.mark.gpu

REL = 1e-5
B = 128
NARC = 8
# (n, resident workgroups (0: default), expected G of the one-sub-batch run, oracle sample size)
CASES = [(3, 0, 1, 5), (3, 4, 21, 5), (6, 4, 10, 4), (16, 4, 4, 3)]
PAIRS = {(3, 1): [(0, 2), (1, 2), (2, 2), (3, 0)], (3, 21): [(0, 2), (1, 2), (2, 1), (3, 0)],
         (6, 10): [(0, 2), (1, 2), (2, 2), (3, 0)], (16, 4): [(0, 2), (1, 2), (2, 2), (3, 0)]}


def _pairs(n, G):
    from distributed_aerial_transportation_amd import _lib

    return [(c, _lib.lib().dat_cadmm_row_mode(n, G, c)) for c in range(4)]


def test_reachable_pairs():
    """the docstring's table, from the library's rule: over every G the pairs of n = 3 are those of G = 1 and
    G = 21, and n = 6 / n = 16 have one set"""
    for n in (3, 6, 16):
        seen = {tuple(_pairs(n, G)) for G in range(1, 64 // n + 1)}
        want = {tuple(v) for (m, _), v in PAIRS.items() if m == n}
        assert seen == want, (n, seen)
    for (n, G), v in PAIRS.items():
        assert _pairs(n, G) == v


@functools.lru_cache(maxsize=None)
def _case_inputs(n):
    from distributed_aerial_transportation_amd import Forest, scenarios

    forests = [Forest.seeded(s) for s in range(4)]
    sf = (np.arange(B) % 4).astype(np.int32)
    x0 = scenarios.forest_path_states(n, B, np.random.default_rng(100 + n), forests, sf)
    for b in range(B - NARC, B):
        forests.append(_with_arc(forests[sf[b]], x0[b], n))
        sf[b] = len(forests) - 1
    return forests, sf, x0


def _step(n, blocks, nsub):
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    forests, sf, x0 = _case_inputs(n)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.set_forests(forests, sf)
        if blocks:
            eng.set_persistent_blocks(blocks)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.set_sub_batches(nsub)
        G = eng.cadmm_slots(B // nsub)
        r = eng.control(None, None)
        cls = [eng.class_work(k)["qp_solves"] for k in range(4)]
        w = eng.work()
    finally:
        eng.close()
    return r, G, cls, w


@functools.lru_cache(maxsize=None)
def _oracle_step(n, b):
    forests, sf, x0 = _case_inputs(n)
    of_ = _oforest(forests[sf[b]])
    ctl = oc.CADMM(osc.params(n), osc.col_radius(n), of_)
    s = _ostate(x0[b], n)
    acc, _, _ = oc.desired_acceleration_forest(s, of_)
    return ctl.control(s, acc)


@pytest.mark.parametrize("n,blocks,G,nsample", CASES)
def test_gpu_cadmm_pairs_groupings_and_oracle(n, blocks, G, nsample):
    r1, G1, cls, w = _step(n, blocks, 1)
    r4, G4, cls4, _ = _step(n, blocks, 4)
    print(f"n = {n}: G {G1} (4 sub-batches: {G4}), pairs {_pairs(n, G1)}, agent QPs per env class {cls}")
    assert G1 == G and _pairs(n, G1) == PAIRS[(n, G)]
    assert all(c > 0 for c in cls), cls  # every (class, row mode) pair of the case ran
    assert np.all(np.isfinite(r1.f_des))
    for a in ("f_des", "iters", "qp_status", "collision", "min_env_dist"):
        assert np.array_equal(getattr(r1, a), getattr(r4, a)), a
    assert w["inband_beyond_clarabel_tol"] == 0
    # the scenarios nearest to a tree, one behind the arc, and another
    order = [b for b in np.argsort(r1.min_env_dist) if b < B - NARC]
    sample = order[: nsample - 2] + [B - 1, order[len(order) // 2]]
    checked = 0
    for b in sample:
        f, st = _oracle_step(n, int(b))
        rel = _rel(r1.f_des[b], f)
        print(f"  scenario {b}: ADMM passes {r1.iters[b]} / {st.iter}, f_des rel {rel:.1e}")
        if _ambiguous(st.err_seq, st.iter):
            continue
        assert r1.iters[b] == st.iter, (b, r1.iters[b], st.iter)
        assert rel < REL, (b, rel)
        checked += 1
    assert checked >= len(sample) - 1


def test_gpu_dd_step_n3_matches_oracle():
    from distributed_aerial_transportation_amd import BatchedController, scenarios
    from tests.test_gpu_parity import _ambiguous as amb

    n, nb = 3, 6
    rng = np.random.default_rng(13)
    states = scenarios.perturbed_states(n, nb, rng)
    acc = rng.uniform(-3, 3, (nb, 6))
    eng = BatchedController("dd", n, nb, scenarios.params_block(n))
    try:
        r = eng.control(states, acc)
        assert eng.work()["inband_beyond_clarabel_tol"] == 0
    finally:
        eng.close()
    skipped = 0
    for b in range(nb):
        f, st = oc.DD(osc.params(n), osc.col_radius(n)).control(_ostate(states[b], n), (acc[b, :3], acc[b, 3:]))
        if amb(st.err_seq):
            skipped += 1
            continue
        assert r.iters[b] == st.iter, (b, r.iters[b], st.iter)
        assert _rel(r.f_des[b], f) < REL, (b, _rel(r.f_des[b], f))
        assert np.all(r.qp_status[b] == 0)
    assert skipped <= 1


def test_gpu_centralized_step_n4_matches_oracle():
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    n, nb = 4, 5
    rng = np.random.default_rng(44)
    states = scenarios.perturbed_states(n, nb, rng)
    acc = rng.uniform(-3, 3, (nb, 6))
    eng = BatchedController("centralized", n, nb, scenarios.params_block(n))
    try:
        r = eng.control(states, acc)
        assert eng.work()["inband_beyond_clarabel_tol"] == 0
    finally:
        eng.close()
    for b in range(nb):
        f, _ = oc.Centralized(osc.params(n), osc.col_radius(n)).control(_ostate(states[b], n), (acc[b, :3], acc[b, 3:]))
        assert _rel(r.f_des[b], f) < REL, (b, _rel(r.f_des[b], f))
        assert np.all(r.qp_status[b] == 0)


def test_gpu_tail_n6_first_stalled_steps():
    """ref_c4_hard.npz, steps 0-2: step 1 (the first 101-pass stall) enters the tail at pass 16, step 2 is routed"""
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios

    d = load("ref_c4_hard.npz")
    n, J = 6, d["x0"].shape[0]
    eng = BatchedController("cadmm", n, J, scenarios.params_block(n))
    try:
        eng.set_forests([Forest.seeded(int(s)) for s in d["forest_seed"]], np.arange(J, dtype=np.int32))
        eng.set_state(d["x0"], np.zeros(J, dtype=np.int32))
        for k in range(3):
            r = eng.control(None, None)
            np.testing.assert_array_equal(r.iters, d["iters"][:, k].astype(int), err_msg=f"step {k}")
            for j in range(J):
                ref = d["f_des"][j, k]
                scale = max(1.0, np.max(np.abs(ref)))
                rel = np.max(np.abs(r.f_des[j] - ref)) / scale
                sens = np.max(np.abs(d["f_des_1e10"][j, k] - ref)) / scale
                sens8 = np.max(np.abs(d["f_des_1e8"][j, k] - ref)) / scale
                print(f"stretch {j} step {k}: f_des rel {rel:.1e} (sensitivity {sens:.1e}, {sens8:.1e})")
                assert rel < max(1e-5, 5.0 * sens, sens8), (j, k, rel, sens, sens8)
            eng.rollout(10)
        w = eng.work()
    finally:
        eng.close()
    assert w["tail_passes"] > 0 and w["tail_routed"] == J
    assert w["inband_beyond_clarabel_tol"] == 0


def test_gpu_tail_n3_routed_step():
    n = 3
    forests, x0 = _inputs(n)
    ref = _oracle(n)
    eng = _engine(n, forests, x0)
    try:
        eng.set_force_err_tolerance(0.0, True)
        eng.set_max_iter(MAX_ITER)
        r1 = eng.control(None, None)
        eng.rollout(10)
        r2 = eng.control(None, None)
        w = eng.work()
    finally:
        eng.close()
    assert w["tail_routed"] == len(x0)
    for b in range(len(x0)):
        f1, _, _, f2, _, _ = ref[b]
        print(f"n = 3 scenario {b}: f_des rel {_rel(r1.f_des[b], f1):.1e} {_rel(r2.f_des[b], f2):.1e}")
        assert _rel(r1.f_des[b], f1) < REL and _rel(r2.f_des[b], f2) < REL
    np.testing.assert_array_equal(r2.iters, MAX_ITER + 1)
    assert np.all(r2.qp_status == 0)
