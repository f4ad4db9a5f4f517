"""Forest C-ADMM and the tail kernel (k_cadmm_tail) at the team sizes the forest tests leave out: n = 3, 4, 8, 11, 16
(test_gpu_c4*.py run n = 6).  What depends on n on this path: the tail's clone count (8 clones up to n = 8, 5 at
n = 11, 4 at n = 16), its LDS carve (n scratch records behind the class area, beyond 64 KB for the larger teams),
k_env_class splitting a scenario's tree window over n lanes, G = 64 // n slots with 64 - G n idle lanes, the
per-class carve of k_cadmm, and the class-3 path (13 row slots, in registers in k_cadmm, in LDS in the tail).

The reference's convergence recipe makes the tail deterministic and cheap: set_force_err_tolerance(0, True) and
set_max_iter(20), so every step runs exactly 21 ADMM passes.  In step 1 k_cadmm hands every scenario to the tail at
pass 16 (TAIL_PASS), whose warm start and stall exit run from pass 17; step 2 is routed to the tail before its first
pass (the previous step's 21 passes exceed TAIL_PREV).  Half the scenarios fly in a seeded forest as it is (at most
5 env rows per agent QP), the other half in a copy with an arc of extra trees ahead of the payload, which fills the
10 env row slots of several agents (env class 3).  Checked against the oracle's C-ADMM with the same settings
(oracle.controllers.CADMM), every agent QP of which is OPTIMAL on these inputs (asserted).

The start states were chosen on the oracle alone (SEED: per scenario the first seed of 100 n + 10 b + 0..9 that
qualifies): every agent QP of both steps OPTIMAL; 10 env rows on some agent behind the arc and at most 5 in the
plain forest; and the oracle reproducible well inside the 1e-9 bound on the states after the rollout -- its own runs
at QP tolerances 1e-11 and 1e-10 end within 3e-10 of each other there.  Twenty-one forced passes stop the ADMM
loop short of consensus, where f_des follows the agent QPs' last digits: of the first seeds drawn, 6 of 17
scenarios moved by 1e-9 to 3e-8 between the oracle's two tolerances (bodies inside or grazing a tree), more than
the bound asks of the GPU.  The chosen scenarios still include bodies inside a tree (collision flag set) at n = 3
and n = 16.

Last, the tail kernels' dynamic-LDS limit with handles of two team sizes alive in one process: it belongs to the
kernel, not to the handle, and a smaller team's handle created later must not lower it under a larger team's."""

import functools

import numpy as np
import pytest

from oracle import controllers as oc
from oracle import model as om
from oracle import scenarios as osc
from oracle.ipm import OPTIMAL
from tests._golden import load
from tests.test_gpu_c4 import _oforest, _ostate, _rel, _xflat, near_tree_states

pytestmark = pytest.mark.gpu

REL = 1e-5
MAX_ITER = 20
NS = (3, 4, 8, 11, 16)
BATCH = {3: 4, 4: 4, 8: 4, 11: 3, 16: 2}
# start-state seed of every scenario, chosen on the oracle alone (see the module docstring)
SEED = {3: (300, 310, 320, 330), 4: (400, 410, 422, 430), 8: (800, 810, 821, 830), 11: (1101, 1110, 1120),
        16: (1602, 1611)}
ARC_TREES, ARC_DIST, ARC_HALF_ANGLE = 12, 3.0, 1.2


def _with_arc(forest, x, n):
    """a copy of the forest with ARC_TREES extra trees on an arc ARC_DIST ahead of the payload of state x, within
    +-ARC_HALF_ANGLE of its heading"""
    import copy

    from distributed_aerial_transportation_amd import env_forest

    F = copy.copy(forest)
    xy, v = x[12 * n:12 * n + 2], x[12 * n + 3:12 * n + 5]
    th = np.arctan2(v[1], v[0]) + np.linspace(-ARC_HALF_ANGLE, ARC_HALF_ANGLE, ARC_TREES)
    pos = np.empty((ARC_TREES, 3))
    pos[:, 0], pos[:, 1] = xy[0] + ARC_DIST * np.cos(th), xy[1] + ARC_DIST * np.sin(th)
    pos[:, 2] = [(forest.terrain_height(q) + env_forest.BARK_HEIGHT) / 2.0 for q in pos[:, :2]]
    F.tree_pos = np.vstack([forest.tree_pos, pos])
    F.num_trees = F.tree_pos.shape[0]
    return F


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(forests, one per scenario: odd scenarios with the arc; start states)"""
    from distributed_aerial_transportation_amd import Forest

    B = BATCH[n]
    plain = [Forest.seeded(s) for s in range(B)]
    x0 = np.stack([near_tree_states(n, plain, [b], np.random.default_rng(SEED[n][b]), d_axis=(1.4, 2.0))[0]
                   for b in range(B)])
    return [_with_arc(plain[b], x0[b], n) if b % 2 else plain[b] for b in range(B)], x0


class _Probe(oc.CADMM):
    """oracle C-ADMM that keeps every agent QP's status and the largest env row count"""

    def __init__(self, *a):
        super().__init__(*a)
        self.statuses, self.max_rows = [], 0

    def solve_agent(self, i, s, acc_des, env, rho):
        out = super().solve_agent(i, s, acc_des, env, rho)
        self.statuses.append(out[1].status)
        self.max_rows = max(self.max_rows, int(np.sum(np.any(env.lhs != 0.0, axis=1))))
        return out


@functools.lru_cache(maxsize=None)
def _oracle(n):
    """per scenario: (f1, st1, state after the rollout, f2, st2, largest env row count), computed once"""
    forests, x0 = _inputs(n)
    p = osc.params(n)
    out = []
    for b in range(BATCH[n]):
        of_ = _oforest(forests[b])
        ctl = _Probe(p, osc.col_radius(n), of_)
        ctl.set_force_err_tolerance(0.0, True)
        ctl.set_max_iter(MAX_ITER)
        s = _ostate(x0[b], n)
        acc, _, _ = oc.desired_acceleration_forest(s, of_)
        f1, st1 = ctl.control(s, acc)
        for _ in range(10):
            f, M = om.low_level_control(p, s, f1)
            s.integrate(*om.forward_dynamics(p, s, f, M), 1e-3)
        x1 = _xflat(s, n)
        acc2, _, _ = oc.desired_acceleration_forest(s, of_)
        f2, st2 = ctl.control(s, acc2)
        # clean inputs: the oracle solves every agent QP of both steps
        assert all(q == OPTIMAL for q in ctl.statuses), (n, b, [q for q in ctl.statuses if q != OPTIMAL])
        assert st1.iter == MAX_ITER + 1 and st2.iter == MAX_ITER + 1
        out.append((f1, st1, x1, f2, st2, ctl.max_rows))
    # the arc fills all 10 env row slots of some agent (env class 3); the plain forest stays below
    assert all(o[5] == 10 for o in out[1::2]) and all(o[5] <= 5 for o in out[0::2]), [o[5] for o in out]
    return out


def _engine(n, forests, x0, **kw):
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    B = len(x0)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n), **kw)
    eng.set_forests(forests, np.arange(B, dtype=np.int32))
    eng.set_state(x0, np.zeros(B, dtype=np.int32))
    return eng


@pytest.mark.parametrize("n", NS)
def test_gpu_tail_team_size_matches_oracle(n):
    forests, x0 = _inputs(n)
    B = BATCH[n]
    ref = _oracle(n)
    eng = _engine(n, forests, x0, record_err=True)
    try:
        eng.set_force_err_tolerance(0.0, True)
        eng.set_max_iter(MAX_ITER)
        eng.set_persistent_blocks(1)  # B > 64 // n slots at n = 16 (and the slots refill)
        r1 = eng.control(None, None)
        w1 = eng.work()
        eng.rollout(10)
        x1, _ = eng.get_state()
        r2 = eng.control(None, None)
        w2 = eng.work()
        cls3 = eng.class_work(3)
    finally:
        eng.close()
    for r in (r1, r2):
        np.testing.assert_array_equal(r.iters, MAX_ITER + 1)
        assert np.all(r.qp_status == 0), np.argwhere(r.qp_status != 0)
    for b in range(B):
        f1, st1, xo, f2, st2, _ = ref[b]
        print(f"n = {n} scenario {b}: f_des rel {_rel(r1.f_des[b], f1):.1e} {_rel(r2.f_des[b], f2):.1e}, states "
              f"{np.max(np.abs(x1[b] - xo)):.1e}")
        assert _rel(r1.f_des[b], f1) < REL, (b, _rel(r1.f_des[b], f1))
        assert _rel(r2.f_des[b], f2) < REL, (b, _rel(r2.f_des[b], f2))
        np.testing.assert_allclose(r1.err_seq[b, :MAX_ITER], st1.err_seq, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(r2.err_seq[b, :MAX_ITER], st2.err_seq, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(x1[b], xo, atol=1e-9, rtol=0)
        for r, st in ((r1, st1), (r2, st2)):
            assert bool(r.collision[b]) == bool(st.collision)
            assert r.min_env_dist[b] == pytest.approx(st.min_env_dist, abs=1e-8)
    assert w2["inband_beyond_clarabel_tol"] == 0
    assert cls3["qp_solves"] > 0
    assert w1["tail_passes"] > 0 and w1["tail_routed"] == 0
    assert w2["tail_routed"] == B


@pytest.mark.parametrize("n", [3, 16])
def test_gpu_tail_team_size_sub_batches_bitwise(n):
    """closed_loop(2) on one and on two sub-batches from the same states ends bitwise equal (the second step is
    routed to the tail launch beside k_cadmm with one sub-batch, handed over by k_cadmm with two), as
    test_gpu_c4_stall_sub_batches_bitwise at n = 6."""
    forests, x0 = _inputs(n)
    out = []
    for nsub in (1, 2):
        eng = _engine(n, forests, x0)
        try:
            eng.set_force_err_tolerance(0.0, True)
            eng.set_max_iter(MAX_ITER)
            eng.set_sub_batches(nsub)
            eng.closed_loop(2)
            eng.synchronize()
            out.append((eng.get_state()[0], eng.work()))
        finally:
            eng.close()
    (s1, w1), (s2, w2) = out
    assert w1["tail_passes"] > 0 and w2["tail_passes"] > 0
    assert w1["tail_routed"] == BATCH[n] and w2["tail_routed"] == 0
    assert np.array_equal(s1, s2)


def _stall_engine():
    from distributed_aerial_transportation_amd import Forest

    d = load("ref_c4_hard.npz")
    J = d["x0"].shape[0]
    eng = _engine(6, [Forest.seeded(int(s)) for s in d["forest_seed"]], d["x0"])
    assert J == eng.batch
    return eng


def _stall_run(eng):
    """3 HL steps of the C4 stall stretches: steps 2 and 3 are 101-pass stalls in the tail"""
    out = []
    for _ in range(3):
        r = eng.control(None, None)
        eng.rollout(10)
        out.append((r.f_des.copy(), r.iters.copy(), eng.get_state()[0]))
    assert np.all(out[1][1] == 101) and np.all(out[2][1] == 101)
    assert eng.work()["tail_passes"] > 0
    return out


def _small_engine():
    forests, x0 = _inputs(3)
    return _engine(3, forests, x0)


def test_gpu_tail_lds_limit_with_two_handles():
    """An n = 6 handle run alone, then again with an n = 3 forest handle created after it and stepped before it
    (dat_create used to set the tail kernels' dynamic-LDS limit to the new handle's own need, below the live n = 6
    handle's): the n = 6 results are bitwise those of the solo run, and the n = 3 handle's those of its own."""
    eng = _stall_engine()
    try:
        solo6 = _stall_run(eng)
    finally:
        eng.close()
    eng = _small_engine()
    try:
        solo3 = eng.control(None, None)
    finally:
        eng.close()
    big, small = _stall_engine(), None
    try:
        small = _small_engine()
        r3 = small.control(None, None)
        both6 = _stall_run(big)
    finally:
        big.close()
        if small is not None:
            small.close()
    for (f, it, x), (f0, it0, x0) in zip(both6, solo6):
        assert np.array_equal(f, f0) and np.array_equal(it, it0) and np.array_equal(x, x0)
    assert np.array_equal(r3.f_des, solo3.f_des) and np.array_equal(r3.iters, solo3.iters)
    assert np.all(r3.qp_status == 0)
