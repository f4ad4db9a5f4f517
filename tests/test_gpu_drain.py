"""GPU: the persistent queue drains must not change any scenario's arithmetic, and the handle keeps no
hidden history across a warm-start reset.

Reference semantics: a scenario's C-ADMM / DD control step (control/rqp_cadmm.py:631-675,
control/rqp_dd.py:695-752) depends only on its own state, inputs and warm state (f, f_mean, lambda /
lambda_F, lambda_M), never on the other scenarios of the batch.  On the device, k_bucket sorts the
scenarios into queues with LDS atomics (the order within a sort key varies from run to run) and the
persistent k_cadmm / k_dd workgroups refill their scenario slots as scenarios stop, so which
scenarios share a wavefront changes with the grid size and from run to run.  These tests compare
different groupings bitwise, including the n = 16 LDS carve (config C5: 4 scenario slots of 16
lanes per wavefront) with slot refill, and require that no agent QP is accepted through the IPM's
in-band best-iterate exit with an iterate outside Clarabel's own 1e-8 tolerance (dat_get_inband_exits;
DESIGN.md section 2).
"""

import numpy as np
import pytest

from oracle import controllers as oc
from oracle import model as om
from oracle import scenarios as osc

pytestmark = pytest.mark.gpu

REL = 1e-5


def _ostate(x, n):
    from distributed_aerial_transportation_amd.system import RQPState

    s = RQPState.unpack(x, n)
    return om.State(s.R, s.w, s.xl, s.vl, s.Rl, s.wl, project=False)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _ambiguous(seq, tol=1e-2):
    return any(abs(e - tol) < 1e-7 * tol for e in seq)


def test_gpu_cadmm_n16_persistent_drain():
    """Config C5 geometry (n = 16, G = 4 slots per wavefront): B = 12 scenarios on ONE resident
    workgroup (every slot refilled twice per ADMM step) over two warm steps must equal the uncapped
    grid bitwise; every agent QP OPTIMAL (no in-band exit beyond Clarabel's tolerance); a sample matches the oracle (ADMM
    iteration counts exact, f_des within 1e-5)."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    n, B = 16, 12
    rng = np.random.default_rng(1616)
    states = scenarios.perturbed_states(n, B, rng)
    a1 = rng.uniform(-0.5, 0.5, (B, 6)) * 6.0
    a2 = rng.uniform(-0.5, 0.5, (B, 6)) * 6.0
    runs = []
    for blocks in (1, 0):
        eng = BatchedController("cadmm", n, B, scenarios.params_block(n), record_err=True)
        eng.set_persistent_blocks(blocks)
        runs.append((eng.control(states, a1), eng.control(states, a2)))
        assert eng.work()["inband_beyond_clarabel_tol"] == 0
        if blocks == 1:
            # one workgroup of 4 slots ran all 12 scenarios: slots were refilled
            assert eng.work()["qp_solves"] >= 2 * B * n
    for r_cap, r_full in zip(*runs):
        np.testing.assert_array_equal(r_cap.f_des, r_full.f_des)
        np.testing.assert_array_equal(r_cap.iters, r_full.iters)
        np.testing.assert_array_equal(r_cap.err_seq, r_full.err_seq)
        assert np.all(r_cap.qp_status == 0)
    r1, r2 = runs[0]
    checked = 0
    for b in (0, 5, 11):
        ctl = oc.CADMM(osc.params(n), osc.col_radius(n))
        s = _ostate(states[b], n)
        f1, st1 = ctl.control(s, (a1[b, :3], a1[b, 3:]))
        f2, st2 = ctl.control(s, (a2[b, :3], a2[b, 3:]))
        if _ambiguous(st1.err_seq) or _ambiguous(st2.err_seq):
            continue
        assert r1.iters[b] == st1.iter and r2.iters[b] == st2.iter, (b, r1.iters[b], st1.iter, r2.iters[b], st2.iter)
        assert _rel(r1.f_des[b], f1) < REL and _rel(r2.f_des[b], f2) < REL, (b, _rel(r1.f_des[b], f1))
        checked += 1
    assert checked >= 2


def _c4_engine(blocks, B=120, n=6):
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios
    from tests.test_gpu_c4 import near_tree_states

    forests = [Forest.seeded(s) for s in range(4)]
    sf = np.arange(B) % 4
    x0 = near_tree_states(n, forests, sf, np.random.default_rng(2024))
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n), record_err=True)
    eng.set_forests(forests, sf)
    eng.set_persistent_blocks(blocks)
    eng.set_state(x0, np.zeros(B, dtype=np.int32))
    return eng


def _c4_two_steps(eng):
    r1 = eng.control(None, None)
    eng.rollout(10)
    r2 = eng.control(None, None)
    return r1, r2


def test_gpu_cadmm_groupings_bitwise():
    """The C4 production path (k_env_class -> k_bucket -> k_cadmm, n = 6 in seeded forests, binding env
    rows) on a grid capped at 2 workgroups, on the full grid, and again on the full grid (k_bucket's
    atomic scatter regroups the scenarios from run to run): f_des, ADMM iteration counts and residual
    sequences bitwise equal over two warm steps, and no in-band exit beyond Clarabel's tolerance."""
    res = []
    for blocks in (2, 0, 0):
        eng = _c4_engine(blocks)
        res.append(_c4_two_steps(eng))
        assert eng.work()["inband_beyond_clarabel_tol"] == 0
    for other in res[1:]:
        for ra, rb in zip(res[0], other):
            np.testing.assert_array_equal(ra.f_des, rb.f_des)
            np.testing.assert_array_equal(ra.iters, rb.iters)
            np.testing.assert_array_equal(ra.err_seq, rb.err_seq)
            np.testing.assert_array_equal(ra.qp_status, rb.qp_status)


@pytest.mark.parametrize("mode", ["cadmm", "dd"])
def test_gpu_reset_warm_start_matches_fresh_handle(mode):
    """dat_reset_warm_start restores the constructor's state completely (control/rqp_cadmm.py:577-580,
    control/rqp_dd.py:628-632): a handle that ran two steps and was reset gives bitwise the step of a
    freshly created handle -- including the previous-step iteration counts that select the IPM start
    and the drain order, which the reference does not have."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    n, B = 6, 40
    rng = np.random.default_rng(99)
    x = scenarios.perturbed_states(n, B, rng)
    accs = [rng.uniform(-0.5, 0.5, (B, 6)) * 8.0 for _ in range(3)]
    used = BatchedController(mode, n, B, scenarios.params_block(n), record_err=True)
    used.control(x, accs[0])
    used.control(x, accs[1])
    used.reset_warm_start()
    fresh = BatchedController(mode, n, B, scenarios.params_block(n), record_err=True)
    ra, rb = used.control(x, accs[2]), fresh.control(x, accs[2])
    np.testing.assert_array_equal(ra.f_des, rb.f_des)
    np.testing.assert_array_equal(ra.iters, rb.iters)
    np.testing.assert_array_equal(ra.err_seq, rb.err_seq)
    # and the next step, whose IPM start depends on this step's iteration counts
    ra, rb = used.control(x, accs[0]), fresh.control(x, accs[0])
    np.testing.assert_array_equal(ra.f_des, rb.f_des)
    np.testing.assert_array_equal(ra.iters, rb.iters)


@pytest.mark.parametrize("mode,n,B,blocks", [("cadmm", 3, 40, 1), ("cadmm", 16, 9, 0), ("dd", 6, 30, 1), ("dd", 3, 25, 0)])
def test_gpu_fused_steps_equal_separate_steps(mode, n, B, blocks):
    """dat_control_steps: K control steps fused into one persistent drain (a slot's scenario moves on to
    its next step at once) must give every scenario exactly the arithmetic of K separate
    dat_control_step calls -- warm state carried, rho and the iteration count restarting per step
    (control/rqp_cadmm.py:631-675, control/rqp_dd.py:695-752): bitwise equal f_des, iteration counts,
    statuses and warm state, on a capped grid (slots refilled across steps) and on the full grid."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    K = 4
    rng = np.random.default_rng(500 + n)
    states = scenarios.perturbed_states(n, B, rng)
    accs = rng.uniform(-0.5, 0.5, (K, B, 6)) * 8.0
    # (the same grid cap on both sides: a C-ADMM wavefront's slot count G follows the grid, and G selects
    # where the class's IPM state lives -- registers or LDS -- i.e. another compiled instantiation)
    sep = BatchedController(mode, n, B, scenarios.params_block(n))
    sep.set_persistent_blocks(blocks)
    sep.set_state(states)
    seps = [sep.control(None, accs[k]) for k in range(K)]
    # the separate path against itself on another handle: run-to-run determinism
    sep2 = BatchedController(mode, n, B, scenarios.params_block(n))
    sep2.set_persistent_blocks(blocks)
    sep2.set_state(states)
    for k in range(K):
        r2 = sep2.control(None, accs[k])
        assert np.array_equal(r2.f_des, seps[k].f_des) and np.array_equal(r2.iters, seps[k].iters), ("separate", k)
    for k in range(1, K + 1):
        fus = BatchedController(mode, n, B, scenarios.params_block(n))
        fus.set_persistent_blocks(blocks)
        fus.set_state(states)
        r_fus = fus.control_steps(accs[:k])
        r_sep = seps[k - 1]
        bad = [b for b in range(B) if not np.array_equal(r_fus.f_des[b], r_sep.f_des[b])]
        diff = max([float(np.max(np.abs(r_fus.f_des[b] - r_sep.f_des[b]))) for b in bad] or [0.0])
        assert not bad and np.array_equal(r_fus.iters, r_sep.iters), (
            f"after {k} fused steps: scenarios {bad[:8]} differ (max {diff:.3e}); iters fused "
            f"{r_fus.iters[bad[:8]].tolist()} separate {r_sep.iters[bad[:8]].tolist()}")
        assert np.array_equal(r_fus.qp_status, r_sep.qp_status)
        fus.close()
    assert sep.work()["hl_steps"] == K


@pytest.mark.parametrize("subs", [2, 3, 4])
def test_gpu_closed_loop_sub_batches_bitwise(subs):
    """dat_set_sub_batches: the C4 closed loop (desired acceleration, env classes, class sort, C-ADMM drain,
    rollout) on 2 or 3 sub-batches, each on its own stream with no synchronisation between them, must
    leave every scenario in exactly the state of the single-stream loop after 3 HL steps (a scenario's
    arithmetic does not depend on its grouping), with the same work counters -- and with the same checkpoint of
    all scenarios, byte for byte: f_des, f, f_mean, lambda_f, iters, ipmx and the counter, every warm array a
    sub-batch's kernels reach through an offset view of the handle's."""
    n, B, K = 6, 131, 3
    one, many = (_sub_batch_run(n, B, K, sb) for sb in (1, subs))
    _assert_same_run(one, many)


def _sub_batch_run(n, B, K, subs, per_scenario_params=False):
    """K closed-loop HL steps of B near-tree scenarios in four forests on `subs` sub-batches: the final state, the
    checkpoint blob of all scenarios and the work counters."""
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios
    from tests.test_gpu_c4 import near_tree_states

    forests = [Forest.seeded(s) for s in range(4)]
    sf = np.arange(B) % 4
    x0 = near_tree_states(n, forests, sf, np.random.default_rng(77))
    params = scenarios.params_block(n)
    if per_scenario_params:
        params = np.tile(params, (B, 1))
    eng = BatchedController("cadmm", n, B, params, per_scenario_params=per_scenario_params)
    eng.set_forests(forests, sf)
    eng.set_state(x0, np.zeros(B, dtype=np.int32))
    eng.set_sub_batches(subs)
    eng.closed_loop(K)
    st, _ = eng.get_state()
    out = st, eng.checkpoint().tobytes(), eng.work()
    eng.close()
    return out


def _assert_same_run(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1] == b[1], "checkpoint blobs differ"
    for key in ("qp_solves", "ipm_iters", "ipm_row_iters", "hl_steps"):
        assert a[2][key] == b[2][key], key


def test_gpu_sub_batch_views_smallest_uneven_ranges():
    """The smallest shape at which a sub-batch's view of the handle's arrays can go wrong: n = 3, B = 7 on four
    sub-batches, whose ranges hold 1, 2, 2 and 2 scenarios (uneven, one of a single scenario), with per-scenario
    parameters (their view is offset by the parameter block, the others by the arrays' own extents) and a forest,
    over 2 HL steps.  Against one sub-batch: the state, the whole checkpoint blob and the work counters equal."""
    n, B, K = 3, 7, 2
    one, four = (_sub_batch_run(n, B, K, sb, per_scenario_params=True) for sb in (1, 4))
    _assert_same_run(one, four)
