"""Point-mass rigid-link system on the GPU (k_pmrl_forward, k_pmrl_rollout) against the reference's own
PMRLDynamics (ref_pmrl.npz, written by tests/golden/make_pmrl.py): the four (n, B) cases with per-scenario
parameters, the bitwise invariances of the lane mapping and of the launch schedule, the PMRLDynamics drop-in over
the reference's own recipe, and the error paths.  Bounds: those of test_pmrl_host.py (tests/_pmrl.py)."""

import numpy as np
import pytest

from tests import _pmrl as F

pytestmark = pytest.mark.gpu


def _engine(c, scenarios=None):
    """a handle over the case's scenarios (all, or the listed ones) at their start states"""
    from distributed_aerial_transportation_amd.control import BatchedController

    idx = np.arange(c.B) if scenarios is None else np.asarray(scenarios)
    eng = BatchedController("centralized", c.n, len(idx), c.prm[idx], per_scenario_params=True, dt=c.dt)
    eng.set_state(c.x0[idx], c.c0[idx])
    return eng


@pytest.mark.parametrize("n", [n for n, _ in F.CASES])
def test_forward_matches_reference(n):
    """pmrl_forward at the start and, after 40 steps, at the state the reference reached: T and the accelerations
    within 1e-11 of max(1, |.|); the call leaves the state bits alone."""
    c = F.case(n)
    eng = _engine(c)
    for j in range(len(c.acc_at)):
        if c.acc_at[j] != 0:
            ref, rc = c.ref_block(c.keep.index(c.acc_at[j]))
            eng.set_state(ref, rc)
        before = eng.get_state()
        (ddq, dvl, dwl), T = eng.pmrl_forward(c.acc_force(j))
        after = eng.get_state()
        assert np.array_equal(before[0].view(np.uint64), after[0].view(np.uint64))
        assert np.array_equal(before[1], after[1])
        for b in range(c.B):
            F.check_acc("gpu", ((ddq[b], dvl[b], dwl[b]), T[b]), c, j, b)
    eng.close()


def _run(c, eng, launches):
    """the case's 45 steps in `launches` launches (1, nf or steps); the states at the kept steps a launch ends on"""
    hold = c.steps // c.nf
    got = {}
    if launches == 1:
        eng.pmrl_rollout(c.steps, c.f)
    elif launches == c.nf:
        for k in range(c.nf):
            eng.pmrl_rollout(hold, c.f[k])
            if (k + 1) * hold in c.keep:
                got[(k + 1) * hold] = eng.get_state()
    else:
        assert launches == c.steps
        for k in range(c.steps):
            eng.pmrl_rollout(1, c.f[k // hold])
            if k + 1 in c.keep:
                got[k + 1] = eng.get_state()
    got[c.steps] = eng.get_state()
    return got


@pytest.mark.parametrize("n", [n for n, _ in F.CASES])
def test_rollout_matches_reference_and_schedules_agree(n):
    """45 steps under the 9-set schedule.  One launch: the final states within 1e-10 of the reference's, the
    counters equal.  Nine launches of 5 steps and 45 launches of one step: the same bits as the one launch, and
    every stored state (steps 1, 20, 21, 40, 45) within 1e-10 with its counters equal."""
    c = F.case(n)
    eng = _engine(c)
    one = _run(c, eng, 1)[c.steps]
    ref, rc = c.ref_block(c.keep.index(c.steps))
    e = float(np.max(np.abs(one[0] - ref)))
    print(f"n = {n}: one launch, max state diff {e:.2e}")
    assert e <= F.TOL_STATE, (n, e)
    assert np.array_equal(one[1], rc)
    for launches in (c.nf, c.steps):
        eng.set_state(c.x0, c.c0)
        got = _run(c, eng, launches)
        assert np.array_equal(got[c.steps][0].view(np.uint64), one[0].view(np.uint64)), launches
        assert np.array_equal(got[c.steps][1], one[1]), launches
        if launches == c.steps:
            assert sorted(got) == sorted(c.keep)
        for k, (x, cnt) in got.items():
            ref, rc = c.ref_block(c.keep.index(k))
            e = float(np.max(np.abs(x - ref)))
            assert e <= F.TOL_STATE, (n, launches, k, e)
            assert np.array_equal(cnt, rc), (n, launches, k)
    eng.close()


@pytest.mark.parametrize("n", [3, 6])
def test_scenario_alone_gives_the_batch_bits(n):
    """Scenario b run alone in a B = 1 handle (lane group 0 of block 0) gives the bits it gives inside the batch,
    whatever its lane group and block there: the states after the 45 steps, and T and the accelerations."""
    c = F.case(n)
    eng = _engine(c)
    acc_b, T_b = eng.pmrl_forward(c.f[0])
    eng.pmrl_rollout(c.steps, c.f)
    xb, cb = eng.get_state()
    eng.close()
    for b in range(c.B):
        one = _engine(c, [b])
        acc_1, T_1 = one.pmrl_forward(c.f[0][b:b + 1])
        for u, v in zip(acc_1 + (T_1,), tuple(a[b:b + 1] for a in acc_b) + (T_b[b:b + 1],)):
            assert np.array_equal(np.ascontiguousarray(u).view(np.uint64), np.ascontiguousarray(v).view(np.uint64)), b
        one.pmrl_rollout(c.steps, c.f[:, b:b + 1])
        x1, c1 = one.get_state()
        one.close()
        assert np.array_equal(x1[0].view(np.uint64), xb[b].view(np.uint64)), (n, b)
        assert c1[0] == cb[b]


def test_dropin_reference_recipe():
    """PMRLDynamics over the reference's own n = 3 recipe (test/system/test_pmrldynamics.py:9-49): 400 steps, one
    integrate(f) per step, the states every 100 steps within 1e-10."""
    from distributed_aerial_transportation_amd import PMRLDynamics, pmrl

    p, s0, dt, f, every, kept = F.recipe()
    dyn = PMRLDynamics(p, s0, dt)
    for k in range(f.shape[0]):
        if k == 0:
            acc, T = dyn.forward_dynamics(f[k])
            assert PMRLDynamics.inverse_dynamics_error(dyn.state, p, f[k], T, acc) <= 1e-12
        dyn.integrate(f[k])
        if (k + 1) % every == 0:
            e = float(np.max(np.abs(pmrl.pack_pmrl_state(dyn.state) - pmrl.pack_pmrl_state(kept[(k + 1) // every - 1]))))
            print(f"step {k + 1}: state diff {e:.2e}")
            assert e <= F.TOL_STATE, (k + 1, e)
    assert dyn.state.counter == f.shape[0] % 20


def test_error_paths():
    """steps % nf != 0 and parameters not set: an error code, a dat_last_error text, and nothing launched (the
    states keep their bits)."""
    from distributed_aerial_transportation_amd import _lib as L
    from distributed_aerial_transportation_amd import layout

    c = F.case(3)
    eng = _engine(c)
    before = eng.get_state()
    f = L.f64(c.f.transpose(0, 1, 3, 2).reshape(c.nf, c.B, 9))
    lib = L.lib()
    assert lib.dat_pmrl_rollout(eng._h, 10, L.ptr(f), c.nf) < 0
    msg = lib.dat_last_error().decode()
    assert "dat_pmrl_rollout" in msg and "multiple of nf" in msg, msg
    assert lib.dat_pmrl_rollout(eng._h, 9, L.ptr(f), 0) < 0
    assert "nf must be" in lib.dat_last_error().decode()
    with pytest.raises(L.DatError, match="multiple of nf"):
        eng.pmrl_rollout(10, c.f)
    after = eng.get_state()
    assert np.array_equal(before[0].view(np.uint64), after[0].view(np.uint64)) and np.array_equal(before[1], after[1])
    eng.close()

    # a handle whose parameters were never set
    cfg = L.Config()
    lib.dat_default_config(cfg)
    cfg.mode, cfg.n, cfg.batch, cfg.dt = L.MODE_CENTRALIZED, 3, c.B, c.dt
    h = L.H()
    assert lib.dat_create(cfg, h) == 0, lib.dat_last_error()
    try:
        x0 = L.f64(c.x0)
        assert lib.dat_set_state(h, L.ptr(x0), L.ptr(c.c0, L.I)) == 0
        assert lib.dat_pmrl_rollout(h, c.steps, L.ptr(f), c.nf) < 0
        msg = lib.dat_last_error().decode()
        assert "dat_pmrl_rollout" in msg and "params not set" in msg, msg
        out = [np.zeros(c.B * 9), np.zeros(c.B * 3), np.zeros(c.B * 3), np.zeros(c.B * 3)]
        assert lib.dat_pmrl_forward(h, L.ptr(f), *(L.ptr(o) for o in out)) < 0
        msg = lib.dat_last_error().decode()
        assert "dat_pmrl_forward" in msg and "params not set" in msg, msg
        assert not any(np.any(o) for o in out)
        x = np.empty((c.B, layout.state_size(3)))
        cnt = np.empty(c.B, dtype=np.int32)
        assert lib.dat_get_state(h, L.ptr(x), L.ptr(cnt, L.I)) == 0
        assert np.array_equal(x.view(np.uint64), x0.view(np.uint64)) and np.array_equal(cnt, c.c0)
    finally:
        lib.dat_destroy(h)
