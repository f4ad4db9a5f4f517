"""The trajectory-tracking law in the resident closed loop (dat_set_tracking, dat_set_clock, dat_set_plant): the law of
the reference's controller tests (test/control/test_rqpcontrollers.py:24-48, test/control/test_rpcentralized.py:14-38)
evaluated on the device at t = clock * dt, for both plants.

1. the rigid payload, resident (k_cent + k_rp_advance), against the reference's own 20 s recording (ref_rp.npz), with
   the bounds of test_gpu_rp_closed_loop, whose loop this is: states 1e-4, forces 1e-5 relative;
2. per-scenario records and T0: 22 scenarios (one more than floor(64 / 3)) started along that recording;
3. the quadrotor plant against the oracle's tracked loops (ref_track.npz, tests/_track.py);
4. every schedule of the closed loop against the serial one under tracking, bitwise: an advance pass of step k
   computes the inputs of step k + 1 and has to carry that step's tick;
5. the log's x_ref / v_ref under tracking, and example.simulate(law="circle") resident against step by step;
6. set_tracking(None) gives the forest loop back bitwise, and the error cases leave the handle usable.

Bounds of 3 (tests/_tolerances.py's rules): iters exact except where the oracle's own count moves between IPM
tolerances 1e-11 and 1e-10 (count_moves) or a residual sits in the stopping band (_ambiguous), at most one step in 8;
f_des within max(REL, 5 x sens_f); states within 1e-6.  The oracle's own 1e-10-vs-1e-11 state spread over these loops
(stored with the fixture, make_track.py): C-ADMM n = 3 3.0e-9, n = 6 1.7e-7, DD 1.5e-9, centralized 2.0e-9; five times
the largest is 8.5e-7, below 1e-6, so the bound stands as it is (test_track_fixture.py asserts that)."""

import functools

import numpy as np
import pytest

from tests import _track
from tests._golden import load
from tests._tolerances import REL, _ambiguous

pytestmark = pytest.mark.gpu

RP_STATE_ATOL, RP_F_REL = 1e-4, 1e-5  # test_gpu_rp_closed_loop's
STATE_ATOL = 1e-6
F_MARGIN = 5.0


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _rp_vec(s):
    return np.concatenate([s.xl, s.vl, s.Rl.reshape(-1), s.wl])


# ---- 1, 2: the rigid payload ---------------------------------------------------------------------------------------
def test_rp_resident_loop_matches_the_reference_recording():
    from distributed_aerial_transportation_amd import rigid_payload as rp

    d = load("ref_rp.npz")
    p, _, s0 = rp.rp_setup(3)
    loop = rp.RPClosedLoop(p, s0, float(d["dt"]))
    worst_x = worst_f = 0.0
    try:
        for j in range(1, 21):
            loop.run(100)
            k = 100 * j - 1
            assert loop.clock == 100 * j
            ex = float(np.max(np.abs(_rp_vec(loop.state) - d["states"][k])))
            ef = _rel(loop.f[0], d["f"][k])
            worst_x, worst_f = max(worst_x, ex), max(worst_f, ef)
            print(f"step {k}: state diff {ex:.2e}, f rel diff {ef:.2e}")
            assert ex < RP_STATE_ATOL, (k, ex)
            assert ef < RP_F_REL, (k, ef)
            assert loop.state.counter == 0  # 100 j steps: the projection counter has just wrapped
    finally:
        loop.close()
    print(f"rigid payload resident, 20 s: max f rel diff {worst_f:.2e}, max state diff {worst_x:.2e}")


def test_rp_per_scenario_records_and_time_offsets():
    """Scenario j < 20 starts from the recording's state before step 100 j with T0 = 100 j dt; fifty resident steps
    later it stands where the recording stands after step 100 j + 49.  The recording has 2,000 steps, so scenarios 20
    and 21 of the 22 start before steps 50 and 950 instead (projection counter 10: the counter's other phase)."""
    from distributed_aerial_transportation_amd import rigid_payload as rp
    from distributed_aerial_transportation_amd import tracking

    d = load("ref_rp.npz")
    dt = float(d["dt"])
    p, _, s0 = rp.rp_setup(3)
    starts = [100 * j for j in range(20)] + [50, 950]
    assert len(starts) == 64 // 3 + 1
    states = []
    for s in starts:
        x = d["states"][s - 1] if s else _rp_vec(s0)
        st = rp.RPState(x[:3], x[3:6], x[6:15].reshape(3, 3), x[15:18], project=False)
        st.counter = s % 20
        states.append(st)
    rec = np.stack([tracking.circle_record(t0=s * dt) for s in starts])
    loop = rp.RPClosedLoop(p, states, dt, track=rec)
    try:
        loop.run(50)
        assert loop.clock == 50
        got, f = loop.states, loop.f
    finally:
        loop.close()
    for j, s in enumerate(starts):
        k = s + 49
        ex = float(np.max(np.abs(_rp_vec(got[j]) - d["states"][k])))
        ef = _rel(f[j], d["f"][k])
        print(f"scenario {j} (steps {s} .. {k}): state diff {ex:.2e}, f rel diff {ef:.2e}")
        assert ex < RP_STATE_ATOL, (j, ex)
        assert ef < RP_F_REL, (j, ef)
        assert got[j].counter == (s + 50) % 20


# ---- 3: the quadrotor plant against the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(_track.CASES))
def test_quadrotor_plant_matches_the_oracle(name):
    from distributed_aerial_transportation_amd import BatchedController, scenarios, tracking

    c = _track.Case(load("ref_track.npz"), name)
    n, K = c.n, c.K
    eng = BatchedController(c.kind, n, 1, scenarios.params_block(n), dt=_track.DT, hl_every=_track.HL_EVERY)
    try:
        eng.set_tracking(tracking.circle_record())
        eng.set_state(c.start[None], np.zeros(1, dtype=np.int32))
        eng.log_begin(None, log_every=1, hl_capacity=K, summary=True)
        eng.closed_loop(K)
        assert eng.clock == K * _track.HL_EVERY
        log = eng.log_read()
        eng.log_end()
    finally:
        eng.close()
    iters = log["sum_iters"][:, 0]
    assert np.array_equal(iters, log["iters"][:, 0])
    # the state after HL period k: the record of simulation step 10 k + 9
    ends = log["step_index"] % _track.HL_EVERY == _track.HL_EVERY - 1
    states = log["state"][ends, 0]
    assert states.shape == c.state.shape
    excused, worst_f = 0, 0.0
    for k in range(K):
        if iters[k] != c.iters[k]:
            err = c.err[k][np.isfinite(c.err[k])]
            assert c.count_moves[k] or _ambiguous(err), (name, k, int(iters[k]), int(c.iters[k]))
            excused += 1
            continue
        bound = max(REL, F_MARGIN * float(c.sens_f[k])) if np.isfinite(c.sens_f[k]) else REL
        ef = _rel(log["f_des"][k, 0], c.f_des[k])
        worst_f = max(worst_f, ef)
        assert ef <= bound, (name, k, ef, bound)
    ex = float(np.max(np.abs(states - c.state)))
    print(f"{name}: iters {iters.tolist()}; excused {excused} of {K}; f_des worst rel {worst_f:.2e}; state diff "
          f"{ex:.2e} (oracle's own spread {float(c.state_spread):.2e})")
    assert excused <= K // 8, (name, excused)
    assert ex <= STATE_ATOL, (name, ex)


# ---- 4: the schedules ------------------------------------------------------------------------------------------------
HL = 6
SHAPES = [(6, 31), (3, 64)]
# variant: (overlap, pipeline, fused, sub-batches, forced early / late split, calls; None: host-driven steps)
VARIANTS = {
    "overlap": (True, False, False, 1, False, (HL,)),
    "overlap_fused": (True, False, True, 1, False, (HL,)),
    "overlap_fused_split": (True, False, True, 1, True, (HL,)),
    "pipeline": (True, True, False, 1, False, (HL,)),
    "pipeline_split": (True, True, False, 1, True, (HL,)),
    "pipeline_fused": (True, True, True, 1, False, (HL,)),
    "pipeline_fused_split": (True, True, True, 1, True, (HL,)),
    "sub2": (True, True, True, 2, False, (HL,)),
    "sub4": (True, True, True, 4, False, (HL,)),
    "two_calls": (True, True, True, 1, False, (2, 4)),
    "host_driven": (True, True, True, 1, False, None),
}
SERIAL = (False, False, False, 1, False, (HL,))


@functools.lru_cache(maxsize=None)
def _scene(n, B, crowd):
    """(start states, trees or None, per-scenario records): read-only, shared by the variants"""
    from distributed_aerial_transportation_amd import scenarios, tracking

    rng = np.random.default_rng(100 * n + B + crowd)
    trees = None
    if crowd:
        from tests import _envscenes as es

        cases = es.battery(n)[0]
        trees = np.array(next(c for c in cases if c.name == "crowd").trees)
        x0 = np.stack([cases[b % len(cases)].state for b in range(B)])
    else:
        x0 = scenarios.perturbed_states(n, B, rng)
    # circles about where the scenarios stand, so the tracked paths stay among the trees
    o = 12 * n
    rec = np.stack([tracking.circle_record(center=(x0[b, o] - 1.0, x0[b, o + 1]), radius=rng.uniform(0.5, 2.0),
                                           height=x0[b, o + 2], t0=rng.uniform(0.0, 10.0),
                                           amax=rng.choice([0.0, rng.uniform(0.5, 2.0)])) for b in range(B)])
    for a in (x0, rec):
        a.setflags(write=False)
    return x0, trees, rec


def _schedule_run(n, B, crowd, variant):
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    overlap, pipeline, fused, sub, split, calls = variant
    x0, trees, rec = _scene(n, B, crowd)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        if trees is not None:
            from tests.test_gpu_env_rows_reference import _forest

            eng.set_forests([_forest(trees)])
        eng.set_tracking(rec)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.set_sub_batches(sub)
        eng.set_advance_overlap(overlap)
        eng.set_step_pipeline(pipeline)
        eng.set_fused_advance(fused)
        if split:
            eng.debug_advance_split(np.arange(B) % 2 == 0)
        if calls is None:
            for _ in range(HL):
                eng.control(None, None)
                eng.rollout(eng.cfg.hl_every)
        else:
            for k in calls:
                eng.closed_loop(k)
        eng.synchronize()
        st, cnt = eng.get_state()
        return {"state": st, "counter": cnt, "blob": eng.checkpoint().tobytes(), "clock": eng.clock,
                "advance": eng.advance_counts(), "launches": eng.fused_launches(), "hl_every": eng.cfg.hl_every}
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _serial_run(n, B, crowd):
    return _schedule_run(n, B, crowd, SERIAL)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("crowd", [False, True], ids=["open", "crowd"])
@pytest.mark.parametrize("n,B", SHAPES)
def test_schedules_agree_bitwise_under_tracking(n, B, crowd, variant):
    ref = _serial_run(n, B, crowd)
    assert ref["advance"] == (0, 0) and ref["launches"] == (0, 0)
    out = _schedule_run(n, B, crowd, VARIANTS[variant])
    print(f"n = {n}, B = {B}, {variant}: advance counts {out['advance']}, launches {out['launches']}")
    overlap, pipeline, fused, sub, split, calls = VARIANTS[variant]
    if calls is not None and sub == 1:  # the schedule under test ran: the results alone could not tell
        assert sum(out["advance"]) == B * HL
        assert (out["launches"][0] > 0) == fused
        if split:
            assert out["advance"][0] > 0 and out["advance"][1] > 0
    assert out["clock"] == ref["clock"] == HL * out["hl_every"]
    assert np.array_equal(out["state"], ref["state"])
    assert np.array_equal(out["counter"], ref["counter"])
    assert out["blob"] == ref["blob"]


def test_the_tracked_loop_is_not_the_forest_loop():
    """(the comparisons above compare a law that took effect)"""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    n, B = 3, 64
    x0, _, rec = _scene(n, B, False)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.closed_loop(HL)
        st, _ = eng.get_state()
    finally:
        eng.close()
    assert not np.array_equal(st, _serial_run(n, B, False)["state"])


# ---- 5: the log ------------------------------------------------------------------------------------------------------
def test_log_records_the_tracked_references():
    from distributed_aerial_transportation_amd import BatchedController, scenarios, tracking

    n, B, K, clock0 = 3, 5, 6, 1230
    x0, _, rec = _scene(3, 64, False)
    x0, rec = x0[:B], rec[:B]
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.set_tracking(rec)
        eng.set_clock(clock0)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.log_begin(None, log_every=1, hl_capacity=K)
        eng.closed_loop(K)
        log = eng.log_read()
        eng.log_end()
        hl, dt = eng.cfg.hl_every, eng.cfg.dt
        assert eng.clock == clock0 + K * hl
    finally:
        eng.close()
    o = 12 * n
    for k in range(K):
        xr, vr, _ = tracking.references(rec, (clock0 + k * hl) * dt)
        assert np.max(np.abs(log["x_ref"][k] - xr)) <= 1e-12, k
        assert np.max(np.abs(log["v_ref"][k] - vr)) <= 1e-12, k
        # ... and the errors of the period's steps are taken against them
        for s in range(hl):
            st = log["state"][k * hl + s]
            assert np.max(np.abs(log["x_err"][k * hl + s] - np.linalg.norm(xr - st[:, o:o + 3], axis=1))) <= 1e-12
            assert np.max(np.abs(log["v_err"][k * hl + s] - np.linalg.norm(vr - st[:, o + 3:o + 6], axis=1))) <= 1e-12


def test_example_circle_resident_equals_stepwise():
    from distributed_aerial_transportation_amd import example
    from tests.test_gpu_closed_loop_log import _same_logs

    kw = dict(controller_type="consensus-admm", n=3, T=0.2, law="circle", verbose=False)
    ref = example.simulate(**kw)
    res = example.simulate(resident=True, **kw)
    assert len(ref["f_des_seq"]) == 20 and len(ref["state_seq"]) == 20 and ref["num_trees"] == 0
    _same_logs([res], [ref])
    # the errors are the tracked ones: the payload starts at rest at the origin, one metre below and beside the circle
    assert 1.0 < ref["x_err_seq"][0] < 1.5 and abs(ref["v_err_seq"][0] - 0.5) < 0.05


# ---- 6: nothing else moved ---------------------------------------------------------------------------------------
def test_forest_law_comes_back_bitwise():
    from distributed_aerial_transportation_amd import BatchedController, scenarios
    from tests.test_gpu_env_rows_reference import _forest

    n, B, K = 3, 25, 4
    x0, trees, rec = _scene(n, 64, True)
    x0, rec = x0[:B], rec[:B]

    def forest_loop(eng):
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.reset_warm_start()
        eng.closed_loop(K)
        eng.synchronize()
        return eng.get_state()[0], eng.checkpoint().tobytes()

    fresh = BatchedController("cadmm", n, B, scenarios.params_block(n))
    used = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        for eng in (fresh, used):
            eng.set_forests([_forest(trees)])
        want = forest_loop(fresh)
        used.set_tracking(rec)
        used.set_state(x0, np.zeros(B, dtype=np.int32))
        used.closed_loop(K)
        tracked = used.get_state()[0]
        assert not np.array_equal(tracked, want[0])
        used.set_tracking(None)
        got = forest_loop(used)
        assert used.clock == 2 * K * used.cfg.hl_every  # (the forest law does not read it)
    finally:
        fresh.close()
        used.close()
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]


def test_error_cases_leave_the_handle_usable():
    from distributed_aerial_transportation_amd import BatchedController, scenarios, tracking
    from distributed_aerial_transportation_amd import rigid_payload as rp
    from distributed_aerial_transportation_amd._lib import DatError

    n, B = 3, 4
    x0, _, rec = _scene(3, 64, False)
    x0, rec = x0[:B], rec[:B]
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.set_tracking(rec)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.closed_loop(2)
        want = eng.get_state()[0]
        # a bad record: nothing is copied, the records in force stay
        for field, value in (("RADIUS", -1.0), ("FREQ", -0.1), ("KP", -2.0), ("KV", -2.0), ("HEIGHT", np.nan),
                             ("T0", np.inf)):
            bad = rec.copy()
            bad[B - 1, tracking.T[field]] = value
            with pytest.raises(DatError, match=rf"record {B - 1}.*{field}"):
                eng.set_tracking(bad)
        with pytest.raises(DatError, match="negative clock"):
            eng.set_clock(-1)
        with pytest.raises(DatError, match="centralized handles only"):
            eng.set_plant("rp")
        assert eng.clock == 2 * eng.cfg.hl_every
        # the handle goes on as if nothing had been asked: the same two steps from the same start
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.reset_warm_start()
        eng.set_clock(0)
        eng.closed_loop(2)
        assert np.array_equal(eng.get_state()[0], want)
        # the clock counts the steps of rollout as well
        eng.rollout(7)
        assert eng.clock == 2 * eng.cfg.hl_every + 7
    finally:
        eng.close()
    # the RP plant and the log exclude each other, in either order
    p, _, s0 = rp.rp_setup(3)
    cent = BatchedController("centralized", 3, 1, rp.pack_rp_params(p), dt=1e-2, hl_every=1)
    try:
        cent.set_tracking(tracking.circle_record())
        cent.set_state(rp.pack_rp_state(s0, 3)[None], np.zeros(1, dtype=np.int32))
        cent.log_begin(None, hl_capacity=4)
        with pytest.raises(DatError, match="log does not record the rigid-payload plant"):
            cent.set_plant("rp")
        cent.log_end()
        cent.set_plant("rp")
        with pytest.raises(DatError, match="log does not record the rigid-payload plant"):
            cent.log_begin(None, hl_capacity=4)
        cent.closed_loop(3)
        assert cent.clock == 3
        d = load("ref_rp.npz")
        x, _ = cent.get_state()
        assert np.max(np.abs(x[0, 12 * 3:] - d["states"][2])) < RP_STATE_ATOL
        cent.rp_rollout(2)  # (the clock counts the steps of rp_rollout as well)
        assert cent.clock == 5
        cent.set_plant("rqp")
    finally:
        cent.close()
