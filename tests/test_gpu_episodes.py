"""Episodes in the resident closed loop (dat_episode_*): a scenario's episode ends after its control step and before
its rollout, its outcome is recorded once and its slot takes the next record of a device-resident pool.

1. a respawn is a restore: every outcome, and every slot's live state, against a fresh handle that restores the pool
   record and runs the episode's steps host-driven (control, rollout), bitwise; C-ADMM, DD, centralized;
2. every schedule of the closed loop against the serial one, bitwise, under rules that end about half the records at
   their first step; the early pass of the overlapped schedules respawns nothing and leaves the ending scenarios to
   the rest pass;
3. the reference controller's own stall (ref_c4_hard.npz) and collision (c4_collision.npz) end as STALL and COLLISION;
4. the table's capacity, idle slots without wrap, the exclusions, and the plain loop after episodes_end."""

import functools

import numpy as np
import pytest

from tests._golden import load

pytestmark = pytest.mark.gpu


def _R():
    from distributed_aerial_transportation_amd import layout

    return layout.EP_REASONS


@functools.lru_cache(maxsize=None)
def _pool(kind, n, P, crowd=False, seed=7):
    """(blob of P records with the constructor's warm state, their states): read-only, shared"""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    rng = np.random.default_rng(seed + 100 * n + P)
    if crowd:
        from tests import _envscenes as es

        cases = es.battery(n)[0]
        x = np.stack([cases[b % len(cases)].state for b in range(P)])
    else:
        x = scenarios.perturbed_states(n, P, rng)
    eng = BatchedController(kind, n, P, scenarios.params_block(n))
    try:
        eng.set_state(x, np.zeros(P, dtype=np.int32))
        blob = eng.checkpoint().tobytes()
    finally:
        eng.close()
    x.setflags(write=False)
    return blob, x


def _replay(kind, n, blob, records, steps, forest=None):
    """A fresh handle restores blob record records[k] into scenario k and runs steps[k] >= 1 control steps of it
    host-driven, control() then rollout().  Returns per scenario the state its last control step saw (the run
    without the last rollout), the sum and maximum of iters and the smallest distance over its steps, and, for the
    live-state comparison, the state and the checkpoint record after the last rollout."""
    from distributed_aerial_transportation_amd import BatchedController, Checkpoint, scenarios

    K = len(records)
    eng = BatchedController(kind, n, K, scenarios.params_block(n))
    try:
        if forest is not None:
            eng.set_forests([forest])
        eng.restore(Checkpoint.frombytes(blob), records=records)
        T = int(max(steps))
        S = 12 * n + 18
        term = np.zeros((K, S))
        after = np.zeros((K, S))
        isum, imax, mind = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64), np.full(K, np.inf)
        blobs = [None] * K
        for t in range(T):
            r = eng.control(None, None)
            pre = eng.get_state()[0]
            live = np.asarray(steps) > t
            isum[live] += r.iters[live]
            imax[live] = np.maximum(imax[live], r.iters[live])
            mind[live] = np.minimum(mind[live], r.min_env_dist[live])
            last = np.asarray(steps) == t + 1
            term[last] = pre[last]
            eng.rollout(eng.cfg.hl_every)
            post = eng.get_state()[0]
            after[last] = post[last]
            if last.any():
                ck = eng.checkpoint(np.nonzero(last)[0])
                for j, k in enumerate(np.nonzero(last)[0]):
                    blobs[k] = ck.select([j]).tobytes()
        return term, isum, imax, mind, after, blobs
    finally:
        eng.close()


# ---- 1: a respawn is a restore -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,B", [("cadmm", 3, 22), ("dd", 3, 5), ("centralized", 3, 5)])
def test_a_respawn_is_a_restore(kind, n, B):
    from distributed_aerial_transportation_amd import BatchedController, Checkpoint, scenarios

    P, HL, MAXS = 2 * B + 5, 7, 3
    blob, x = _pool(kind, n, P)
    o = 12 * n
    eng = BatchedController(kind, n, B, scenarios.params_block(n))
    try:
        eng.set_advance_overlap(False)  # the serial schedule
        eng.episodes_begin(Checkpoint.frombytes(blob), max_steps=MAXS)
        assert np.array_equal(eng.get_state()[0], x[:B])  # slot s runs record s first
        eng.closed_loop(HL)
        out = eng.episodes_read()
        counts = eng.episodes_counts()
        slots = eng.episodes_slots()
        live, _ = eng.get_state()
        live_blob = eng.checkpoint()
        hl = eng.cfg.hl_every
    finally:
        eng.close()
    R = _R()
    K = len(out["slot"])
    assert K == B * (HL // MAXS) and counts["ended"]["TIME_LIMIT"] == K and counts["lost"] == 0
    assert np.all(out["reason"] == R["TIME_LIMIT"]) and np.all(out["steps"] == MAXS)
    assert np.array_equal(out["record"], (out["slot"] + out["episode"] * B) % P)
    assert np.array_equal(out["end_tick"], out["start_tick"] + (MAXS - 1) * hl)
    assert np.array_equal(out["start_tick"], out["episode"] * MAXS * hl)
    term, isum, imax, mind, _, _ = _replay(kind, n, blob, out["record"], out["steps"])
    assert np.array_equal(out["xl"], term[:, o:o + 3])
    assert np.array_equal(out["vl"], term[:, o + 3:o + 6])
    assert np.array_equal(out["iter_sum"], isum) and np.array_equal(out["iter_max"], np.maximum(imax, 0))
    assert np.array_equal(out["min_env_dist"], mind)
    # every slot's live scenario: its current record restored, plus the steps of its running episode, rolled out
    assert np.array_equal(slots["episodes"], np.full(B, HL // MAXS)) and np.all(slots["steps"] == HL % MAXS)
    assert np.array_equal(slots["record"], (np.arange(B) + slots["episodes"] * B) % P)
    _, _, _, _, after, blobs = _replay(kind, n, blob, slots["record"], slots["steps"])
    assert np.array_equal(live, after)
    for s in range(B):
        assert live_blob.select([s]).tobytes() == blobs[s], s


# ---- 2: the schedules ------------------------------------------------------------------------------------------------
HL = 6
SHAPES = [(6, 31), (3, 64)]
# test_gpu_tracking.py's table without the host-driven row:
# (overlap, pipeline, fused, sub-batches, forced early / late split, calls)
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
}
SERIAL = (False, False, False, 1, False, (HL,))


def _schedule_run(n, B, crowd, variant):
    from distributed_aerial_transportation_amd import BatchedController, Checkpoint, scenarios

    overlap, pipeline, fused, sub, split, calls = variant
    P = 2 * B + 5
    blob, x = _pool("cadmm", n, P, crowd)
    goal = float(np.median(x[:, 12 * n]))
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        if crowd:
            from tests import _envscenes as es
            from tests.test_gpu_env_rows_reference import _forest

            eng.set_forests([_forest(np.array(next(c for c in es.battery(n)[0] if c.name == "crowd").trees))])
        # One resident workgroup (a scenario's arithmetic does not depend on it): the drain's slots are refilled, so
        # by the time its last queue is claimed empty all but one wavefront's scenarios (at most floor(64 / n)) are
        # finished and stamped, and the early pass has scenarios to take by construction, not by timing (with the
        # whole batch in flight at once it took 0 to 7 of 186 scenario-steps, as the drain's ramp-down fell).
        eng.set_persistent_blocks(1)
        eng.set_sub_batches(sub)
        eng.set_advance_overlap(overlap)
        eng.set_step_pipeline(pipeline)
        eng.set_fused_advance(fused)
        if split:
            eng.debug_advance_split(np.arange(B) % 2 == 0)
        # (the two rules alone: among the crowd's trees the collision rule would end 56 of 64 records at their first
        # step instead of about half; test 3 covers it)
        eng.episodes_begin(Checkpoint.frombytes(blob), goal_x=goal, max_steps=3, on_collision=False,
                           capacity=B * HL)
        for k in calls:
            eng.closed_loop(k)
        eng.synchronize()
        st, cnt = eng.get_state()
        return {"state": st, "counter": cnt, "blob": eng.checkpoint().tobytes(), "clock": eng.clock,
                "advance": eng.advance_counts(), "launches": eng.fused_launches(), "table": eng.episodes_read(),
                "counts": eng.episodes_counts(), "slots": eng.episodes_slots(), "respawns": eng.episodes_respawns(),
                "hl_every": eng.cfg.hl_every}
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _serial_run(n, B, crowd):
    return _schedule_run(n, B, crowd, SERIAL)


@pytest.mark.parametrize("crowd", [False, True], ids=["open", "crowd"])
@pytest.mark.parametrize("n,B", SHAPES)
def test_the_serial_comparison_bites(n, B, crowd):
    ref = _serial_run(n, B, crowd)
    R = _R()
    t = ref["table"]
    assert ref["advance"] == (0, 0) and ref["launches"] == (0, 0)
    assert ref["counts"]["lost"] == 0 and ref["counts"]["held"] == len(t["slot"]) == ref["counts"]["ended"]["total"]
    assert ref["counts"]["ended"]["GOAL"] > 0 and ref["counts"]["ended"]["TIME_LIMIT"] > 0
    assert set(np.unique(t["reason"])) == {R["GOAL"], R["TIME_LIMIT"]}
    per_step = np.bincount((t["end_tick"] // ref["hl_every"]).astype(int), minlength=HL)
    print(f"n = {n}, B = {B}: ended per HL step {per_step.tolist()}, by reason {ref['counts']['ended']}")
    assert np.any((per_step > 0) & (per_step < B)), per_step
    # ... and in the open field, at the first step, whose drain holds every scenario, more scenarios go on than one
    # wavefront holds: the early pass of the overlapped schedules (one resident workgroup, _schedule_run) has
    # scenarios to advance whatever the timing.  (The crowd's records stand in a few columns of equal x, so the
    # median ends most of them at once -- 27 of 31 at the first step at n = 6; there the early pass takes the
    # scenarios that go on unless all of them are among the last floor(64 / n) the drain claims.)
    if not crowd:
        assert B - 64 // n - per_step[0] > 0, per_step
    assert ref["respawns"][0] == 0 and ref["respawns"][1] == len(t["slot"]) and ref["respawns"][2] == 0
    # the goal rule ends an episode at its first step where the record already stands past the goal
    first = t["steps"] == 1
    assert first.any() and np.all(t["reason"][first] == R["GOAL"])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("crowd", [False, True], ids=["open", "crowd"])
@pytest.mark.parametrize("n,B", SHAPES)
def test_schedules_agree_bitwise_with_episodes(n, B, crowd, variant):
    ref = _serial_run(n, B, crowd)
    out = _schedule_run(n, B, crowd, VARIANTS[variant])
    overlap, pipeline, fused, sub, split, calls = VARIANTS[variant]
    print(f"n = {n}, B = {B}, {variant}: advance counts {out['advance']}, launches {out['launches']}, respawns "
          f"(early, rest, deferred) {out['respawns']}")
    if sub == 1:  # the schedule under test ran: the results alone could not tell
        assert sum(out["advance"]) == B * HL
        assert (out["launches"][0] > 0) == fused
        if pipeline:
            assert out["advance"][0] > 0
        if split:
            assert out["advance"][0] > 0 and out["advance"][1] > 0
            assert out["respawns"][0] == 0 and out["respawns"][1] > 0 and out["respawns"][2] > 0
    assert out["respawns"][0] == 0
    assert out["respawns"][1] == ref["respawns"][1]
    assert out["clock"] == ref["clock"] == HL * out["hl_every"]
    assert np.array_equal(out["state"], ref["state"])
    assert np.array_equal(out["counter"], ref["counter"])
    assert out["blob"] == ref["blob"]
    assert out["counts"] == ref["counts"]
    for k in ref["table"]:
        assert np.array_equal(out["table"][k], ref["table"][k]), k
    for k in ref["slots"]:
        assert np.array_equal(out["slots"][k], ref["slots"][k]), k


# ---- 3: the reference's own stall and collision ------------------------------------------------------------------------
def test_reference_stall_ends_as_stall():
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios

    d = load("ref_c4_hard.npz")
    n, J = 6, d["x0"].shape[0]
    assert np.all(d["iters"][:, 1:4] == 101) and np.all(d["iters"][:, 0] < 101)
    eng = BatchedController("cadmm", n, J, scenarios.params_block(n))
    try:
        eng.set_forests([Forest.seeded(int(s)) for s in d["forest_seed"]], np.arange(J, dtype=np.int32))
        eng.set_state(d["x0"], np.zeros(J, dtype=np.int32))
        eng.episodes_begin(stall_steps=3, on_collision=False)
        eng.closed_loop(5)
        t = eng.episodes_read()
    finally:
        eng.close()
    R = _R()
    for s in range(J):
        k = np.nonzero(t["slot"] == s)[0][0]  # (sorted by end tick: the slot's first outcome)
        assert t["episode"][k] == 0 and t["reason"][k] == R["STALL"], (s, t["reason"][k])
        assert t["steps"][k] == 4 and t["full_steps"][k] == 3 and t["stall_run"][k] == 3
        assert t["iter_max"][k] == 101 and t["iter_sum"][k] == int(d["iters"][s, :4].sum())


def test_reference_collision_ends_as_collision():
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios

    d = load("c4_collision.npz")
    n, Q = 6, len(d["ids"])
    eng = BatchedController("cadmm", n, Q, scenarios.params_block(n))
    try:
        eng.set_qp_tolerance(1e-10)
        eng.set_forests([Forest.seeded(s) for s in range(64)], d["forest"].astype(np.int32))
        eng.set_state(d["st0"], d["c0"])
        eng.episodes_begin(on_collision=True)
        eng.closed_loop(5)
        t = eng.episodes_read()
    finally:
        eng.close()
    R = _R()
    for q in range(Q):
        first = int(d["first"][q] - d["s0"][q])
        assert first == 3
        k = np.nonzero(t["slot"] == q)[0][0]
        assert t["reason"][k] == R["COLLISION"] and t["steps"][k] == first + 1
        assert t["iter_sum"][k] == int(d["iters"][:first + 1, q].sum())
        print(f"scenario {q}: smallest distance {t['min_env_dist'][k]:.12f}, the fixture's at the step "
              f"{float(d['min_env_dist'][first, q]):.12f}")
        assert abs(t["min_env_dist"][k] - float(d["min_env_dist"][first, q])) <= 1e-9


# ---- 4: overflow, idle, errors -----------------------------------------------------------------------------------------
def test_table_overflow_keeps_the_totals():
    from distributed_aerial_transportation_amd import BatchedController, Checkpoint, scenarios
    from distributed_aerial_transportation_amd._lib import DatError

    n, B = 3, 5
    blob, _ = _pool("cadmm", n, 2 * B + 5)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.episodes_begin(Checkpoint.frombytes(blob), max_steps=2, capacity=3)
        eng.closed_loop(4)
        c = eng.episodes_counts()
        assert c["ended"]["TIME_LIMIT"] == c["ended"]["total"] == 2 * B and c["held"] == 3 and c["lost"] == 2 * B - 3
        with pytest.raises(DatError, match="lost to the table's capacity"):
            eng.episodes_read()
        t = eng.episodes_read(allow_lost=True)
        assert len(t["slot"]) == 3 and np.all(t["steps"] == 2)
        assert np.all(eng.episodes_slots()["episodes"] == 2)  # every episode ended and respawned all the same
        eng.episodes_clear()
        c = eng.episodes_counts()
        assert c["held"] == 0 and c["lost"] == 0 and c["ended"]["total"] == 2 * B
        eng.closed_loop(1)
        assert eng.episodes_counts()["held"] == 0
        eng.closed_loop(1)
        assert eng.episodes_counts()["held"] == 3 and eng.episodes_counts()["ended"]["total"] == 3 * B
    finally:
        eng.close()


def test_without_wrap_the_slots_go_idle():
    from distributed_aerial_transportation_amd import BatchedController, Checkpoint, scenarios

    n, B = 3, 5
    P = B + 2
    blob, _ = _pool("cadmm", n, P)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.episodes_begin(Checkpoint.frombytes(blob), max_steps=2, wrap=False)
        assert eng.episodes_counts()["idle"] == 0
        eng.closed_loop(2)  # every slot's first episode ends: slots 0, 1 take records 5, 6, the others go idle
        assert eng.episodes_counts()["idle"] == B - 2
        s = eng.episodes_slots()
        assert np.array_equal(s["idle"], np.arange(B) >= 2)
        assert np.array_equal(s["record"], [5, 6, 2, 3, 4])
        eng.closed_loop(2)
        assert eng.episodes_counts()["idle"] == B
        eng.closed_loop(4)  # idle slots run on and record nothing
        c = eng.episodes_counts()
        t = eng.episodes_read()
        assert c["idle"] == B and c["ended"]["total"] == P == len(t["slot"])
        assert np.array_equal(np.sort(t["record"]), np.arange(P))  # every record of the pool, once
        assert np.array_equal(eng.episodes_slots()["record"], np.arange(B) % P)
        assert t["end_tick"].max() == 3 * eng.cfg.hl_every
    finally:
        eng.close()


def test_monte_carlo_runs_every_start_once():
    from distributed_aerial_transportation_amd import example

    n, B, P = 3, 4, 11
    _, x = _pool("cadmm", n, P)
    t = example.monte_carlo("consensus-admm", n, x, [], dict(max_steps=2), B, chunk_hl=3)
    assert np.array_equal(np.sort(t["record"]), np.arange(P)) and np.all(t["steps"] == 2)
    assert t["hl_steps"] == 6  # three episodes of two steps in the busiest slots


def test_exclusions_and_the_plain_loop_afterwards():
    from distributed_aerial_transportation_amd import BatchedController, Checkpoint, scenarios, tracking
    from distributed_aerial_transportation_amd import rigid_payload as rp
    from distributed_aerial_transportation_amd._lib import DatError

    n, B, K = 3, 6, 3
    blob, x = _pool("cadmm", n, B)
    pool = Checkpoint.frombytes(blob)

    def plain(eng):
        eng.restore(pool)
        eng.closed_loop(K)
        eng.synchronize()
        return eng.get_state()[0], eng.checkpoint().tobytes()

    fresh = BatchedController("cadmm", n, B, scenarios.params_block(n))
    used = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        want = plain(fresh)
        with pytest.raises(DatError, match="no episodes open"):
            used.episodes_counts()
        # a log and episodes, in either order
        used.log_begin(None, hl_capacity=4)
        with pytest.raises(DatError, match="log does not record episodes"):
            used.episodes_begin(pool, max_steps=2)
        used.log_end()
        used.set_tracking(tracking.circle_record())
        with pytest.raises(DatError, match="tracking records"):
            used.episodes_begin(pool, max_steps=2)
        used.set_tracking(None)
        # bad arguments: nothing opens
        for kw, word in ((dict(capacity=-1), "negative capacity"), (dict(max_steps=-1), "negative max_steps"),
                         (dict(bound=0.0), "bound must be"), (dict(goal_x=np.nan), "goal_x is NaN")):
            with pytest.raises(DatError, match=word):
                used.episodes_begin(pool, **kw)
        with pytest.raises(DatError, match="records take"):
            used.episodes_begin(blob[:-8], max_steps=2)
        with pytest.raises(DatError, match="mode"):
            used.episodes_begin(_pool("dd", n, B)[0], max_steps=2)
        with pytest.raises(DatError, match="no episodes open"):
            used.episodes_end()
        used.episodes_begin(pool, max_steps=2)
        with pytest.raises(DatError, match="already open"):
            used.episodes_begin(pool, max_steps=2)
        with pytest.raises(DatError, match="log does not record episodes"):
            used.log_begin(None, hl_capacity=4)
        with pytest.raises(DatError, match="tracking records"):
            used.set_tracking(tracking.circle_record())
        with pytest.raises(DatError, match="episodes are open"):
            used.restore(pool)
        assert used._lib.dat_episode_read(used._h, 0, 1, *([None] * 14)) < 0  # (no record is held yet)
        assert b"must lie in the 0 held" in used._lib.dat_last_error()
        assert used.checkpoint().tobytes() == blob  # saving is allowed (and begin loaded record s into slot s)
        used.closed_loop(4)
        assert used.episodes_counts()["ended"]["TIME_LIMIT"] == 2 * B
        used.episodes_end()
        got = plain(used)
    finally:
        fresh.close()
        used.close()
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    # centralized handles: no stall rule, and the rigid-payload plant and episodes exclude each other
    p, _, s0 = rp.rp_setup(3)
    cent = BatchedController("centralized", 3, 1, rp.pack_rp_params(p), dt=1e-2, hl_every=1)
    try:
        cent.set_state(rp.pack_rp_state(s0, 3)[None], np.zeros(1, dtype=np.int32))
        with pytest.raises(DatError, match="stall rule"):
            cent.episodes_begin(stall_steps=3)
        cent.set_plant("rp")
        with pytest.raises(DatError, match="rigid-payload plant"):
            cent.episodes_begin(max_steps=2)
        cent.set_plant("rqp")
        cent.episodes_begin(max_steps=2)
        with pytest.raises(DatError, match="rigid-payload plant"):
            cent.set_plant("rp")
        cent.episodes_end()
        cent.set_plant("rp")
        cent.closed_loop(2)
        assert cent.clock == 2
    finally:
        cent.close()
