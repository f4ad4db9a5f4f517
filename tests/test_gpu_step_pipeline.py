"""The closed loop's step pipeline (dat_set_step_pipeline): the next step's drain of the scenarios the early pass has
advanced ("main") starts beside the current drain's ramp-down, the others' drain ("rest") follows the late pass.  A
scenario's step is the same sequence of the same device functions on the same inputs whichever drain and pass run
it, so every comparison here is bitwise (np.array_equal) between the three schedules of the same handle
configuration: pipeline on, pipeline off (the advance overlap) and the serial schedule.  Compared: the states and
rotation counters after closed_loop(3) and closed_loop(2), iters / f_des / qp_status of one more control step from
there (which reads the warm state the loop left), and the lane-level work counters as integers (the occupancy
counters depend on which scenarios share a wavefront, which the sort does not fix).

Shapes: n = 3 with 7 and 23 scenarios (one wavefront of 21 slots; one full and a partial one), n = 6 with 21 (two
full wavefronts of 10 slots and a partial one) and 131 (more rollout blocks than one, 14).
"""

import functools

import numpy as np
import pytest

from tests._golden import load
from tests.test_gpu_advance_overlap import WORK, _forests, _same, _start

pytestmark = pytest.mark.gpu

SHAPES = [(3, 7), (3, 23), (6, 21), (6, 131)]
CALLS = (3, 2)
SCHEDULES = {"pipeline": (True, True), "overlap": (True, False), "serial": (False, False)}


def _result(eng):
    eng.synchronize()
    st, cnt = eng.get_state()
    r = eng.control(None, None)
    w = eng.work()
    return {"state": st, "hl_counter": cnt, "iters": r.iters.copy(), "f_des": r.f_des.copy(),
            "qp_status": r.qp_status.copy(), "work": tuple(int(w[k]) for k in WORK),
            "min_env_dist": np.float64(w["min_env_dist"])}


def _loop(n, x0, forests, sf, schedule, mask=None, calls=CALLS, sub=1, log=False, mode="cadmm"):
    """closed_loop(k) for every k of `calls` in the named schedule, then one control step.  Returns what the tests
    compare, the (early, late) advance counts and the handle's stream count after the loop."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    B = x0.shape[0]
    overlap, pipeline = SCHEDULES[schedule]
    eng = BatchedController(mode, n, B, scenarios.params_block(n))
    try:
        eng.set_forests(forests, sf)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.set_sub_batches(sub)
        eng.set_advance_overlap(overlap)
        eng.set_step_pipeline(pipeline)
        if mask is not None:
            eng.debug_advance_split(mask)
        if log:
            eng.log_begin(None, hl_capacity=sum(calls))
        for k in calls:
            eng.closed_loop(k)
        if log:
            eng.log_end()
        eng.synchronize()
        counts, streams = eng.advance_counts(), eng.stream_count()
        return _result(eng), counts, streams
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _yardstick(n, B, schedule):
    """Computed once per shape: the same loop in the overlap or the serial schedule."""
    x0, sf = _start(n, B)
    out, counts, streams = _loop(n, x0, _forests(), sf, schedule)
    assert streams == (2 if schedule == "serial" else 3)  # the handle's and the tail's; the advance stream
    if schedule == "serial":
        assert counts == (0, 0)
    return out


@pytest.mark.parametrize("n,B", SHAPES)
def test_three_schedules_bitwise_and_natural_timing(n, B):
    """Cases 1 and 3: no mask, so the split between the drains is what the timing makes it; only its sum is fixed."""
    x0, sf = _start(n, B)
    out, (early, late), streams = _loop(n, x0, _forests(), sf, "pipeline")
    print(f"n = {n}, B = {B}: early {early}, late {late}, streams {streams}")
    assert early + late == B * sum(CALLS)
    assert streams == 4  # the handle's, the tail's, the two pipeline streams
    _same(_yardstick(n, B, "overlap"), _yardstick(n, B, "serial"))
    _same(out, _yardstick(n, B, "overlap"))


def _masks(B):
    m = {"all_early": np.ones(B, bool), "all_late": np.zeros(B, bool), "alternating": np.arange(B) % 2 == 0,
         "one_late": np.ones(B, bool), "one_early": np.zeros(B, bool)}
    m["one_late"][B // 2] = False
    m["one_early"][B - 1] = True
    return m


@pytest.mark.parametrize("which", ["all_early", "all_late", "alternating", "one_late", "one_early"])
@pytest.mark.parametrize("n,B", SHAPES)
def test_forced_split(n, B, which):
    """dat_debug_advance_split: the early pass follows both drains of its step and takes exactly the mask, so the
    main drain of the next step holds the masked scenarios and the rest drain the others: any partition."""
    mask = _masks(B)[which]
    x0, sf = _start(n, B)
    out, (early, late), _ = _loop(n, x0, _forests(), sf, "pipeline", mask=mask)
    steps = sum(CALLS)
    assert early == int(mask.sum()) * steps and late == (B - int(mask.sum())) * steps
    _same(out, _yardstick(n, B, "overlap"))


def test_tail_regime():
    """The two stall stretches of ref_c4_hard.npz, 4 steps from x0 (as test_gpu_advance_overlap's
    test_tail_kernel_stamps): in a scenario's first stalled step k_cadmm hands it to the tail kernel, from the next
    step on the sort routes it to the tail launch beside the drain.  A routed scenario is always sorted into the rest
    drain (one tail launch per step holds them all); the hand-over happens in the drain the split puts the scenario
    in: by natural timing and with every scenario early in main drains, with every scenario late in rest drains, with
    one of each in both."""
    from distributed_aerial_transportation_amd import Forest

    d = load("ref_c4_hard.npz")
    n, J = 6, d["x0"].shape[0]
    forests = [Forest.seeded(int(s)) for s in d["forest_seed"]]
    sf = np.arange(J, dtype=np.int32)
    ref, _, _ = _loop(n, d["x0"], forests, sf, "overlap", calls=(4,))
    w = dict(zip(WORK, ref["work"]))
    assert w["tail_routed"] > 0 and w["robust_redos"] > w["tail_routed"]
    for mask in (None, np.ones(J, bool), np.zeros(J, bool), np.array([True, False]), np.array([False, True])):
        out, (early, late), _ = _loop(n, d["x0"], forests, sf, "pipeline", mask=mask, calls=(4,))
        assert early + late == 4 * J
        if mask is not None:
            assert early == 4 * int(mask.sum())
        _same(out, ref)  # (the work counters hold the tail's: routed, redone, certified, stall exits, warm starts)


def test_fall_backs_keep_their_schedule():
    """A log open and two sub-batches run the serial schedule (nothing advanced early, no pipeline stream made), DD
    its own; the results are the overlap schedule's."""
    n, B = 6, 21
    x0, sf = _start(n, B)
    for kw in ({"log": True}, {"sub": 2}):
        out, counts, streams = _loop(n, x0, _forests(), sf, "pipeline", **kw)
        assert counts == (0, 0) and streams <= 2, (kw, counts, streams)
        _same(out, _yardstick(n, B, "overlap"))
    dd = [_loop(n, x0, _forests(), sf, s, mode="dd") for s in ("pipeline", "overlap")]
    assert dd[0][1] == (0, 0) and dd[0][2] == 1
    _same(dd[0][0], dd[1][0])


def test_streams_are_given_back():
    """After a pipelined call the handle holds four streams; dat_set_sub_batches(4) gives the tail's and the
    pipeline's back before it makes its own, and back on one sub-batch the pipeline makes its streams again."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    n, B = 3, 23
    x0, sf = _start(n, B)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.set_forests(_forests(), sf)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        seen = [eng.stream_count()]
        for sub, steps in ((1, 3), (4, 1), (1, 1)):
            eng.set_sub_batches(sub)
            seen.append(eng.stream_count())
            eng.closed_loop(steps)
            seen.append(eng.stream_count())
        print("streams:", seen)
        assert seen == [1, 1, 4, 4, 4, 1, 4]
        early, late = eng.advance_counts()
        assert early + late == 4 * B  # (the sub-batch call advances nothing early or late)
        _same(_result(eng), _yardstick_mixed(n, B))
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _yardstick_mixed(n, B):
    x0, sf = _start(n, B)
    return _loop(n, x0, _forests(), sf, "serial", calls=(3, 1, 1))[0]


def test_two_handles_alternate():
    """Two handles of different team sizes (n = 6, then n = 3) pipelining in turn on one device: each launch of a
    drain carries its own dynamic LDS size."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    shapes = [(6, 21), (3, 23)]
    engs = []
    try:
        for n, B in shapes:
            x0, sf = _start(n, B)
            eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
            engs.append(eng)
            eng.set_forests(_forests(), sf)
            eng.set_state(x0, np.zeros(B, dtype=np.int32))
        for k in CALLS:
            for eng in engs:
                eng.closed_loop(k)
        for eng, (n, B) in zip(engs, shapes):
            early, late = eng.advance_counts()
            assert early + late == B * sum(CALLS) and eng.stream_count() == 4
            _same(_result(eng), _yardstick(n, B, "overlap"))
    finally:
        for eng in engs:
            eng.close()
