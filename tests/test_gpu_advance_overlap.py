"""The closed loop's advance overlap (dat_set_advance_overlap): the rollout and the next step's desired acceleration
and env rows of the scenarios the C-ADMM drain has finished run beside the drain's ramp-down ("early"), the others
after it ("late").  A scenario's step is the same sequence of the same device functions on the same inputs in either
pass, so every comparison here is bitwise (np.array_equal) against the same handle configuration with the overlap
switched off: the states and rotation counters after the loop, and iters / f_des / qp_status of one more control step
from there (which also reads the warm state the loop left).  The lane-level work counters are compared as integers;
the occupancy counters are left out, they depend on which scenarios share a wavefront, which k_bucket does not fix.
"""

import functools

import numpy as np
import pytest

from tests._golden import load

pytestmark = pytest.mark.gpu

WORK = ("qp_solves", "ipm_iters", "ipm_row_iters", "hl_steps", "inband_exits", "inband_beyond_clarabel_tol",
        "refine_passes", "refine_corrections", "robust_redos", "tail_routed", "certified_infeasible", "stall_exits",
        "warm_starts", "collisions")


def _forests():
    from distributed_aerial_transportation_amd import Forest

    return [Forest.seeded(0), Forest.seeded(1)]


def _start(n, B):
    from distributed_aerial_transportation_amd import scenarios

    sf = (np.arange(B) % 2).astype(np.int32)
    return scenarios.forest_path_states(n, B, np.random.default_rng(11), _forests(), sf), sf


def _loop(n, x0, forests, sf, calls, overlap=True, pb=0, mask=None, sub=1, log=False, restate=False):
    """closed_loop(k) for every k of `calls` (restate: set_state(x0) before each call after the first), then one
    control step.  Returns what the tests compare, and the (early, late) advance counts."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    B = x0.shape[0]
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    try:
        eng.set_forests(forests, sf)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.set_persistent_blocks(pb)
        eng.set_sub_batches(sub)
        eng.set_advance_overlap(overlap)
        if mask is not None:
            eng.debug_advance_split(mask)
        if log:
            eng.log_begin(None, hl_capacity=sum(calls))
        for j, k in enumerate(calls):
            if restate and j > 0:
                eng.set_state(x0, np.zeros(B, dtype=np.int32))
            eng.closed_loop(k)
        if log:
            eng.log_end()
        eng.synchronize()
        counts = eng.advance_counts()
        st, cnt = eng.get_state()
        r = eng.control(None, None)
        w = eng.work()
        out = {"state": st, "hl_counter": cnt, "iters": r.iters.copy(), "f_des": r.f_des.copy(),
               "qp_status": r.qp_status.copy(), "work": tuple(int(w[k]) for k in WORK),
               "min_env_dist": np.float64(w["min_env_dist"])}
        return out, counts
    finally:
        eng.close()


def _same(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "work":
            assert a[key] == b[key], dict(zip(WORK, zip(a[key], b[key])))
        else:
            assert np.array_equal(a[key], b[key]), key


@functools.lru_cache(maxsize=None)
def _serial(n, B, calls, pb=0, restate=False):
    """The yardstick, computed once per configuration: the same loop with the overlap off."""
    x0, sf = _start(n, B)
    out, counts = _loop(n, x0, _forests(), sf, calls, overlap=False, pb=pb, restate=restate)
    assert counts == (0, 0)
    return out


@pytest.mark.parametrize("pb", [1, 0])
@pytest.mark.parametrize("n,B", [(6, 97), (3, 50), (16, 13)])
def test_natural_timing(n, B, pb):
    """Partial last blocks (10, 21 and 4 scenarios per block); one resident k_cadmm workgroup and the default.  The
    split between the passes depends on timing at these sizes: only its sum is fixed."""
    x0, sf = _start(n, B)
    out, (early, late) = _loop(n, x0, _forests(), sf, (6,), pb=pb)
    print(f"n = {n}, B = {B}, persistent_blocks = {pb}: early {early}, late {late}")
    assert early + late == B * 6
    _same(out, _serial(n, B, (6,), pb))


def _masks(B):
    m = {"all": np.ones(B, bool), "none": np.zeros(B, bool), "alternating": np.arange(B) % 2 == 0,
         "block_late": np.ones(B, bool), "last_only": np.zeros(B, bool)}
    m["block_late"][20:30] = False  # the rollout's third block of 10 scenarios (n = 6)
    m["last_only"][B - 1] = True
    return m


@pytest.mark.parametrize("which", ["all", "none", "alternating", "block_late", "last_only"])
def test_forced_split(which):
    """dat_debug_advance_split: the early pass takes exactly the masked scenarios, after the drain.  In three of the
    five masks both passes handle scenarios (asserted through the counts)."""
    n, B, steps = 6, 97, 4
    mask = _masks(B)[which]
    x0, sf = _start(n, B)
    out, (early, late) = _loop(n, x0, _forests(), sf, (steps,), mask=mask)
    assert early == int(mask.sum()) * steps and late == (B - int(mask.sum())) * steps
    if which in ("alternating", "block_late", "last_only"):
        assert early > 0 and late > 0
    _same(out, _serial(n, B, (steps,)))


def test_tail_kernel_stamps():
    """The two stall stretches of ref_c4_hard.npz, 4 steps from x0.  In a scenario's first stalled step k_cadmm
    hands it to k_cadmm_tail (the tail rule: the hand-over lists, tmode 0), from the next step on k_env_class routes
    it to the tail launch beside k_cadmm (tmode 1): the done stamps of those steps are written by k_cadmm_tail, in
    both of its modes, while k_cadmm's class-0 queue is empty from the start.  (Routing cannot be switched off
    without sub-batches, which keep the serial schedule: the hand-over mode is reached through the first stalled
    step instead, and the counters below show that both modes finished scenario-steps.)"""
    from distributed_aerial_transportation_amd import Forest

    d = load("ref_c4_hard.npz")
    n, J = 6, d["x0"].shape[0]
    forests = [Forest.seeded(int(s)) for s in d["forest_seed"]]
    sf = np.arange(J, dtype=np.int32)
    ref, c0 = _loop(n, d["x0"], forests, sf, (4,), overlap=False)
    out, (early, late) = _loop(n, d["x0"], forests, sf, (4,))
    assert c0 == (0, 0) and early + late == 4 * J
    w = dict(zip(WORK, out["work"]))
    # (scenario-steps the tail finished: some routed before the step, some taken from the hand-over lists)
    assert w["tail_routed"] > 0 and w["robust_redos"] > w["tail_routed"]
    _same(out, ref)
    # the same with the split forced either way: the tail's stamps are what the early pass goes by
    for mask in (np.ones(J, bool), np.array([True, False])):
        out, (early, late) = _loop(n, d["x0"], forests, sf, (4,), mask=mask)
        assert early == 4 * int(mask.sum())
        _same(out, ref)


def test_call_boundaries():
    """The serial runs on across calls, the last step of a call leaves no early env rows behind, and the next call
    recomputes its first step's desired acceleration and env rows from the state (which set_state replaces)."""
    n, B = 6, 97
    x0, sf = _start(n, B)
    f = _forests()
    mask = np.arange(B) % 3 != 0
    for kw in ({}, {"mask": mask}):
        out, (early, late) = _loop(n, x0, f, sf, (3, 3), restate=True, **kw)
        assert early + late == 6 * B
        _same(out, _serial(n, B, (3, 3), 0, True))
        out, (early, late) = _loop(n, x0, f, sf, (2, 2, 2), **kw)
        assert early + late == 6 * B
        _same(out, _serial(n, B, (6,)))
    out, _ = _loop(n, x0, f, sf, (6,), mask=mask)
    _same(out, _serial(n, B, (6,)))


def test_fall_backs():
    """With a log open and with sub-batches the serial schedule runs: nothing is advanced early."""
    n, B = 6, 97
    x0, sf = _start(n, B)
    ref = _serial(n, B, (4,))
    out, counts = _loop(n, x0, _forests(), sf, (4,), log=True)
    assert counts == (0, 0)
    _same(out, ref)
    out, counts = _loop(n, x0, _forests(), sf, (4,), sub=4)
    assert counts == (0, 0)
    _same(out, ref)
