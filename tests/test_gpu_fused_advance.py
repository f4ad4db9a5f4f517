"""The fused advance (dat_set_fused_advance): where the closed loop splits the advance into an early and a late pass
(the advance overlap, the step pipeline), a pass runs the rollout, the desired acceleration and the env rows and keys
of its scenarios in one launch, k_advance, instead of three.  k_advance calls the device functions the three kernels
call, on the same inputs in the same order, so every comparison here is bitwise (np.array_equal) between the switch
on and off, from the same start on the same handle configuration.  Under the step pipeline k_advance also counts the
sort keys it makes, and the sorts behind it only scatter (k_bucket_scatter instead of k_bucket_adv): which scenarios
share a wavefront is not fixed by either sort, a scenario's arithmetic does not depend on it, and the lane-level
work counters compared here would show a scenario listed twice or not at all.

A run is closed_loop(3), then closed_loop(2): five closed-loop steps, of which the passes after steps 1, 2 and 4
run k_advance (a call's first step takes its inputs up front and its last step only rolls out: both keep the three
kernels).  After each call the run reads the state and the rotation counters, the env rows and env class the call's
last drain consumed (dat_debug_get_env_class: written by the pass before it) and one control step from there
(f_des, iters, qp_status: it reads the warm state the loop left); at the end the lane-level work counters.  f_des is
sampled there, once per call, not at every step: a step's f_des can be read only through a log, and an open log is
one of the fall-backs that keep the three kernels.  A step's f_des is what its rollout integrates, so the states
compared after each call carry every step's.  Since the results are the same by construction whichever kernels
ran, every case also checks the launch counts of dat_get_fused_launches.

Shapes: the smallest that reach each way the block mapping (G = floor(64 / n) scenarios per 64-lane block, lane
ls * n + i) can go wrong -- one partial block; several blocks with a partial last one; 63, 60, 63 and 64 of 64 lanes
in use; and no forest, where every key is in class 0.
"""

import functools

import numpy as np
import pytest

from tests._golden import load
from tests.test_gpu_advance_overlap import WORK, _forests, _same, _start

pytestmark = pytest.mark.gpu

CALLS = (3, 2)
# k_advance and k_bucket_scatter launches of a run with the switch on under the pipeline: an early and a late pass, a
# main and a rest sort, after every step of a call but its last (steps 0, 1 of the first call, step 0 of the second)
FUSED_LAUNCHES = (6, 6)
# (6, 300): two blocks of the sort behind k_advance (k_bucket_scatter, 256 scenarios each), the last one partial and
# not the one that writes the class table
SHAPES = [(6, 7), (6, 97), (3, 43), (5, 25), (9, 15), (16, 9), (6, 300)]


def _run(n, x0, forests, sf, fused, pipeline=True, mask=None, calls=CALLS, sub=1, log=False, mode="cadmm", ll="pd"):
    """The run described above, under the low-level law ll.  Returns what the tests compare, the (early, late) advance
    counts, and (the counts and the stream count after the first call, the launches of (k_advance, k_bucket_scatter)
    of the whole run)."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    B = x0.shape[0]
    eng = BatchedController(mode, n, B, scenarios.params_block(n))
    try:
        if forests is not None:
            eng.set_forests(forests, sf)
        eng.set_state(x0, np.zeros(B, dtype=np.int32))
        eng.set_low_level(ll)
        eng.set_sub_batches(sub)
        eng.set_step_pipeline(pipeline)
        eng.set_fused_advance(fused)
        if mask is not None:
            eng.debug_advance_split(mask)
        if log:
            eng.log_begin(None, hl_capacity=sum(calls))
        out = {}
        for j, k in enumerate(calls):
            eng.closed_loop(k)
            eng.synchronize()
            out[f"state{j}"], out[f"hl_counter{j}"] = eng.get_state()
            if mode == "cadmm":
                lhs, rhs, nrow, cls = eng.debug_env_class()
                out.update({f"env_lhs{j}": lhs, f"env_rhs{j}": rhs, f"env_nrow{j}": nrow, f"env_class{j}": cls})
            if j == 0:
                counts, streams = eng.advance_counts(), eng.stream_count()
            r = eng.control(None, None)
            out.update({f"f_des{j}": r.f_des.copy(), f"iters{j}": r.iters.copy(), f"qp_status{j}": r.qp_status.copy()})
        if log:
            eng.log_end()
        total = eng.advance_counts()
        launches = eng.fused_launches()
        w = eng.work()
        out["work"] = tuple(int(w[k]) for k in WORK)
        out["min_env_dist"] = np.float64(w["min_env_dist"])
        return out, total, (counts, streams, launches)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _unfused(n, B, forest=True, pipeline=True, ll="pd"):
    """The yardstick, computed once per configuration: the same run with the switch off (the three kernels)."""
    x0, sf = _start(n, B)
    out, _, (_, _, launches) = _run(n, x0, _forests() if forest else None, sf, False, pipeline, ll=ll)
    assert launches == (0, 0)  # the switch off: the three kernels and k_bucket_adv
    return out


@pytest.mark.parametrize("n,B", SHAPES)
def test_shapes_bitwise(n, B):
    x0, sf = _start(n, B)
    out, (early, late), (_, streams, launches) = _run(n, x0, _forests(), sf, True)
    print(f"n = {n}, B = {B}: early {early}, late {late}, streams {streams}, launches {launches}")
    assert early + late == B * sum(CALLS)
    assert launches == FUSED_LAUNCHES  # the new kernels ran: the results alone could not tell
    assert streams == 4  # the handle's, the tail's, the two pipeline streams: none beyond them
    assert out["env_class0"].max() > 0  # (the forest puts env rows on some scenario)
    _same(out, _unfused(n, B))


@pytest.mark.parametrize("n,B", [(6, 97), (5, 25)])
def test_sm_law_bitwise(n, B):
    """The "sm" attitude law through k_advance: ll_control_agent's other branch is inlined into k_advance as into
    k_rollout_agents (the comment at k_low_level), so the fused run gives the bits of the three kernels under it too."""
    x0, sf = _start(n, B)
    out, (early, late), (_, _, launches) = _run(n, x0, _forests(), sf, True, ll="sm")
    assert early + late == B * sum(CALLS) and launches == FUSED_LAUNCHES
    ref = _unfused(n, B, ll="sm")
    _same(out, ref)
    assert not np.array_equal(ref["state1"], _unfused(n, B)["state1"])  # (the law took effect)


def test_without_a_forest_every_key_is_class_0():
    n, B = 6, 97
    x0, sf = _start(n, B)
    out, (early, late), (_, _, launches) = _run(n, x0, None, sf, True)
    assert early + late == B * sum(CALLS) and launches == FUSED_LAUNCHES
    assert not out["env_class0"].any() and not out["env_class1"].any() and not out["env_nrow1"].any()
    _same(out, _unfused(n, B, forest=False))


def test_overlap_schedule_bitwise():
    """Pipeline off: the advance overlap runs k_advance for both of its passes too."""
    n, B = 6, 97
    x0, sf = _start(n, B)
    out, (early, late), (_, streams, launches) = _run(n, x0, _forests(), sf, True, pipeline=False)
    assert early + late == B * sum(CALLS) and streams == 3
    assert launches == (FUSED_LAUNCHES[0], 0)  # (the overlap's one sort per step stays k_bucket)
    _same(out, _unfused(n, B, pipeline=False))
    _same(out, _unfused(n, B))  # (and the two schedules agree)


def _masks(B):
    m = {"all_early": np.ones(B, bool), "all_late": np.zeros(B, bool), "alternating": np.arange(B) % 2 == 0,
         "one_late": np.ones(B, bool), "one_early": np.zeros(B, bool)}
    m["one_late"][B // 2] = False
    m["one_early"][B - 1] = True
    return m


@pytest.mark.parametrize("which", ["all_early", "all_late", "alternating", "one_late", "one_early"])
def test_forced_split(which):
    """dat_debug_advance_split: the early k_advance takes exactly the mask, the late one the others (blocks with
    none, some and all of their scenarios taking part in either)."""
    n, B = 6, 97
    mask = _masks(B)[which]
    x0, sf = _start(n, B)
    out, (early, late), (_, _, launches) = _run(n, x0, _forests(), sf, True, mask=mask)
    steps = sum(CALLS)
    assert launches == FUSED_LAUNCHES
    assert early == int(mask.sum()) * steps and late == (B - int(mask.sum())) * steps
    _same(out, _unfused(n, B))


def test_tail_regime():
    """The two stall stretches of ref_c4_hard.npz, 4 steps from x0 (test_gpu_step_pipeline's test_tail_regime): a
    tail-routed scenario (key >= NKEY, written by k_advance) is advanced by either pass and still lands in the rest
    list."""
    from distributed_aerial_transportation_amd import Forest

    d = load("ref_c4_hard.npz")
    n, J = 6, d["x0"].shape[0]
    forests = [Forest.seeded(int(s)) for s in d["forest_seed"]]
    sf = np.arange(J, dtype=np.int32)
    ref, _, _ = _run(n, d["x0"], forests, sf, False, calls=(4,))
    w = dict(zip(WORK, ref["work"]))
    assert w["tail_routed"] > 0 and w["robust_redos"] > w["tail_routed"]
    for mask in (None, np.ones(J, bool), np.zeros(J, bool), np.array([True, False]), np.array([False, True])):
        out, (early, late), (_, _, launches) = _run(n, d["x0"], forests, sf, True, mask=mask, calls=(4,))
        assert early + late == 4 * J and launches == (6, 6)  # (the passes and sorts after steps 0, 1, 2)
        if mask is not None:
            assert early == 4 * int(mask.sum())
        _same(out, ref)


def test_fall_backs_run_the_three_kernels():
    """A log open and two sub-batches run the serial schedule, DD its own: no pass is split off (nothing counted as
    advanced early or late, which both k_advance instantiations do), no further stream, and the results stand."""
    n, B = 6, 97
    x0, sf = _start(n, B)
    for kw in ({"log": True}, {"sub": 2}):
        out, total, (_, streams, launches) = _run(n, x0, _forests(), sf, True, **kw)
        assert total == (0, 0) and streams <= 2 and launches == (0, 0), (kw, total, streams, launches)
        _same(out, _unfused(n, B))
    dd = [_run(n, x0, _forests(), sf, fused, mode="dd") for fused in (True, False)]
    assert dd[0][1] == (0, 0) and dd[0][2][1] == 1 and dd[0][2][2] == (0, 0)
    _same(dd[0][0], dd[1][0])


def test_streams_through_sub_batches_and_back():
    """The fused advance adds no stream: four after a pipelined call, given back for dat_set_sub_batches(4), made
    again back on one sub-batch."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    n, B = 6, 97
    x0, sf = _start(n, B)
    res = []
    for fused in (True, False):
        eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
        try:
            eng.set_forests(_forests(), sf)
            eng.set_state(x0, np.zeros(B, dtype=np.int32))
            eng.set_fused_advance(fused)
            seen = [eng.stream_count()]
            for sub, steps in ((1, 3), (4, 1), (1, 2)):
                eng.set_sub_batches(sub)
                seen.append(eng.stream_count())
                eng.closed_loop(steps)
                seen.append(eng.stream_count())
            assert seen == [1, 1, 4, 4, 4, 1, 4], seen
            early, late = eng.advance_counts()
            assert early + late == 5 * B  # (the sub-batch call advances nothing early or late)
            assert eng.fused_launches() == ((6, 6) if fused else (0, 0))  # (after steps 0, 1 of call 1, 0 of call 3)
            eng.synchronize()
            st, cnt = eng.get_state()
            r = eng.control(None, None)
            res.append({"state": st, "hl_counter": cnt, "f_des": r.f_des.copy(), "iters": r.iters.copy()})
        finally:
            eng.close()
    _same(res[0], res[1])
