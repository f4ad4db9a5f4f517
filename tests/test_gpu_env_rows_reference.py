"""The device env rows against the long-double reference (tests/_envref.py) over the scene battery
(tests/_envscenes.py), and the rows k_cadmm consumes against them.

a. k_env (dat_env_rows: the serial env_rows of csrc/dat_core.hpp, device build) against the reference, at the bars of
   test_gpu_env_rows_match_oracle: atol 1e-9 on the rows, 1e-8 on min_env_dist.
b. k_env_class (env_rows_coop: one tree per lane, chunks of n candidates through LDS) against k_env on the same
   handle, bit for bit, through dat_debug_get_env_class: after a control step, and after closed_loop(1) on 1, 2 and
   3 sub-batches (dat_control_step always runs the whole batch as one block of the row image; the sub-batch blocks
   of sub_kargs exist in the closed loop only).
c. the gated instantiations of k_env_class (advance overlap, step pipeline, with a forced early / rest split)
   against k_env on a twin handle one period behind.

Worst deviations of k_env from the reference measured over the battery on an MI355X (no bar is derived from them):
row entry 4.6e-14, min_env_dist 1.3e-15 (cadmm and dd handles; centralized 3.6e-14, 1.3e-15)."""

import copy
import functools

import numpy as np
import pytest

from tests import _envref as er
from tests import _envscenes as es

pytestmark = pytest.mark.gpu

CLASS_ROWS = (0, 2, 5, 10)  # class_env_rows, csrc/dat_kargs.hpp


@functools.lru_cache(maxsize=None)
def _template():
    from distributed_aerial_transportation_amd import Forest

    return Forest.seeded(0)


def _forest(trees):
    """a forest object holding `trees` (set_forests reads tree_pos and the mountain constants)"""
    f = copy.copy(_template())
    f.tree_pos = np.array(trees, dtype=float).reshape(-1, 3)
    f.num_trees = f.tree_pos.shape[0]
    return f


def _engine(mode, n, cases, scenario_forest=None):
    from distributed_aerial_transportation_amd import BatchedController

    B = len(cases)
    eng = BatchedController(mode, n, B, es.params(n))
    eng.set_forests([_forest(c.trees) for c in cases],
                    np.arange(B, dtype=np.int32) if scenario_forest is None else scenario_forest)
    eng.set_state(np.stack([c.state for c in cases]), np.zeros(B, dtype=np.int32))
    return eng


# ---- a. k_env against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", es.NS)
@pytest.mark.parametrize("mode", ["cadmm", "dd", "centralized"])
def test_gpu_env_rows_match_long_double_reference(mode, n):
    es.coverage()
    cases, refs = es.battery(n)
    eng = _engine(mode, n, cases)
    try:
        lhs, rhs, nr, col, md = eng.env_rows()
    finally:
        eng.close()
    worst_row = worst_dist = 0.0
    for k, (case, ref) in enumerate(zip(cases, refs)):
        for i in range(n):
            want = ref.central if mode == "centralized" else ref.agents[i]
            dr, dm = er.same_rows(want, lhs[k, i, :nr[k, i]], rhs[k, i, :nr[k, i]], col[k, i], md[k, i],
                                  f"{mode} n = {n} {case.name} agent {i}")
            assert not np.any(lhs[k, i, nr[k, i]:]) and not np.any(rhs[k, i, nr[k, i]:])
            worst_row, worst_dist = max(worst_row, dr), max(worst_dist, dm)
    print(f"{mode} n = {n}: worst row entry {worst_row:.2e}, worst min_env_dist {worst_dist:.2e}")


# ---- b. k_env_class against k_env ---------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _expected_class(lhs, rhs, nr):
    """env class per scenario from the compacted rows (B, n, 10, .): the smallest class whose capacity holds the
    largest nonzero-row count among the agents, at least 1 if any kept row is all-zero with rhs > 0"""
    kept = np.arange(lhs.shape[2])[None, None, :] < nr[:, :, None]
    nonzero = kept & np.any(lhs != 0.0, axis=3)
    need = np.any(nonzero | (kept & (rhs > 0.0)), axis=(1, 2))
    most = np.max(np.sum(nonzero, axis=2), axis=1)
    cls = np.array([next(c for c in (1, 2, 3) if m <= CLASS_ROWS[c]) for m in most])
    return np.where(need, cls, 0)


def _same_image(got, exp, what):
    glhs, grhs, gnr, gcls = got
    lhs, rhs, nr, col, md = exp
    assert np.array_equal(gnr, nr), (what, np.argwhere(gnr != nr))
    assert np.array_equal(_bits(glhs), _bits(lhs)), (what, np.argwhere(_bits(glhs) != _bits(lhs))[:5])
    assert np.array_equal(_bits(grhs), _bits(rhs)), (what, np.argwhere(_bits(grhs) != _bits(rhs))[:5])
    assert np.array_equal(gcls, _expected_class(lhs, rhs, nr)), (what, gcls, _expected_class(lhs, rhs, nr))


@pytest.mark.parametrize("n", es.NS)
def test_gpu_env_class_rows_are_env_rows_bitwise(n):
    """23 scenes (no multiple of 64 // n = 21, 16, 10, 5, 4 nor of 2 or 3), one forest each: windows of 0 trees (the
    empty forest stands between two others), 1, n, 2 n + 1 and up to 60 trees share workgroups; one scenario has no
    forest (scenario_forest = -1).  The trees are handed over unsorted."""
    cases, _ = es.battery(n)
    cases = cases[:23]
    B = len(cases)
    assert B % (64 // n) and B % 2 and B % 3
    names = [c.name for c in cases]
    assert 0 < names.index("empty") < B - 1 and all(cases[names.index("empty") + d].trees.size for d in (-1, 1))
    assert any(np.any(np.diff(c.trees[:, 0]) < 0) for c in cases)
    sf = np.arange(B, dtype=np.int32)
    bare = names.index("random1")
    sf[bare] = -1
    states = np.stack([c.state for c in cases])
    acc = np.random.default_rng(n).uniform(-1, 1, (B, 6))
    for sub in (1, 2, 3):
        eng = _engine("cadmm", n, cases, sf)
        try:
            eng.set_max_iter(2)
            eng.set_sub_batches(sub)
            exp = eng.env_rows()
            r = eng.control(states, acc)
            _same_image(eng.debug_env_class(), exp, f"n = {n}, control, {sub} sub-batches")
            eng.log_begin([0], hl_capacity=1, summary=True)
            eng.closed_loop(1)
            _same_image(eng.debug_env_class(), exp, f"n = {n}, closed_loop(1), {sub} sub-batches")
            log = eng.log_read()
            eng.log_end()
        finally:
            eng.close()
        lhs, rhs, nr, col, md = exp
        assert nr[bare].max() == 0 and nr.max() == 10 and len({int(k) for k in nr.reshape(-1)}) >= 6
        for what, c, m in (("control", r.collision, r.min_env_dist),
                           ("closed_loop", log["sum_collision"][0], log["sum_min_env_dist"][0])):
            assert np.array_equal(c, np.any(col, axis=1)), (what, sub)
            assert np.array_equal(_bits(m), _bits(np.min(md, axis=1))), (what, sub)


# ---- c. the gated variants ----------------------------------------------------------------------------------------
GN, GB, GK = 6, 12, 3
SCHEDULES = {"plain": (False, False), "overlap": (True, False), "pipeline": (True, True)}


@functools.lru_cache(maxsize=None)
def _gated_inputs():
    from distributed_aerial_transportation_amd import Forest
    from tests.test_gpu_c4 import near_tree_states
    from tests.test_gpu_tail_team_sizes import _with_arc

    plain = [Forest.seeded(s) for s in range(4)]
    x0 = np.stack([near_tree_states(GN, plain, [b % 4], np.random.default_rng(600 + b), d_axis=(1.4, 2.0))[0]
                   for b in range(GB)])
    return [_with_arc(plain[b % 4], x0[b], GN) if b % 2 else plain[b % 4] for b in range(GB)], x0


def _gated_engine(schedule):
    from distributed_aerial_transportation_amd import BatchedController

    forests, x0 = _gated_inputs()
    eng = BatchedController("cadmm", GN, GB, es.params(GN))
    eng.set_forests(forests, np.arange(GB, dtype=np.int32))
    eng.set_state(x0, np.zeros(GB, dtype=np.int32))
    overlap, pipeline = SCHEDULES[schedule]
    eng.set_advance_overlap(overlap)
    eng.set_step_pipeline(pipeline)
    if overlap:  # both gated passes take scenarios, whatever the timing
        eng.debug_advance_split(np.arange(GB) % 2 == 0)
    return eng


@functools.lru_cache(maxsize=None)
def _gated_expected():
    """k_env's rows on the state after GK - 1 periods (the plain schedule; the three end bitwise equal:
    test_gpu_step_pipeline.py)"""
    eng = _gated_engine("plain")
    try:
        eng.closed_loop(GK - 1)
        out = eng.env_rows()
    finally:
        eng.close()
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_gpu_env_class_rows_in_the_closed_loop_schedules(schedule):
    exp = _gated_expected()
    assert exp[2].max() == 10 and exp[2].min() == 0  # the arcs fill the 10 slots of some agent
    eng = _gated_engine(schedule)
    try:
        eng.closed_loop(GK)
        got = eng.debug_env_class()
        early, late = eng.advance_counts()
    finally:
        eng.close()
    if schedule != "plain":
        assert early == GK * (GB // 2) and late == GK * (GB - GB // 2)
    _same_image(got, exp, schedule)
