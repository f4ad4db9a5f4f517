"""k_dd on long dual-ascent chains (tests/golden/make_dd_long.py, ref_dd_long.npz): steps that stop before pass
DD_WARM_PASS (dat_dd_step.hpp), steps of 31-100 passes and steps stalled at max_iter (101), two consecutive control
steps per scenario, batches of G + 2 scenarios (G = floor(64 / n) slots per workgroup) -- the passes from which
k_dd starts every agent QP from the previous pass's iterate (wson, the HBM warm record), which no other DD test
reaches.  n = 3 (register path), n = 8 (two columns per lane), n = 9 (LDS path) without a forest (k_dd<false>), n = 3
in the `crowd` trees (k_dd<true>), and for the grouping test n = 16 (G = 4, B = 6).

1. against the oracle's cold solves, under the fixture's per-step bounds (tests/_dd_long.py);
2. against the host build of the same step rules, at ERR_RTOL / ERR_ATOL / REL (both warm-start by one rule): where
   1 fails and 2 passes the rule is inaccurate, where 2 fails the kernel is wrong;
3. grouping, bitwise: one workgroup (refills; warm and cold slots in one wavefront), the full grid, every scenario
   alone, the batch reversed -- outputs and the warm state the step leaves (checkpoint records);
4. control_steps(K = 2) against two control calls, bitwise (the chain restarts at the step boundary);
5. a short scenario refilled into the slot of a stalled one against the same scenario alone, bitwise."""

import functools

import numpy as np
import pytest

from tests import _dd_long as dl

pytestmark = pytest.mark.gpu

OUT = ("f_des", "iters", "qp_status", "err_seq")
WARM = ("lambda_F", "lambda_M", "prev", "f_des", "iters", "ipmx")


def _eng(c, B, blocks=0, record_err=True):
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    eng = BatchedController("dd", c.n, B, scenarios.params_block(c.n), record_err=record_err)
    eng.set_persistent_blocks(blocks)
    if c.trees is not None:
        from tests.test_gpu_env_rows_reference import _forest

        eng.set_forests([_forest(c.trees)])
    return eng


def _two_steps(c, idx, blocks=0):
    """the scenarios idx of case c as one batch, two control steps: ([step 1, step 2] outputs, warm state after)"""
    idx = np.asarray(idx)
    eng = _eng(c, len(idx), blocks)
    steps = []
    for k in range(2):
        r = eng.control(c.state[idx], c.acc[idx, k])
        steps.append({"f_des": r.f_des, "iters": r.iters, "qp_status": r.qp_status, "err_seq": r.err_seq})
    warm = {k: v.copy() for k, v in eng.checkpoint().arrays().items() if k in WARM}
    assert eng.work()["inband_beyond_clarabel_tol"] == 0
    eng.close()
    return steps, warm


@functools.lru_cache(maxsize=None)
def _capped(name):
    """case `name` on one persistent workgroup (shared by the tests; nobody writes to it)"""
    c = dl.case(name)
    return c, _two_steps(c, np.arange(c.B), blocks=1)


@functools.lru_cache(maxsize=None)
def _host(name):
    """the host step on every scenario of the case: [(DDStep, DDStep)]"""
    from distributed_aerial_transportation_amd import scenarios
    from tests import hostsim as hs

    c = dl.case(name)
    prm = scenarios.params_block(c.n)
    out = []
    for b in range(c.B):
        warm = hs.dd_warm(prm, c.n)
        out.append(tuple(hs.dd_step(prm, c.n, c.state[b], c.acc[b, k], warm, c.trees) for k in range(2)))
    return out


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (what, k)


def _n16():
    from tests._golden import load

    d = load("ref_dd_long.npz")

    class C:
        name, n, trees = "n16", 16, None
        state, acc = d["n16_state"], d["n16_acc"]
        B, G = d["n16_state"].shape[0], 4
    return C


@pytest.mark.parametrize("name", dl.CASES)
def test_gpu_dd_long_chains_match_oracle(name):
    """One workgroup drains the G + 2 scenarios (two refills), both steps, err_seq recorded: pass counts exact,
    f_des within max(REL, 5 x sens_f), err_seq within max(ERR_RTOL, 3 x sens_err) / ERR_ATOL of the oracle at every
    scenario-step the fixture does not exclude (check_cap bounds those), every QP OPTIMAL, no accept beyond Clarabel's
    tolerance, and the run held steps on both sides of DD_WARM_PASS.  Measured on an MI355X: see DESIGN.md
    "Long DD chains"."""
    c, (steps, _) = _capped(name)
    ex = dl.check_cap(c)
    wp = dl.warm_pass()
    its = np.stack([s["iters"] for s in steps], axis=1)
    assert np.sum(its > wp) >= 3 and np.sum(its < wp) >= 3 and np.sum(its > dl.MAX_ITER) >= 2, its.tolist()
    worst = dl.Worst()
    for b in range(c.B):
        for k in range(2):
            if ex[b, k]:
                break
            s = steps[k]
            assert np.all(s["qp_status"][b] == 0), (b, k, s["qp_status"][b])
            dl.compare(c, b, k, s["iters"][b], s["f_des"][b], s["err_seq"][b], worst)
    print(f"{name}: k_dd against the oracle, {int((~ex).sum())} scenario-steps: {worst}")


@pytest.mark.parametrize("name", dl.CASES)
def test_gpu_dd_long_chains_match_host_step(name):
    """The same run against the host build of the step rules (hs_dd_step: the long-chain rule and the warm start by
    dd_long_chain / dd_warm_start, as k_dd), every scenario-step, none excluded: pass counts and statuses exact,
    f_des within REL, err_seq within ERR_RTOL / ERR_ATOL (the host fuses no multiply-adds: not bitwise)."""
    c, (steps, _) = _capped(name)
    worst = dl.Worst()
    for b, hh in enumerate(_host(name)):
        for k, h in enumerate(hh):
            s = steps[k]
            assert np.array_equal(s["qp_status"][b], h.qp_status), (b, k)
            dl.compare(c, b, k, s["iters"][b], s["f_des"][b], s["err_seq"][b], worst, tight=True,
                       ref=(h.iters, h.f_des, h.err_seq))
    print(f"{name}: k_dd against the host step, {2 * c.B} scenario-steps: {worst}")


@pytest.mark.parametrize("name", dl.NOFOREST + ("f3", "n16"))
def test_gpu_dd_long_chains_grouping_bitwise(name):
    """A scenario's arithmetic does not depend on what shares its wavefront, in the warm passes either: the batch on
    one workgroup (the last two scenarios of the sorted queue refill freed slots, and slots past pass DD_WARM_PASS sit
    beside cold ones), on the full grid, every scenario alone on a B = 1 handle, and the batch reversed give f_des,
    iters, qp_status and err_seq (NaN by position) equal to the bit at both steps, and leave the same warm state
    (lambda_F, lambda_M, prev, iters, ipmx of the checkpoint records)."""
    if name == "n16":
        c = _n16()
        base = _two_steps(c, np.arange(c.B), blocks=1)
    else:
        c, base = _capped(name)
    wp = dl.warm_pass()
    its = np.stack([s["iters"] for s in base[0]], axis=1)
    assert np.any(its > wp) and np.any(its < wp), its.tolist()
    full = _two_steps(c, np.arange(c.B))
    rev = _two_steps(c, np.arange(c.B)[::-1], blocks=1)
    for k in range(2):
        _same(base[0][k], full[0][k], ("full grid", k))
        _same(base[0][k], {key: v[::-1] for key, v in rev[0][k].items()}, ("reversed", k))
    _same(base[1], full[1], "full grid, warm state")
    _same(base[1], {key: v[::-1] for key, v in rev[1].items()}, "reversed, warm state")
    for b in range(c.B):
        steps, warm = _two_steps(c, [b])
        for k in range(2):
            _same({key: v[b: b + 1] for key, v in base[0][k].items()}, steps[k], ("alone", b, k))
        _same({key: v[b: b + 1] for key, v in base[1].items()}, warm, ("alone, warm state", b))


@pytest.mark.parametrize("name", ["n3", "n9"])
def test_gpu_dd_long_chains_fused_steps(name):
    """dat_control_steps with K = 2 on chains that cross DD_WARM_PASS in the first step and restart in the second
    (the warm record's flag and the long-chain flag reset at the step boundary, in the slot): f_des, iters, qp_status
    and the warm state equal two dat_control_step calls to the bit, on one workgroup and on the full grid."""
    c = dl.case(name)
    assert np.sum(np.any(c.iters > dl.warm_pass(), axis=1)) >= 3
    for blocks in (1, 0):
        sep = _eng(c, c.B, blocks, record_err=False)
        sep.set_state(c.state)
        r1 = sep.control(None, c.acc[:, 0])
        r2 = sep.control(None, c.acc[:, 1])
        assert np.any(r1.iters > dl.warm_pass())
        fus = _eng(c, c.B, blocks, record_err=False)
        fus.set_state(c.state)
        rf = fus.control_steps(np.ascontiguousarray(c.acc.transpose(1, 0, 2)))
        for key in ("f_des", "iters", "qp_status"):
            assert np.array_equal(getattr(rf, key), getattr(r2, key)), (blocks, key)
        ws, wf = sep.checkpoint().arrays(), fus.checkpoint().arrays()
        _same({k: ws[k] for k in WARM}, {k: wf[k] for k in WARM}, ("warm state", blocks))
        sep.close()
        fus.close()


@pytest.mark.parametrize("name", dl.NOFOREST)
def test_gpu_dd_refill_after_stall_leaves_no_trace(name):
    """A slot a 101-pass scenario frees is refilled without a trace of it.  The batch is G scenarios that stall in
    both steps (copies of the fixture's, alternating) followed by one whose first step is short, on one workgroup.
    The second step's queue is sorted by the first step's pass counts, longest first (k_dd_key): the G stalled
    scenarios take the G slots, run 101 passes (70 of them warm) and free them in the same pass, and the short-first
    scenario, last in the queue, takes one of those slots -- it runs its own second step, past DD_WARM_PASS, there.
    Both of its steps equal the same scenario alone on a B = 1 handle, to the bit, and so does its warm state."""
    c = dl.case(name)
    wp = dl.warm_pass()
    both = np.nonzero(np.all(c.iters > dl.MAX_ITER, axis=1))[0]
    late = np.nonzero((c.iters[:, 0] < wp) & (c.iters[:, 1] > wp))[0]
    assert both.size >= 2 and late.size >= 1, (both, late)
    idx = [int(both[j % 2]) for j in range(c.G)] + [int(late[0])]
    steps, warm = _two_steps(c, idx, blocks=1)
    assert np.all(steps[0]["iters"][: c.G] > dl.MAX_ITER) and np.all(steps[1]["iters"][: c.G] > dl.MAX_ITER)
    assert steps[0]["iters"][c.G] < wp < steps[1]["iters"][c.G], steps[1]["iters"][c.G]
    alone, awarm = _two_steps(c, [idx[-1]])
    for k in range(2):
        _same({key: v[c.G:] for key, v in steps[k].items()}, alone[k], ("refilled", k))
    _same({key: v[c.G:] for key, v in warm.items()}, awarm, "refilled, warm state")
    # (and the copies of one stalled scenario agree among themselves, whichever slot ran them)
    for k in range(2):
        for key, v in steps[k].items():
            assert np.array_equal(v[0], v[2], equal_nan=v.dtype.kind == "f"), (k, key)
