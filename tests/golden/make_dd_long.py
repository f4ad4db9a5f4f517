"""Fixture ref_dd_long.npz: DD control steps whose dual ascent runs long -- past pass DD_WARM_PASS (dat_dd_step.hpp),
from which k_dd starts every agent QP from the previous pass's iterate, up to the stall at max_iter (101 passes) --
answered by the oracle (oracle/controllers.py DD, cold at every pass, IPM tolerance 1e-11).  Read by
tests/_dd_long.py for tests/test_hostsim.py and tests/test_gpu_dd_long.py.

Cases (CASES below): n = 3 (k_dd's register path, G = 21 slots per workgroup), n = 8 (two columns per lane, G = 8),
n = 9 (the smallest team of the LDS path, G = 7), each without a forest (k_dd<false>) from
scenarios.perturbed_states and accelerations uniform in +-s, where the force bounds become active and the chains
long; and f3: n = 3 in the `crowd` trees of tests/_envscenes.battery(3) (k_dd<true>, env rows on the agents' QPs), the
battery's states, accelerations uniform in +-6.  Every scenario runs two consecutive control steps (lambda_F, lambda_M
and prev carried); the second step's acceleration is the one of another scenario of the pool.

Selection: from a seeded pool of POOL scenarios the host build of the step rules (tests/hostsim hs_dd_step, fast)
names the pass counts, and a batch of G + 2 scenarios is picked that holds stalled steps, steps of 31-100 passes and
short steps, two scenarios that stall in both steps and one whose short first step is followed by a long one
(test_gpu_dd_long.py's refill test).  The host's counts only choose which scenarios are recorded: the regime counts
and the exclusion cap (tests/_dd_long.py check_cap) are then asserted on the oracle's own results, and another seed
is tried if they do not hold.  The oracle runs twice, at 1e-11 and at 1e-10 (patched as tools/dd_sensitivity.py
patches solve_qp); the difference gives the per-step sensitivities sens_err, sens_f and count_moves.

n16: n = 16 (G = 4, B = 6) states and accelerations with long chains by the host step, for the GPU grouping test
alone (no oracle run: 16 agents x 100 passes of the dense oracle IPM per step).

    python tests/golden/make_dd_long.py [case ...]       (all cases: ~9 CPU-minutes, 1.5 minutes on 8 cores)
"""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "ref_dd_long.npz")

# case: (n, acceleration scale s, forest)
CASES = {"n3": (3, 10.0, False), "n8": (8, 15.0, False), "n9": (9, 15.0, False), "f3": (3, 6.0, True)}
N16 = (16, 25.0, 6)  # n, s, B
POOL = 40
WANT = 4  # scenario-steps of each regime the selection aims at (3 are asserted on the oracle's counts)


def _crowd():
    from tests import _envscenes as es

    cases = es.battery(3)[0]
    return cases, np.array(next(c for c in cases if c.name == "crowd").trees)


def pool(n, s, forest, attempt):
    """(states (POOL, S), acc (POOL, 2, 6), trees or None), seeded"""
    from distributed_aerial_transportation_amd import scenarios

    rng = np.random.default_rng(7 * n + int(s) + 1000 * attempt)
    trees = None
    if forest:
        cases, trees = _crowd()
        states = np.stack([cases[p % len(cases)].state for p in range(POOL)])
    else:
        states = scenarios.perturbed_states(n, POOL, rng)
    a = rng.uniform(-s, s, (POOL, 6))
    return states, np.stack([a, a[::-1]], axis=1), trees


def host_steps(n, states, acc, trees):
    """the host step on every scenario: [(DDStep, DDStep)]"""
    from distributed_aerial_transportation_amd import scenarios
    from tests import hostsim as hs

    prm = scenarios.params_block(n)
    out = []
    for x, a in zip(states, acc):
        warm = hs.dd_warm(prm, n)
        out.append(tuple(hs.dd_step(prm, n, x, a[k], warm, trees) for k in range(2)))
    return out


def select(it, B):
    """B pool indices from the host's pass counts it (POOL, 2), in pool order"""
    from tests._dd_long import MAX_ITER, warm_pass

    wp = warm_pass()
    stall, mid, short = it > MAX_ITER, (it > wp) & (it <= MAX_ITER), it < wp
    chosen = []

    def take(mask, count):
        for p in np.nonzero(mask)[0]:
            if count <= 0:
                break
            if p not in chosen:
                chosen.append(int(p))
                count -= 1
        return count

    assert take(stall[:, 0] & stall[:, 1], 2) == 0, "no two scenarios stall in both steps"
    assert take(short[:, 0] & ~short[:, 1] & (it[:, 1] > wp), 1) == 0, "no short step followed by a long one"
    for m in (mid, short, stall):
        have = int(m[chosen].sum())
        take(m.any(axis=1), max(0, (WANT - have + 1) // 2))
    take(np.ones(len(it), dtype=bool), B - len(chosen))
    assert len(chosen) == B, (len(chosen), B)
    return sorted(chosen)


def _oracle_job(job):
    """one scenario's two steps by the oracle at IPM tolerance tol: (iters (2), f_des (2, 3, n), err (2, MAX_ITER))"""
    n, x, acc, trees, tol = job
    import oracle.controllers as oc
    import oracle.ipm as oi
    from distributed_aerial_transportation_amd.system import RQPState
    from oracle import forest as of
    from oracle import model as om
    from oracle import scenarios as osc
    from tests._dd_long import MAX_ITER

    forest = None
    if trees is not None:
        forest = of.Forest.__new__(of.Forest)
        forest.tree_pos, forest.num_trees = np.array(trees), len(trees)
    orig = oi.solve_qp
    oc.solve_qp = lambda *a, **k: orig(*a, **{**k, "tol": tol})
    try:
        s = RQPState.unpack(x, n)
        st = om.State(s.R, s.w, s.xl, s.vl, s.Rl, s.wl, project=False)
        ctl = oc.DD(osc.params(n), osc.col_radius(n), forest)
        it, f, err = np.zeros(2, dtype=np.int16), np.zeros((2, 3, n)), np.full((2, MAX_ITER), np.nan)
        for k in range(2):
            f[k], stat = ctl.control(st, (acc[k, :3], acc[k, 3:]))
            it[k] = stat.iter
            err[k, : stat.iter - 1] = stat.err_seq
    finally:
        oc.solve_qp = orig
    return it, f, err


def make_case(name, workers):
    from tests import _dd_long as dl

    n, s, forest = CASES[name]
    B = 64 // n + 2
    for attempt in range(6):
        states, acc, trees = pool(n, s, forest, attempt)
        host = host_steps(n, states, acc, trees)
        try:
            idx = select(np.array([[h.iters for h in hh] for hh in host]), B)
        except AssertionError as e:
            print(f"{name}: attempt {attempt}: selection: {e}", flush=True)
            continue
        jobs = [(n, states[p], acc[p], trees, tol) for tol in (1e-11, 1e-10) for p in idx]
        res = workers.map(_oracle_job, jobs)
        r11, r10 = res[:B], res[B:]
        d = {"state": states[idx], "acc": acc[idx], "scale": np.float64(s), "attempt": np.int64(attempt),
             "iters": np.stack([r[0] for r in r11]), "f_des": np.stack([r[1] for r in r11]),
             "err": np.stack([r[2] for r in r11]), "iters_1e10": np.stack([r[0] for r in r10]),
             "f_des_1e10": np.stack([r[1] for r in r10]), "err_1e10": np.stack([r[2] for r in r10])}
        d["sens_err"], d["sens_f"], d["count_moves"] = dl.sensitivities(d["iters"], d["f_des"], d["err"],
                                                                        d["iters_1e10"], d["f_des_1e10"], d["err_1e10"])
        if forest:
            d["trees"] = trees
        c = dl.Case({f"{name}_{k}": v for k, v in d.items()}, name)
        # the regimes and the exclusion cap, on the oracle's results alone
        reg = dl.regimes(c.iters)
        try:
            assert min(reg) >= 3, f"regimes (stalled, 31-100, short) {reg}"
            two = np.sum(np.all(c.iters > dl.MAX_ITER, axis=1))
            assert two >= 2, f"{two} scenarios stall in both steps"
            wp = dl.warm_pass()
            assert np.any((c.iters[:, 0] < wp) & (c.iters[:, 1] > wp)), "no short step followed by a long one"
            ex = dl.check_cap(c)
        except AssertionError as e:
            print(f"{name}: attempt {attempt}: {e}", flush=True)
            continue
        print(f"{name}: attempt {attempt}, B = {B}: (stalled, 31-100, short) steps {reg}, excluded {int(ex.sum())} of "
              f"{ex.size}; sens_err max {np.nanmax(c.sens_err):.3g} median {np.nanmedian(c.sens_err):.3g}, sens_f max "
              f"{np.nanmax(c.sens_f):.3g}, count moves {int(c.count_moves.sum())}", flush=True)
        # the host step against the oracle: reported, never a reason to pick other scenarios
        worst, failed = dl.Worst(), []
        for j, p in enumerate(idx):
            for k in range(2):
                if ex[j, k]:
                    continue
                h = host[p][k]
                try:
                    dl.compare(c, j, k, h.iters, h.f_des, h.err_seq, worst)
                except AssertionError as e:
                    failed.append(str(e))
        print(f"{name}: host step against the oracle: {worst}; {len(failed)} outside the rules", flush=True)
        for f in failed:
            print("   ", f, flush=True)
        return d
    raise SystemExit(f"{name}: no seed met the regime counts and the exclusion cap")


def make_n16():
    n, s, B = N16
    from tests._dd_long import warm_pass

    for attempt in range(6):
        states, acc, _ = pool(n, s, False, attempt)
        it = np.array([[h.iters for h in hh] for hh in host_steps(n, states, acc, None)])
        longest = np.argsort(-it.max(axis=1), kind="stable")[: B // 2]
        idx = sorted(set(longest.tolist()) | set(np.nonzero(it.max(axis=1) < warm_pass())[0][: B - B // 2].tolist()))
        if len(idx) == B and np.sum(it[idx] > warm_pass()) >= 3:
            print(f"n16: attempt {attempt}: host pass counts {it[idx].tolist()}", flush=True)
            return {"state": states[idx], "acc": acc[idx], "host_iters": it[idx].astype(np.int16)}
    raise SystemExit("n16: no long chains")


def main():
    names = sys.argv[1:] or list(CASES) + ["n16"]
    old = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    with mp.Pool(min(8, os.cpu_count() or 1)) as workers:
        for name in names:
            d = make_n16() if name == "n16" else make_case(name, workers)
            old = {k: v for k, v in old.items() if not k.startswith(name + "_")}
            old.update({f"{name}_{k}": v for k, v in d.items()})
    np.savez_compressed(OUT, **old)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
