"""The long DD chains of ref_dd_long.npz (tests/golden/make_dd_long.py) and the rules every comparison against the
fixture's oracle results follows: the generator (oracle alone), the host step (test_hostsim.py) and the GPU
(test_gpu_dd_long.py) state them here once.

A case is one batch of G + 2 scenarios (G = floor(64 / n) slots of a k_dd workgroup), two consecutive control steps
each (lambda_F, lambda_M and prev carried), recorded from the oracle at IPM tolerance 1e-11 (its default) and 1e-10.
A scenario-step is addressed as [b, k]: scenario b, step k in {0, 1}."""
import os
import re

import numpy as np

from tests._golden import load
from tests._tolerances import DD_LONG_F_MARGIN, DD_LONG_MARGIN, ERR_ATOL, ERR_RTOL, REL, _ambiguous

CASES = ("n3", "n8", "n9", "f3")  # f3: n = 3 in the `crowd` trees of tests/_envscenes.battery(3) (k_dd<true>)
NOFOREST = ("n3", "n8", "n9")
MAX_ITER, RES_TOL = 100, 1e-2  # the controller's defaults (control/rqp_dd.py), the fixture's


def warm_pass():
    """DD_WARM_PASS as dat_dd_step.hpp defines it"""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(os.path.dirname(here), "distributed_aerial_transportation_amd", "csrc",
                            "dat_dd_step.hpp")).read()
    m = re.search(r"constexpr int DD_WARM_PASS = (\d+);", src)
    assert m and "DAT_HD bool dd_warm_pass(int iter) { return iter >= DD_WARM_PASS; }" in src
    return int(m.group(1))


class Case:
    """one case of the fixture: state (B, S), acc (B, 2, 6), and of the oracle at 1e-11 iters (B, 2), f_des
    (B, 2, 3, n), err (B, 2, MAX_ITER) NaN-padded; the same at 1e-10 (*_1e10); the derived tables sens_err, sens_f
    (B, 2) and count_moves (B, 2); trees (T, 3) or None"""

    def __init__(self, d, name):
        self.name = name
        for k in ("state", "acc", "iters", "f_des", "err", "iters_1e10", "f_des_1e10", "err_1e10", "sens_err",
                  "sens_f", "count_moves"):
            setattr(self, k, d[f"{name}_{k}"])
        self.trees = d[f"{name}_trees"] if f"{name}_trees" in d else None
        self.n = self.f_des.shape[3]
        self.B = self.state.shape[0]
        self.G = 64 // self.n
        self.iters = self.iters.astype(int)

    def err_seq(self, b, k):
        return self.err[b, k, : self.iters[b, k] - 1]


def case(name):
    return Case(load("ref_dd_long.npz"), name)


def sensitivities(iters, f_des, err, iters10, f_des10, err10):
    """The oracle against itself, 1e-10 against 1e-11, per scenario-step: (sens_err, sens_f, count_moves).  sens_err
    is the largest relative err_seq change over the step's passes, sens_f the largest f_des change relative to the
    step's largest force component; both NaN where the pass count itself moves (count_moves), and from then on in
    that scenario (its second step starts from another warm state)."""
    B = iters.shape[0]
    se, sf, cm = np.full((B, 2), np.nan), np.full((B, 2), np.nan), np.zeros((B, 2), dtype=bool)
    for b in range(B):
        for k in range(2):
            if iters[b, k] != iters10[b, k]:
                cm[b, k:] = True
                break
            m = iters[b, k] - 1
            a, c = err[b, k, :m], err10[b, k, :m]
            se[b, k] = float(np.max(np.abs(c / a - 1.0))) if m else 0.0
            sf[b, k] = float(np.max(np.abs(f_des10[b, k] - f_des[b, k])) / max(1.0, np.max(np.abs(f_des[b, k]))))
    return se, sf, cm


def err_rtol(c, b, k):
    """err_seq: max(ERR_RTOL, DD_LONG_MARGIN x the oracle's own sensitivity) of the scenario-step"""
    return max(ERR_RTOL, DD_LONG_MARGIN * c.sens_err[b, k])


def f_bound(c, b, k):
    """f_des: max(REL, DD_LONG_F_MARGIN x the oracle's own sensitivity), test_gpu_hard_stretch.py's rule"""
    return max(REL, DD_LONG_F_MARGIN * c.sens_f[b, k])


def excluded(c):
    """(B, 2) bool: the scenario-steps whose pass count the oracle itself does not pin -- its count moves between
    the two tolerances, or a residual lies within the band of the stopping tolerance (1e-7, or the step's measured
    sensitivity where that made the err_seq tolerance larger) -- and the step after such a step (another warm
    state).  Decided by the fixture alone, never by the code under test."""
    ex = np.zeros((c.B, 2), dtype=bool)
    for b in range(c.B):
        for k in range(2):
            if c.count_moves[b, k]:
                ex[b, k:] = True
                break
            rtol = err_rtol(c, b, k)
            band = rtol / DD_LONG_MARGIN if rtol > ERR_RTOL else 1e-7
            if _ambiguous(c.err_seq(b, k), tol=RES_TOL, band=band):
                ex[b, k:] = True
                break
    return ex


def regimes(iters, keep=None):
    """scenario-steps (stalled at max_iter, of DD_WARM_PASS + 1 .. MAX_ITER passes, below DD_WARM_PASS) among `keep`"""
    it = iters if keep is None else iters[keep]
    wp = warm_pass()
    return int(np.sum(it > MAX_ITER)), int(np.sum((it > wp) & (it <= MAX_ITER))), int(np.sum(it < wp))


def check_cap(c):
    """Exclusions may not hide the warm path: at most 1 scenario-step in 8, and 2 stalled and 2 of 31-100 passes
    remain.  Returns the exclusion mask."""
    ex = excluded(c)
    assert 8 * int(ex.sum()) <= ex.size, (c.name, int(ex.sum()), ex.size)
    stalled, mid, _ = regimes(c.iters, ~ex)
    assert stalled >= 2 and mid >= 2, (c.name, stalled, mid)
    return ex


class Worst:
    """the largest err_seq differences (relative, where beyond ERR_ATOL) seen by compare(), kept apart: cold passes,
    warm passes, steps that follow a stalled step; and the largest f_des difference"""

    def __init__(self):
        self.cold = self.warm = self.after_stall = self.f = 0.0

    def __str__(self):
        return (f"err_seq passes < {warm_pass()}: {self.cold:.2e}, passes >= {warm_pass()}: {self.warm:.2e}, steps "
                f"after a stalled step: {self.after_stall:.2e}; f_des {self.f:.2e}")


def compare(c, b, k, iters, f_des, err_seq, worst=None, tight=False, ref=None):
    """One scenario-step of the code under test against the oracle's (ref None) under the fixture's rules, or with
    tight=True under ERR_RTOL / ERR_ATOL / REL against ref = (iters, f_des, err_seq) of the host step.  The caller
    skips excluded steps.  err_seq is held to ERR_ATOL + rtol |ref|: np.testing.assert_allclose(rtol, atol), the
    form in which every DD step test applies "rtol OR ERR_ATOL" (tests/_tolerances.py)."""
    r_it, r_f, r_err = ref if ref is not None else (c.iters[b, k], c.f_des[b, k], c.err_seq(b, k))
    assert int(iters) == int(r_it), (c.name, b, k, int(iters), int(r_it))
    rtol, fb = (ERR_RTOL, REL) if tight else (err_rtol(c, b, k), f_bound(c, b, k))
    e = np.asarray(err_seq)[: r_it - 1]
    assert e.shape == r_err.shape and np.all(np.isfinite(e)), (c.name, b, k)
    diff = np.abs(e - r_err)
    rel = np.where(diff > ERR_ATOL, diff / np.abs(r_err), 0.0)
    frel = float(np.max(np.abs(f_des - r_f)) / max(1.0, float(np.max(np.abs(r_f)))))
    if worst is not None:
        wp = warm_pass()
        worst.cold = max(worst.cold, float(np.max(rel[:wp], initial=0.0)))
        worst.warm = max(worst.warm, float(np.max(rel[wp:], initial=0.0)))
        if k == 1 and c.iters[b, 0] > MAX_ITER:
            worst.after_stall = max(worst.after_stall, float(np.max(rel, initial=0.0)))
        worst.f = max(worst.f, frel)
    bad = np.nonzero(diff > ERR_ATOL + rtol * np.abs(r_err))[0]
    assert bad.size == 0, (c.name, b, k, "err_seq pass", int(bad[0]), float(rel[bad[0]]), rtol, int(r_it))
    assert frel < fb, (c.name, b, k, "f_des", frel, fb)
