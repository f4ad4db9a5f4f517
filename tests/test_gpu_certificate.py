"""The Farkas certificate of infeasible dvl rows (dvl_rows_infeasible, csrc/dat_qp.hpp) on the GPU, through the raw
agent-QP entry that takes the caller's env rows (dat_solve_agent_qp_rows_batch, k_agent_qp): the row sets of
tests/_rowsets.py (an infeasible core -- antiparallel pair, coplanar triple, horizontal triple, positively spanning
4-set, a core with the |vl| base row -- at margins from +1e-2 to -1, with decoy rows), classified by an LP's
Chebyshev margin t.  One launch per team size (473 items: seven full wavefronts and a partial one).  As
tests/test_certificate_host.py on the host build: no false positive at t >= 0, certified (INFEASIBLE, 0 IPM
iterations) at t <= -1e-4, the oracle's answer within 1e-5 wherever the oracle solves the QP, and there no in-band
accept beyond Clarabel's 1e-8.

The tail kernel's own call site of the certificate (k_cadmm_tail, through its LDS accessors) takes its rows from
the forest geometry and cannot be fed chosen rows without a hook in the hot path; it instantiates the same
template and is covered through it only."""

import numpy as np
import pytest

from oracle import model as om
from oracle import scenarios as osc
from oracle.ipm import OPTIMAL
from tests import _rowsets as rs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", rs.NS)
def test_gpu_certificate(n):
    from distributed_aerial_transportation_amd import BatchedController, scenarios
    from distributed_aerial_transportation_amd.system import pack_state

    fams = rs.families(n)
    cs = rs.cases(n)
    K = len(cs)
    sc = np.array([c.fam for c in cs])
    args = dict(lam=np.stack([fams[c.fam].lam for c in cs]), rho=np.ones(K),
                f_mean=np.stack([fams[c.fam].fm for c in cs]))
    ag = np.array([fams[c.fam].agent for c in cs])
    acc = np.stack([fams[c.fam].acc for c in cs])
    eng = BatchedController("cadmm", n, len(fams), scenarios.params_block(n))
    try:
        eng.set_state(np.stack([pack_state(f.state) for f in fams]), np.zeros(len(fams), dtype=np.int32))
        r = eng.solve_agent_qps(sc, ag, acc, env_lhs=[c.lhs for c in cs], env_rhs=[c.rhs for c in cs], **args)
        # the items the oracle solves, again in a launch of their own: none accepted in band beyond 1e-8
        opt = np.array([k for k, c in enumerate(cs) if c.oracle_status == OPTIMAL])
        w0 = eng.work()["inband_beyond_clarabel_tol"]
        r2 = eng.solve_agent_qps(sc[opt], ag[opt], acc[opt], env_lhs=[cs[k].lhs for k in opt],
                                 env_rhs=[cs[k].rhs for k in opt], lam=args["lam"][opt], rho=np.ones(len(opt)),
                                 f_mean=args["f_mean"][opt])
        loose = eng.work()["inband_beyond_clarabel_tol"] - w0
    finally:
        eng.close()
    x = r["x"].transpose(0, 2, 1).reshape(K, 3 * n)
    # certified items are INFEASIBLE before the first IPM iteration; without a forest query nothing collides
    assert np.all(r["status"][r["certified"]] == 2) and np.all(r["ipm_iters"][r["certified"]] == 0)
    assert not np.any(r["collision"]) and np.all(np.isposinf(r["min_env_dist"]))
    rs.check(n, r["certified"], r["status"], r["ipm_iters"], x)
    assert loose == 0
    # an item's result does not depend on the launch it is in
    assert np.array_equal(r2["x"], r["x"][opt]) and np.array_equal(r2["status"], r["status"][opt])


def test_gpu_rows_entry_matches_forest_entry():
    """dat_solve_agent_qp_rows_batch fed the rows dat_env_rows reports returns what dat_solve_agent_qp_batch
    computes from the forest itself, bitwise (same kernel, same arithmetic from the rows on); DD handles take the
    rows and certify nothing."""
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios
    from tests.test_gpu_c4 import near_tree_states

    n, B = 6, 8
    forests = [Forest.seeded(s) for s in range(2)]
    sf = np.arange(B) % 2
    rng = np.random.default_rng(5)
    x0 = near_tree_states(n, forests, sf, rng, d_axis=(1.4, 2.0))
    sc, ag = np.repeat(np.arange(B), n), np.tile(np.arange(n), B)
    K = B * n
    acc = rng.uniform(-2, 2, (K, 6))
    for mode in ("cadmm", "dd"):
        eng = BatchedController(mode, n, B, scenarios.params_block(n))
        try:
            eng.set_forests(forests, sf)
            eng.set_state(x0, np.zeros(B, dtype=np.int32))
            lhs, rhs, nr, _, _ = eng.env_rows()
            assert nr.max() >= 3
            kw = dict(c=rng.normal(0, 1, (K, 9))) if mode == "dd" else dict(
                lam=rng.normal(0, 0.5, (K, 3, n)), rho=np.ones(K),
                f_mean=om.equilibrium_forces(osc.params(n))[None] + rng.normal(0, 1, (K, 3, n)))
            a = eng.solve_agent_qps(sc, ag, acc, **kw)
            b = eng.solve_agent_qps(sc, ag, acc, env_lhs=lhs.reshape(K, 10, 3), env_rhs=rhs.reshape(K, 10),
                                    nenv=nr.reshape(K), **kw)
        finally:
            eng.close()
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["status"], b["status"])
        assert np.array_equal(a["ipm_iters"], b["ipm_iters"])
        assert np.all(a["status"] == 0) and not np.any(b["certified"])
