"""The Farkas certificate of infeasible dvl rows (dvl_rows_infeasible, csrc/dat_qp.hpp) on the host build of the
C-ADMM agent QP (hs.qp_cadmm_ex), on the row sets of tests/_rowsets.py: an infeasible core (antiparallel pair,
coplanar triple, horizontal triple, positively spanning 4-set, a core with the |vl| base row) at margins from
+1e-2 to -1 with decoy rows, classified by an LP's Chebyshev margin t.  No false positive at t >= 0, certified at
t <= -1e-4, and the oracle's answer wherever the oracle solves the QP.  The inputs hold no zero row and the base
rows are non-degenerate (|vl|, |wl| != 0), so "certified" is status INFEASIBLE with 0 IPM iterations: nothing
else ends a solve before its first iteration.  tests/test_gpu_certificate.py asserts the same on the GPU.

The tail kernel's own call site of the certificate (k_cadmm_tail, through its LDS accessors) takes its rows from
the forest geometry and cannot be fed chosen rows without a hook in the hot path; it instantiates the same
template and is covered through it only."""

import numpy as np
import pytest

from tests import _rowsets as rs
from tests import hostsim as hs


@pytest.mark.parametrize("n", rs.NS)
def test_certificate_host(n):
    from distributed_aerial_transportation_amd import scenarios
    from distributed_aerial_transportation_amd.system import pack_state

    prm = scenarios.params_block(n)
    fams = rs.families(n)
    cs = rs.cases(n)
    K = len(cs)
    status, iters, x = np.zeros(K, int), np.zeros(K, int), np.zeros((K, 3 * n))
    for k, c in enumerate(cs):
        f = fams[c.fam]
        assert np.all(np.linalg.norm(c.lhs, axis=1) > 1e-12 * np.abs(c.rhs))  # no zero row
        assert np.linalg.norm(f.state.vl) > 0 and np.linalg.norm(f.state.wl) > 0
        x[k], status[k], iters[k], _ = hs.qp_cadmm_ex(prm, n, pack_state(f.state), f.acc, c.lhs, c.rhs, f.agent,
                                                       f.lam.T.reshape(-1), f.fm.T.reshape(-1), 1.0)
    rs.check(n, (status == 2) & (iters == 0), status, iters, x)
