"""The serial env rows (env_rows, csrc/dat_core.hpp) on the host build against the long-double reference
(tests/_envref.py) over the scene battery (tests/_envscenes.py).  No GPU needed; the device builds of the same
code run the same battery in test_gpu_env_rows_reference.py."""

import numpy as np
import pytest

from tests import _envref as er
from tests import _envscenes as es
from tests import hostsim as hs


def test_battery_reaches_the_hard_branches():
    """interior minimisers, rim and cap contacts, penetrations and truncated solves, counted on the reference"""
    got = es.coverage()
    print(got)
    for n in es.NS:
        cases, _ = es.battery(n)
        assert len({c.name for c in cases}) == len(cases) == 13 + es.RANDOM


@pytest.mark.parametrize("n", es.NS)
def test_host_env_rows_match_long_double_reference(n):
    """Every agent (alpha 1.5) and the centralized query (agent -1, alpha 2.0) of every scene: row count, collision
    flag, the rows as a set (atol 1e-9) and min_env_dist (1e-8), the project's bars for these quantities.

    Worst deviations from the reference measured over the battery (no bar is derived from them):
      host build (x86-64, -O2):                 row entry 4.1e-14, min_env_dist 1.3e-15
      device, k_env (gfx950, -ffp-contract=on): row entry 4.6e-14, min_env_dist 1.3e-15
    (test_gpu_env_rows_reference.py; k_env_class' rows are k_env's bit for bit)."""
    prm = es.params(n)
    cases, refs = es.battery(n)
    worst_row = worst_dist = 0.0
    for case, ref in zip(cases, refs):
        for agent, alpha, want in [(i, es.ALPHA_D, ref.agents[i]) for i in range(n)] + [(-1, es.ALPHA_C, ref.central)]:
            lhs, rhs, col, md = hs.env_rows(prm, n, case.state, case.trees, agent, alpha)
            dr, dm = er.same_rows(want, lhs, rhs, col, md, f"n = {n} {case.name} agent {agent}")
            worst_row, worst_dist = max(worst_row, dr), max(worst_dist, dm)
    print(f"n = {n}: worst row entry {worst_row:.2e}, worst min_env_dist {worst_dist:.2e}")
