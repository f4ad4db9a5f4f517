"""The tolerances the step parity tests share: the GPU against the oracle (test_gpu_parity.py) and the host build of
the same step rules against the oracle (test_hostsim.py).

Per-step controls within 1e-5 relative (relative to the largest force component of the step)."""

REL = 1e-5
# Residual sequences (err_seq) are consensus errors F_i - sum_j f_j: differences of forces of order
# m_T g (17-30 N) that shrink to ~1e-2, so they inherit the agent-QP solution error amplified by that
# cancellation.  tools/dd_sensitivity.py runs the ORACLE against itself on the DD step test's
# scenarios: IPM tolerance 1e-10 vs 1e-11 moves err_seq by up to 9.6e-5 relative (1.3e-6 N
# absolute at err ~ 1e-2), 1e-12 vs 1e-11 by 1.6e-5, while an explicit H^-1 instead of cho_solve
# moves it by 2e-11.  The comparison is therefore rtol 1e-4 OR 2e-6 N absolute (1e-7 of m_T g).
ERR_RTOL, ERR_ATOL = 1e-4, 2e-6
# DD err_seq by team size where the oracle's own sensitivity is larger (tools/dd_sensitivity.py n: IPM
# tolerance 1e-11 -> 1e-10 moves the oracle's err_seq by 1.05e-2 relative at n = 4, 5.27e-4 at n = 9, 7.7e-4 at
# n = 11 and 5.7e-3 at n = 16 -- those teams' agent QPs are strongly convex only through the 1e-6
# regularisation in some directions, so the solution moves ~tol / 1e-6 -- against 4.3e-5 at n = 3,
# 9.6e-5 at n = 6 and 2.7e-5 at n = 8): 3x the measured change.
DD_ERR_RTOL = {4: 3e-2, 9: 1.6e-3, 11: 2.5e-3, 16: 1.8e-2}


def _ambiguous(seq, tol=1e-2, band=1e-7):
    """The reference stops when err < tol; a residual within `band` (relative) of tol can flip the count
    (such scenarios are excluded from exact-count checks, and tests assert they are rare)."""
    return any(abs(e - tol) < band * tol for e in seq)
