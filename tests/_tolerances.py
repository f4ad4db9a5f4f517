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
# Long DD chains (ref_dd_long.npz, tests/_dd_long.py): the bounds are per scenario-step, from the oracle's own change
# between IPM tolerances 1e-11 and 1e-10 stored with the fixture: err_seq within max(ERR_RTOL, 3 x sens_err) relative
# OR ERR_ATOL absolute (the 3x of DD_ERR_RTOL), f_des within max(REL, 5 x sens_f) (test_gpu_hard_stretch.py's rule).
# Measured by tests/golden/make_dd_long.py, cases n3 / n8 / n9 / f3 (n = 3 in a forest), 46 / 20 / 18 / 46
# scenario-steps: sens_err maxima 1.0e-3 / 1.8e-2 / 1.1e-3 / 9.5e-4 (medians 5.1e-7 / 2.4e-5 / 1.3e-6 / 3.9e-8), sens_f
# maxima 3.9e-6 / 6.7e-7 / 3.0e-6 / 7.4e-8; the oracle's pass count moved at no step and no residual lies in the
# band, so nothing is excluded.  Worst err_seq differences from the oracle (relative, where beyond ERR_ATOL; the
# largest sit on the steps with the largest sens_err), host step: passes < 30 5.3e-4 / 1.8e-4 / 8.9e-5 / 3.9e-4,
# passes >= 30 1.2e-4 / 2.8e-3 / 1.4e-4 / 3.3e-5; k_dd on an MI355X the same figures (f3, passes >= 30: 6.6e-5).
# k_dd against the host step: 1.8e-6 below pass 30, 9.1e-6 from it on (f3: 2.2e-5, 6.5e-5).  Before the long-chain
# rule (dat_dd_step.hpp) the first warm pass was 4.5e-4 off at n = 8 and 1.6e-4 at n = 3 where the bound is 1e-4.
DD_LONG_MARGIN, DD_LONG_F_MARGIN = 3.0, 5.0
# The simulation step against the long-double reference (tests/_simref.py; test_sim_reference.py,
# test_gpu_sim_reference.py).  The bars are the project's own for these quantities, none is new: every entry of a
# rolled-out state within 1e-12 absolute and the rotation counters equal (test_gpu_rollout_matches_oracle,
# test_rollout_matches_oracle_dynamics),
# thrust rtol 1e-12 / atol 1e-12 and moments rtol 1e-10 / atol 1e-12 (test_gpu_low_level_controller_golden).  What makes
# them meaningful is SIM_ORACLE_FRACTION: oracle/model.py, an independent float64 statement of the same operations, has
# to sit within a tenth of each bar of the reference on every case the kernels are held to (test_sim_reference.py), so
# a kernel beyond a bar is ten times further from the truth than double rounding explains.
SIM_STATE_ATOL = 1e-12
SIM_THRUST_RTOL, SIM_THRUST_ATOL = 1e-12, 1e-12
SIM_MOMENT_RTOL, SIM_MOMENT_ATOL = 1e-10, 1e-12
SIM_ORACLE_FRACTION = 0.1
# Measured, largest absolute difference from the reference over the cases of tests/_simref.py ("pd" / "sm").
#   first-step law, thrust and moment:  oracle 5.3e-16, 6.0e-17 / 5.3e-16, 1.9e-16;  host build 6.2e-16, 6.0e-17 /
#     6.2e-16, 6.5e-16;  k_low_level on an MI355X 5.3e-16, 6.0e-17 / 5.3e-16, 5.5e-16;  the logging rollout's 20
#     recorded steps under "sm" 4.4e-16, 1.0e-16.  At rest all three give M = 0 and f = fz exactly.
#   state after 45 steps:  oracle 1.6e-15 / 9.2e-15;  host build 1.1e-15 / 1.1e-14;  k_rollout_agents on an MI355X
#     1.2e-15 / 4.0e-15;  rigid payload (no attitude law): host build and k_rp_rollout 2.6e-15 both.
#   the reference against the reference project's own fixtures: thrust 4.2e-16, moment 5.0e-17 / 1.2e-16, 45 steps
#     of ref_dynamics.npz 4.8e-4 of their bar, 2000 steps of ref_rp.npz 1.0e-14.
#   the reference's polar factors, every matrix it projected: |U'U - I| <= 2.2e-19, |U'X - (U'X)'| <= 1.9e-19.
# The one case that came beyond the tenth (oracle 3.0e-13, host build 8.6e-13: the "sm" law chattering about its
# sliding surface) and why it is not among the cases: test_sim_reference.py.


def _ambiguous(seq, tol=1e-2, band=1e-7):
    """The reference stops when err < tol; a residual within `band` (relative) of tol can flip the count
    (such scenarios are excluded from exact-count checks, and tests assert they are rare)."""
    return any(abs(e - tol) < band * tol for e in seq)
