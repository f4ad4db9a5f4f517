"""Point-mass rigid-link system on the CPU: the serial forms of csrc/dat_pmrl_step.hpp (tests/pmrl_host, the
pieces a lane of k_pmrl_rollout runs) against the reference's own PMRLDynamics (ref_pmrl.npz, written by
tests/golden/make_pmrl.py), and the host-side classes and layout of pmrl.py."""

import numpy as np
import pytest

from tests import _pmrl as F
from tests import pmrl_host as ph


def _residual(s, p, f, T, acc):
    """Norm of the residual of the equations of motion in PMRLDynamics' docstring, term by term:
    robots  m_i (dvl + L_i ddq_i + Rl (hat(wl)^2 + hat(dwl)) r_i) - (f_i - m_i g e3 - T_i q_i),
    payload ml dvl - (sum T_i q_i - ml g e3),  Jl dwl + wl x Jl wl - sum r_i x (T_i Rl' q_i),
    links   q_i . ddq_i + |dq_i|^2."""
    ddq, dvl, dwl = acc
    e3, g = np.array([0.0, 0.0, 1.0]), 9.80665
    n = p.n
    res = []
    mom = np.zeros(3)
    for i in range(n):
        r, q = p.r[:, i], s.q[:, i]
        xdd = dvl + p.L[i] * ddq[:, i] + s.Rl @ (np.cross(s.wl, np.cross(s.wl, r)) + np.cross(dwl, r))
        res.append(p.m[i] * xdd - (f[:, i] - p.m[i] * g * e3 - T[i] * q))
        res.append([q @ ddq[:, i] + s.dq[:, i] @ s.dq[:, i]])
        mom += np.cross(r, T[i] * (s.Rl.T @ q))
    res.append(p.ml * dvl - (s.q @ T - p.ml * g * e3))
    res.append(p.Jl @ dwl + np.cross(s.wl, p.Jl @ s.wl) - mom)
    return float(np.linalg.norm(np.concatenate(res)))


@pytest.mark.parametrize("n", [n for n, _ in F.CASES])
def test_forward_matches_reference(n):
    """T and the accelerations of the reduced 6 x 6 solve within 1e-11 of max(1, |.|) of the reference's n x n solve
    (the two solve orders of the reference itself differ by <= 1.8e-14 on these cases); S stays well conditioned."""
    from distributed_aerial_transportation_amd import pmrl

    c = F.case(n)
    worst_cond = 0.0
    for j in range(len(c.acc_at)):
        f = c.acc_force(j)
        for b in range(c.B):
            st = pmrl.pack_pmrl_state(c.acc_state(j, b))
            F.check_acc("host", ph.forward(c.prm[b], n, st, f[b]), c, j, b)
            S, _ = ph.system(c.prm[b], n, st, f[b])
            ev = np.linalg.eigvalsh(S)
            assert ev[0] >= 1.0 - 1e-12
            worst_cond = max(worst_cond, ev[-1] / ev[0])
    print(f"n = {n}: cond S <= {worst_cond:.1f}")
    assert worst_cond < 1e3


@pytest.mark.parametrize("n", [n for n, _ in F.CASES])
def test_step_matches_reference(n):
    """pmrl_step over the 45 steps of every scenario: the stored states within 1e-10, the counters equal."""
    c = F.case(n)
    hold = c.steps // c.nf
    worst = 0.0
    for b in range(c.B):
        x, cnt = c.x0[b], int(c.c0[b])
        for k in range(c.steps):
            x, cnt = ph.steps(c.prm[b], n, x, cnt, c.f[k // hold, b], c.dt)
            if k + 1 in c.keep:
                j = c.keep.index(k + 1)
                ref, rc = c.ref_block(j)
                e = float(np.max(np.abs(x - ref[b])))
                worst = max(worst, e)
                assert e <= F.TOL_STATE, (n, b, k + 1, e)
                assert cnt == rc[b], (n, b, k + 1)
    print(f"n = {n}: max state diff {worst:.2e}")


def test_reference_recipe_400_steps():
    """The reference's own n = 3 recipe (test/system/test_pmrldynamics.py:9-49), a new force at every step."""
    from distributed_aerial_transportation_amd import pmrl

    p, s0, dt, f, every, kept = F.recipe()
    prm = pmrl.pack_pmrl_params(p)
    x, cnt = pmrl.pack_pmrl_state(s0), 0
    for k in range(f.shape[0]):
        x, cnt = ph.steps(prm, 3, x, cnt, f[k], dt)
        if (k + 1) % every == 0:
            e = float(np.max(np.abs(x - pmrl.pack_pmrl_state(kept[(k + 1) // every - 1]))))
            print(f"step {k + 1}: state diff {e:.2e}")
            assert e <= F.TOL_STATE, (k + 1, e)
    assert cnt == f.shape[0] % 20


@pytest.mark.parametrize("n", [n for n, _ in F.CASES])
def test_equations_of_motion_residual(n):
    """The host build's (acc, T) satisfy the equations of motion: residual <= max(1e-12, 10 x the reference's own
    stored error).  inverse_dynamics_error (pmrl.py) agrees with the residual written here."""
    from distributed_aerial_transportation_amd import pmrl

    c = F.case(n)
    for j in range(len(c.acc_at)):
        f = c.acc_force(j)
        for b in range(c.B):
            s = c.acc_state(j, b)
            acc, T = ph.forward(c.prm[b], n, pmrl.pack_pmrl_state(s), f[b])
            bound = max(1e-12, 10.0 * float(c.g("a_err")[j, b]))
            e = _residual(s, c.params[b], f[b], T, acc)
            assert e <= bound, (n, b, c.acc_at[j], e, bound)
            assert abs(pmrl.PMRLDynamics.inverse_dynamics_error(s, c.params[b], f[b], T, acc) - e) <= 1e-12
            # ... and it sees a wrong tension
            T2 = T.copy()
            T2[0] += 1e-6
            assert _residual(s, c.params[b], f[b], T2, acc) > 1e-7


def test_state_projections():
    from distributed_aerial_transportation_amd import pmrl

    rng = np.random.default_rng(5)
    q = rng.normal(size=(3, 5)) * 3.0
    dq = rng.normal(size=(3, 5))
    Rl = np.eye(3) + 0.1 * rng.normal(size=(3, 3))
    s = pmrl.PMRLState(q, dq, np.zeros(3), np.zeros(3), Rl, np.zeros(3))
    np.testing.assert_allclose(np.linalg.norm(s.q, axis=0), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(s.q, q / np.linalg.norm(q, axis=0), rtol=0, atol=1e-15)
    np.testing.assert_allclose((s.q * s.dq).sum(axis=0), 0.0, atol=1e-15)
    np.testing.assert_allclose(s.Rl.T @ s.Rl, np.eye(3), atol=1e-14)
    assert np.linalg.det(s.Rl) > 0
    # what the projections remove is normal to the constraint: dq changes along q only, Rl by a symmetric factor
    np.testing.assert_allclose(np.cross(dq - s.dq, s.q, axis=0), 0.0, atol=1e-14)
    P = s.Rl.T @ Rl
    np.testing.assert_allclose(P, P.T, atol=1e-14)
    # the fixture's start states, projected by the reference on construction, are fixed points
    c = F.case(3)
    s2 = pmrl.PMRLState(c.s0[0].q, c.s0[0].dq, c.s0[0].xl, c.s0[0].vl, c.s0[0].Rl, c.s0[0].wl)
    np.testing.assert_allclose(s2.q, c.s0[0].q, rtol=0, atol=2e-16)
    np.testing.assert_allclose(s2.dq, c.s0[0].dq, rtol=0, atol=2e-16)
    np.testing.assert_allclose(s2.Rl, c.s0[0].Rl, rtol=0, atol=1e-15)
    unproj = pmrl.PMRLState(q, dq, np.zeros(3), np.zeros(3), Rl, np.zeros(3), project=False)
    assert np.array_equal(unproj.q, q) and np.array_equal(unproj.Rl, Rl)


def test_layout():
    """The new offsets: named, disjoint from each other, inside the regions they borrow; nothing else moved."""
    from distributed_aerial_transportation_amd import layout as L

    for n in (3, 4, 6, 7, 16):
        # state: q at the head of the R region, dq the W region
        assert L.s_off("Q", n) == 0 == L.s_off("R", n)
        assert L.s_off("Q", n) + 3 * n <= L.s_off("R", n) + 9 * n
        assert L.s_off("DQ", n) == L.s_off("W", n) and L.s_off("DQ", n) + 3 * n == L.s_off("XL", n)
        assert L.state_size(n) == 12 * n + 18
        # parameters: m, L, U back to back inside the actuator-inertia region
        spans = [(L.p_off("PM_M", n), n), (L.p_off("PM_L", n), n), (L.p_off("PM_U", n), 9)]
        lo, hi = L.p_off("J", n), L.p_off("JINV", n)
        words = set()
        for o, w in spans:
            assert lo <= o and o + w <= hi, (n, o, w)
            assert not words & set(range(o, o + w))
            words |= set(range(o, o + w))
        assert max(words) + 1 == L.p_off("PM_END", n) <= hi
        assert L.param_size(n) == 41 + 27 * n and L.p_off("J", n) == 41 + 9 * n and L.p_off("JINV", n) == 41 + 18 * n


def test_pack_roundtrip():
    from distributed_aerial_transportation_amd import layout as L
    from distributed_aerial_transportation_amd import pmrl

    for n, _ in F.CASES:
        c = F.case(n)
        s = c.s0[1]
        x = pmrl.pack_pmrl_state(s)
        assert x.shape == (L.state_size(n),)
        assert not np.any(x[3 * n: 9 * n])  # the rest of the R region
        s2 = pmrl.unpack_pmrl_state(x, n)
        for a in ("q", "dq", "xl", "vl", "Rl", "wl"):
            assert np.array_equal(getattr(s, a), getattr(s2, a)), a
        assert np.array_equal(pmrl.pack_pmrl_state(s2), x)
        p = c.params[1]
        b = pmrl.pack_pmrl_params(p)
        assert b.shape == (L.param_size(n),)
        assert b[L.P["MT"]] == p.ml
        assert np.array_equal(b[L.p_off("PM_M", n): L.p_off("PM_M", n) + n], p.m)
        assert np.array_equal(b[L.p_off("PM_L", n): L.p_off("PM_L", n) + n], p.L)
        U = b[L.p_off("PM_U", n): L.p_off("PM_U", n) + 9].reshape(3, 3)
        assert np.array_equal(U, np.triu(U))
        np.testing.assert_allclose(U.T @ U, np.linalg.inv(p.Jl), rtol=1e-14)
        assert np.array_equal(b[L.p_off("R", n): L.p_off("R", n) + 3 * n].reshape(n, 3).T, p.r)
        assert not np.any(b[L.p_off("PM_END", n):])  # no actuator inertias


def test_lazy_exports():
    import distributed_aerial_transportation_amd as pkg

    assert pkg.PMRLDynamics is pkg.pmrl.PMRLDynamics and pkg.PMRLState is pkg.pmrl.PMRLState
    assert pkg.pack_pmrl_params is pkg.pmrl.pack_pmrl_params
