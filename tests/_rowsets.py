"""Row sets for the tests of the Farkas certificate of infeasible dvl rows (dvl_rows_infeasible, csrc/dat_qp.hpp):
a seeded generator of C-ADMM agent QPs whose env rows are built around an "infeasible core", a feasibility oracle
that shares nothing with the code under test (the Chebyshev margin of the row system, an LP solved by scipy's
HiGHS), the QP oracle (oracle.model.build_qp + oracle.ipm.solve_qp), and the assertions the host-build test
(test_certificate_host.py) and the GPU test (test_gpu_certificate.py) both make.

A family fixes a state, the agent's multipliers and a set of row normals; its 11 items differ in the margin m only.
The core rows pass at distance m from a point x0 (|x0|inf <= 1), a_k . (dvl - x0) >= -m_k |a_k|, with normals that
positively span a line, a plane or R^3, so the core alone has Chebyshev margin exactly m: strictly feasible for
m > 0, infeasible by |m| for m < 0.  Core kinds: an antiparallel pair, a coplanar triple in a random plane, a
coplanar triple of exactly horizontal normals (a_z = 0, the rows of vertical trees), four normals of a perturbed
tetrahedron, and a core one member of which is the QP's own |vl| base row -2 vl . dvl >= |vl|^2 - 1 (an env row
antiparallel to it, or two that complete a coplanar triple; the state's |vl| is drawn in [0.6, 0.85] so that x0,
which lies on that row's boundary, stays inside the unit box; the env members take the margin m sum(lambda) /
sum(lambda_env), which makes the core's Chebyshev margin m again).  Normals are scaled by 10^U(-3, 1) (the rows
of real trees carry |a| ~ 6e-4); 0 .. 10 - core decoy rows, satisfied at x0 with slack >= 0.5 |a|, are added (the
first three of them parallel, of the same direction: the pair branch must tell them from an antiparallel pair,
and subsystems of rank 1 or 2 must certify nothing) and
all rows permuted.  Three fixed families: 10 env rows (with the |vl| row all 550 subsystems are visited), no env row,
one env row.

Items are classified by the LP's margin t over the env rows and the |vl| row, not by m: decoys and the |vl| row
make some m > 0 items infeasible."""

import functools
from dataclasses import dataclass

import numpy as np
from scipy.optimize import linprog

from oracle import model as om
from oracle import scenarios as osc
from oracle.ipm import OPTIMAL, solve_qp

NS = (3, 6, 16)
MARGINS = (1e-2, 1e-4, 1e-6, 1e-8, -1e-8, -1e-6, -1e-5, -1e-4, -1e-3, -1e-2, -1.0)
KINDS = ("pair", "triple", "triple_h", "tetra", "vl")
FAMILIES = 40
T_CERT = -1e-4  # at and below this margin the certificate must fire
REL = 1e-5      # the suite's relative tolerance on a QP's solution
NENV = 10


@dataclass
class Family:
    n: int
    kind: str
    state: om.State
    acc: np.ndarray     # (6,)
    lam: np.ndarray     # (3, n)
    fm: np.ndarray      # (3, n)
    agent: int
    x0: np.ndarray
    core: np.ndarray    # (kc, 3) scaled normals of the env members of the core
    scale_m: float      # margin of the env core rows per unit of the core's Chebyshev margin
    decoy: np.ndarray   # (kd, 3)
    decoy_slack: np.ndarray  # (kd,) in units of |a|
    perm: np.ndarray

    def rows(self, m):
        """compacted env rows (lhs (k, 3), rhs (k,)): lhs . dvl >= rhs"""
        nc = np.linalg.norm(self.core, axis=1)
        nd = np.linalg.norm(self.decoy, axis=1)
        lhs = np.vstack([self.core, self.decoy]).reshape(-1, 3)
        rhs = np.concatenate([self.core @ self.x0 - m * self.scale_m * nc, self.decoy @ self.x0 - self.decoy_slack * nd])
        return lhs[self.perm], rhs[self.perm]


@dataclass
class Case:
    fam: int
    m: float
    lhs: np.ndarray
    rhs: np.ndarray
    t: float            # Chebyshev margin of the dvl rows (LP)
    oracle_status: int  # oracle.ipm status; -1: not solved (t <= T_CERT)
    oracle_x: np.ndarray  # (3n,) agent-major, the oracle's f


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _rand_state(rng, n):
    """as tests/test_hostsim.py::_rand_state"""
    R = np.stack([om.exp3(rng.uniform(-0.3, 0.3, 3)) for _ in range(n)], 2)
    return om.State(R, rng.uniform(-0.5, 0.5, (3, n)), rng.uniform(-1, 1, 3), rng.uniform(-0.5, 0.5, 3),
                    om.exp3(rng.uniform(-0.1, 0.1, 3)), rng.uniform(-0.2, 0.2, 3))


def _plane_triple(rng, e1, e2, first=None):
    """three unit normals in span(e1, e2) that positively span it (gaps below pi); `first` fixes the first angle"""
    th0 = rng.uniform(0, 2 * np.pi) if first is None else first
    th = th0 + np.array([0.0, 2 * np.pi / 3 + rng.uniform(-0.4, 0.4), 4 * np.pi / 3 + rng.uniform(-0.4, 0.4)])
    return np.outer(np.cos(th), e1) + np.outer(np.sin(th), e2)


def _weights(U):
    """lambda > 0 with sum_k lambda_k U_k = 0 (the one-dimensional null space of U')"""
    lam = np.linalg.svd(U.T)[2][-1]
    lam = lam * np.sign(lam[0])
    assert np.all(lam > 0.02 * lam.sum()) and np.max(np.abs(lam @ U)) < 1e-12
    return lam


def _tetra(rng):
    T = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
    while True:
        U = T @ om.exp3(rng.uniform(-np.pi, np.pi, 3)).T + rng.normal(0, 0.2, (4, 3))
        U /= np.linalg.norm(U, axis=1, keepdims=True)
        lam = np.linalg.svd(U.T)[2][-1]
        lam = lam * np.sign(lam[0])
        if np.all(lam > 0.05 * np.sum(np.abs(lam))):
            return U


def _scales(rng, k):
    return 10.0 ** rng.uniform(-3, 1, k)


def _family(rng, n, kind, ndecoy=None):
    p = osc.params(n)
    s = _rand_state(rng, n)
    x0 = rng.uniform(-1, 1, 3)
    scale_m = 1.0
    if kind == "pair":
        u = _unit(rng)
        U = np.array([u, -u])
    elif kind == "triple":
        e1 = _unit(rng)
        e2 = np.cross(e1, _unit(rng))
        U = _plane_triple(rng, e1, e2 / np.linalg.norm(e2))
    elif kind == "triple_h":
        U = _plane_triple(rng, np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))
        assert np.all(U[:, 2] == 0.0)
    elif kind == "tetra":
        U = _tetra(rng)
    elif kind == "vl":
        # the |vl| row a_v . dvl >= |vl|^2 - 1, a_v = -2 vl, is a member; x0 lies on its boundary
        s.vl = rng.uniform(0.6, 0.85) * _unit(rng)
        uv = -s.vl / np.linalg.norm(s.vl)
        dv = (1.0 - s.vl @ s.vl) / (2.0 * np.linalg.norm(s.vl))
        e2 = np.cross(uv, _unit(rng))
        e2 /= np.linalg.norm(e2)
        x0 = -dv * uv + rng.uniform(-0.4, 0.4) * e2
        assert np.max(np.abs(x0)) <= 1.0
        if rng.integers(2):
            Ufull = np.array([uv, -uv])
        else:
            Ufull = _plane_triple(rng, uv, e2, first=0.0)
        lam = np.array([1.0, 1.0]) if len(Ufull) == 2 else _weights(Ufull)
        scale_m = lam.sum() / lam[1:].sum()
        U = Ufull[1:]
    elif kind == "single":  # one env row at distance m from x0
        U = _unit(rng)[None]
    elif kind == "none":
        U = np.zeros((0, 3))
    else:
        raise ValueError(kind)
    core = U * _scales(rng, len(U))[:, None]
    if ndecoy is None:
        ndecoy = int(rng.integers(0, NENV - len(core) + 1))
    decoy = np.array([_unit(rng) for _ in range(ndecoy)]).reshape(-1, 3) * _scales(rng, ndecoy)[:, None]
    for j in range(1, min(ndecoy, 3)):
        # parallel rows of the same direction (scales and slacks differ): pairs with a vanishing cross product that
        # certify nothing, and with the core's pair or with each other triples and 4-sets of rank 1 or 2, whose
        # cofactors are rounding remnants
        decoy[j] = decoy[0] * (np.linalg.norm(decoy[j]) / np.linalg.norm(decoy[0]))
    feq = om.equilibrium_forces(p)
    return Family(n=n, kind=kind, state=s, acc=rng.uniform(-5, 5, 6), lam=rng.normal(0, 0.5, (3, n)),
                  fm=feq + rng.normal(0, 1, (3, n)), agent=int(rng.integers(n)), x0=x0, core=core, scale_m=scale_m,
                  decoy=decoy, decoy_slack=rng.uniform(0.5, 2.0, ndecoy), perm=rng.permutation(len(core) + ndecoy))


def chebyshev_margin(lhs, rhs, vl, max_vl_sq=1.0):
    """max t  s.t.  a_j . x - rhs_j >= t |a_j| over the env rows and the |vl| row, |x|inf <= 1e6, t <= 1"""
    A = np.vstack([np.asarray(lhs, float).reshape(-1, 3), -2.0 * vl])
    b = np.concatenate([np.asarray(rhs, float).reshape(-1), [vl @ vl - max_vl_sq]])
    nrm = np.linalg.norm(A, axis=1)
    assert np.all(nrm > 0)
    Aub = np.column_stack([-A / nrm[:, None], np.ones(len(b))])
    r = linprog([0, 0, 0, -1.0], A_ub=Aub, b_ub=-b / nrm, bounds=[(-1e6, 1e6)] * 3 + [(None, 1.0)], method="highs",
                options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
    assert r.status == 0, r.message
    return float(r.x[3])


@functools.lru_cache(maxsize=None)
def families(n):
    rng = np.random.default_rng(7000 + n)
    fams = [_family(rng, n, KINDS[k % len(KINDS)]) for k in range(FAMILIES)]
    fams.append(_family(rng, n, "tetra", ndecoy=6))  # nenv = 10
    fams.append(_family(rng, n, "none", ndecoy=0))   # nenv = 0
    fams.append(_family(rng, n, "single", ndecoy=0))  # nenv = 1
    assert [len(f.perm) for f in fams[-3:]] == [10, 0, 1]
    return fams


@functools.lru_cache(maxsize=None)
def cases(n):
    """every (family, margin) item of team size n with its LP margin and the QP oracle's answer (computed once)"""
    p = osc.params(n)
    feq = om.equilibrium_forces(p)
    c = om.Consts.make(p, osc.col_radius(n), distributed=True)
    out = []
    for k, f in enumerate(families(n)):
        for m in MARGINS:
            lhs, rhs = f.rows(m)
            t = chebyshev_margin(lhs, rhs, f.state.vl, c.max_vl_sq)
            L, R = np.zeros((NENV, 3)), np.zeros(NENV)
            L[:len(rhs)], R[:len(rhs)] = lhs, rhs
            P, q, G, h, dims, A, b = om.build_qp("cadmm", p, c, f.state, (f.acc[:3], f.acc[3:]),
                                                 om.EnvRows(L, R, False, 1.0), i=f.agent, f_eq=feq, lam=f.lam, rho=1.0,
                                                 f_mean=f.fm)
            if t <= T_CERT:
                # rows infeasible by 1e-4 of their scale: no point meets the oracle's 1e-11 residuals, not solved
                out.append(Case(k, m, lhs, rhs, t, -1, np.full(3 * n, np.nan)))
                continue
            ro = solve_qp(P, q, G, h, dims, A, b)
            out.append(Case(k, m, lhs, rhs, t, ro.status, ro.x[9:].reshape(3, n, order="F").T.reshape(-1)))
    return out


def check(n, certified, status, iters, x):
    """The certificate's contract on cases(n): certified, status, iters (K,), x (K, 3n) agent-major.
    1. t >= 0          => not certified (no false positive)
    2. t <= -1e-4      => certified, status INFEASIBLE (2), 0 IPM iterations
    3. oracle OPTIMAL  => status OPTIMAL and x within 1e-5 relative of the oracle's
    4. -1e-4 < t < 0 is left to the IPM: nothing asserted, the status counts are printed per margin."""
    cs = cases(n)
    certified, status, iters = np.asarray(certified, bool), np.asarray(status), np.asarray(iters)
    assert len(cs) == len(certified) == len(status) == len(iters) == len(x)
    assert len(cs) % 64 != 0
    fams = families(n)
    worst, nfeas, ninf, nopt = 0.0, 0, 0, 0
    table = {m: [0, 0, 0, 0, 0] for m in MARGINS}  # feasible (t >= 0), certified, status 0 / 1 / 2
    for k, cse in enumerate(cs):
        tag = (n, fams[cse.fam].kind, cse.fam, cse.m, cse.t)
        row = table[cse.m]
        row[0] += cse.t >= 0
        row[1] += bool(certified[k])
        if status[k] in (0, 1, 2):
            row[2 + int(status[k])] += 1
        if cse.t >= 0.0:
            assert not certified[k], ("false positive", tag)
            nfeas += 1
        if cse.t <= T_CERT:
            assert certified[k] and status[k] == 2 and iters[k] == 0, ("not certified", tag, status[k], iters[k])
            ninf += 1
        if cse.oracle_status == OPTIMAL:
            assert status[k] == 0, ("oracle OPTIMAL", tag, status[k])
            rel = np.max(np.abs(x[k] - cse.oracle_x)) / max(1.0, np.max(np.abs(cse.oracle_x)))
            assert rel < REL, (tag, rel)
            worst = max(worst, rel)
            nopt += 1
    print(f"n = {n}: {len(cs)} items, {nfeas} with t >= 0 (none certified), {ninf} with t <= {T_CERT:g} (all "
          f"certified), {nopt} oracle-OPTIMAL (largest difference {worst:.1e})")
    print("      m   t>=0  certified  OPTIMAL  INACCURATE  INFEASIBLE")
    for m in MARGINS:
        r = table[m]
        print(f"{m:8.0e} {r[0]:6d} {r[1]:10d} {r[2]:8d} {r[3]:11d} {r[4]:11d}")
    # the generator must reach both sides in every core kind
    for kind in KINDS:
        ts = [cse.t for cse in cs if fams[cse.fam].kind == kind]
        assert min(ts) <= T_CERT and max(ts) >= 0.0, kind
    return table
