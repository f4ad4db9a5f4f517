"""Point-mass rigid-link system (system/point_mass_rigid_link.py): n point-mass robots carry the rigid payload
on rigid links.  ``PMRLParameters`` and ``PMRLState`` keep the reference's constructors; ``PMRLDynamics`` runs
``forward_dynamics`` and ``integrate`` on the device (k_pmrl_forward, k_pmrl_rollout: one lane per link, the link
tensions from the reduced 6 x 6 system of csrc/dat_pmrl_step.hpp).

Blocks (csrc/dat_layout.h): a PMRL scenario lives in the state block every other system uses -- q (3n, agent-major) at
DAT_S_Q, the head of the R region whose rest is zero, dq (3n) at DAT_S_DQ = DAT_S_W, the payload and the int counter
where they are -- so ``set_state`` / ``get_state`` and checkpoints carry it unchanged.  Its parameter block has ml,
Jl, Jl^-1 in MT, JT, JTI and r in R and RCOM like the rigid payload's, and m, L and the upper Cholesky factor of
Jl^-1 at DAT_P_PM_M, DAT_P_PM_L, DAT_P_PM_U inside the actuator-inertia region, which the system does not have.
"""

from __future__ import annotations

import numpy as np

from . import layout as L
from .system import GRAVITY, _polar, _skew


class PMRLParameters:
    """system/point_mass_rigid_link.py:37-64: robot masses m (n), payload mass ml and inertia Jl (3, 3, body frame),
    link attachment points r (3, n, body frame), link lengths L (n)."""

    def __init__(self, m: np.ndarray, ml: float, Jl: np.ndarray, r: np.ndarray, L: np.ndarray) -> None:
        m, Jl, r, L = (np.asarray(a, float) for a in (m, Jl, r, L))
        self.n = m.shape[0]
        assert m.shape == (self.n,) and Jl.shape == (3, 3) and r.shape == (3, self.n) and L.shape == (self.n,)
        self.m, self.ml, self.Jl, self.r, self.L = m, float(ml), Jl, r, L
        self.Jl_inv = np.linalg.inv(Jl)
        self.Jl_inv_chol = np.linalg.cholesky(self.Jl_inv).T  # upper: U'U = Jl^-1 (scipy.linalg.cholesky, :59)


class PMRLState:
    """system/point_mass_rigid_link.py:67-111: link directions q (3, n) in (S^2)^n with tangent rates dq, payload
    xl, vl, Rl, wl.  q, dq and Rl are projected on construction, as the reference does."""

    def __init__(self, q, dq, xl, vl, Rl, wl, project: bool = True) -> None:
        self.q, self.dq = np.array(q, float), np.array(dq, float)
        assert self.q.shape == self.dq.shape and self.q.shape[0] == 3
        self.xl, self.vl = np.array(xl, float), np.array(vl, float)
        self.Rl, self.wl = np.array(Rl, float), np.array(wl, float)
        assert self.xl.shape == (3,) and self.vl.shape == (3,) and self.Rl.shape == (3, 3) and self.wl.shape == (3,)
        if project:
            self.project_q()
            self.project_R()
        self.counter = 0

    def project_q(self) -> None:
        """q onto (S^2)^n, dq onto the tangent space at the new q (:101-105)."""
        nq = np.linalg.norm(self.q, axis=0)
        assert np.all(nq > 0)
        self.q = self.q / nq
        self.dq = self.dq - self.q * (self.q * self.dq).sum(axis=0)

    def project_R(self) -> None:
        """Rl onto SO(3): its orthogonal polar factor (:107-111)."""
        self.Rl = _polar(self.Rl)


def pack_pmrl_params(p: PMRLParameters) -> np.ndarray:
    """The PMRL parameter block (module docstring); every word the system does not use is zero."""
    n = p.n
    assert n >= 3
    b = np.zeros(L.param_size(n))
    P = L.P
    b[P["MT"]] = p.ml
    b[P["ML"]] = p.ml
    b[P["JT"]: P["JT"] + 9] = p.Jl.reshape(-1)
    b[P["JTI"]: P["JTI"] + 9] = p.Jl_inv.reshape(-1)
    b[L.p_off("R", n): L.p_off("R", n) + 3 * n] = p.r.T.reshape(-1)
    b[L.p_off("RCOM", n): L.p_off("RCOM", n) + 3 * n] = p.r.T.reshape(-1)
    b[L.p_off("PM_M", n): L.p_off("PM_M", n) + n] = p.m
    b[L.p_off("PM_L", n): L.p_off("PM_L", n) + n] = p.L
    b[L.p_off("PM_U", n): L.p_off("PM_U", n) + 9] = p.Jl_inv_chol.reshape(-1)
    return b


def pack_pmrl_state(s: PMRLState) -> np.ndarray:
    """PMRLState as a dat state block."""
    n = s.q.shape[1]
    x = np.zeros(L.state_size(n))
    x[L.s_off("Q", n): L.s_off("Q", n) + 3 * n] = s.q.T.reshape(-1)
    x[L.s_off("DQ", n): L.s_off("DQ", n) + 3 * n] = s.dq.T.reshape(-1)
    x[L.s_off("XL", n): L.s_off("XL", n) + 3] = s.xl
    x[L.s_off("VL", n): L.s_off("VL", n) + 3] = s.vl
    x[L.s_off("RL", n): L.s_off("RL", n) + 9] = s.Rl.reshape(-1)
    x[L.s_off("WL", n): L.s_off("WL", n) + 3] = s.wl
    return x


def unpack_pmrl_state(x: np.ndarray, n: int) -> PMRLState:
    """The state block's words as they are (no projection)."""
    oq, od, o = L.s_off("Q", n), L.s_off("DQ", n), L.s_off("XL", n)
    return PMRLState(x[oq:oq + 3 * n].reshape(n, 3).T, x[od:od + 3 * n].reshape(n, 3).T, x[o:o + 3], x[o + 3:o + 6],
                     x[o + 6:o + 15].reshape(3, 3), x[o + 15:o + 18], project=False)


class PMRLDynamics:
    """PMRLDynamics of system/point_mass_rigid_link.py:135-254 on the device.

    Robot i is a point mass at x_i = xl + L_i q_i + Rl r_i, pulled by its thrust f_i (the input, ground frame) and
    by its link, whose tension (or compression) T_i acts along q_i.  Equations of motion, e3 = (0, 0, 1):
        m_i x_i'' = f_i - m_i g e3 - T_i q_i                      (each robot)
        ml vl'    = sum_i T_i q_i - ml g e3                        (payload, translation)
        Jl wl' + wl x (Jl wl) = sum_i r_i x (T_i Rl' q_i)          (payload, rotation, body frame)
        q_i . q_i'' = -|q_i'|^2                                    (the links stay unit vectors)
    """

    def __init__(self, params: PMRLParameters, state: PMRLState, dt: float, device: int = 0) -> None:
        from .control import BatchedController

        assert params.m.shape[0] == state.q.shape[1]
        self.num_quadrotors = self.n = params.n
        self.params, self.dt = params, dt
        self.gravity = -GRAVITY * np.array([0.0, 0.0, 1.0])
        self._eng = BatchedController("centralized", self.n, 1, pack_pmrl_params(params), dt=dt, device=device)
        self._eng.set_state(pack_pmrl_state(state)[None], np.array([state.counter], dtype=np.int32))

    def forward_dynamics(self, f: np.ndarray):
        """(ddq (3, n), dvl, dwl), T (n) under the thrusts f (3, n) at the current state (k_pmrl_forward)."""
        f = np.asarray(f, float)
        assert f.shape == (3, self.n)
        (ddq, dvl, dwl), T = self._eng.pmrl_forward(f[None])
        return (ddq[0], dvl[0], dwl[0]), T[0]

    def integrate(self, f: np.ndarray, steps: int = 1) -> None:
        """`steps` steps of dt with the thrusts f (3, n) held (k_pmrl_rollout)."""
        f = np.asarray(f, float)
        assert f.shape == (3, self.n)
        self._eng.pmrl_rollout(steps, f[None])

    @property
    def state(self) -> PMRLState:
        x, c = self._eng.get_state()
        s = unpack_pmrl_state(x[0], self.n)
        s.counter = int(c[0])
        return s

    @staticmethod
    def inverse_dynamics_error(s: PMRLState, p: PMRLParameters, f: np.ndarray, T: np.ndarray, acc) -> float:
        """Norm of the residual of the equations of motion above at (s, f) for the tensions T and the
        accelerations acc = (ddq, dvl, dwl) (:210-249); a host NumPy diagnostic."""
        ddq, dvl, dwl = acc
        g3 = GRAVITY * np.array([[0.0], [0.0], [1.0]])
        W = _skew(s.wl)
        dv_quad = np.vstack(dvl) + ddq * p.L + s.Rl @ (W @ W + _skew(dwl)) @ p.r
        quad = np.linalg.norm(dv_quad * p.m - f + g3 * p.m + s.q * T) ** 2
        load = np.linalg.norm(p.ml * dvl - s.q @ T + p.ml * g3.T) ** 2
        c = np.cross(p.r, s.Rl.T @ s.q, axisa=0, axisb=0, axisc=0)
        ang = np.linalg.norm(p.Jl @ dwl + W @ p.Jl @ s.wl - c @ T) ** 2
        tan = np.linalg.norm((s.q * ddq).sum(axis=0) + np.linalg.norm(s.dq, axis=0) ** 2) ** 2
        return float(np.sqrt(quad + load + ang + tan))


__all__ = ["PMRLParameters", "PMRLState", "PMRLDynamics", "pack_pmrl_params", "pack_pmrl_state", "unpack_pmrl_state"]
