"""Long-double reference of the simulation step, written from the reference project's rules alone:
  system/rigid_quadrotor_payload.py:121-222   RQPParameters' derived constants (:70-84), project_R (:121-127),
                                              integrate (:129-148), forward_dynamics (:173-222)
  control/rqp_centralized.py:457-535          the gains (:488-496), _rotation_from_unit_vector (:503-516), control
                                              (:518-535: f = f_des . R e3, Rd from f_des / |f_des|, wd = dwd = 0)
  utils/so3_tracking_controllers.py:18-95     the "pd" law (:18-43) and the "sm" law (:60-95)
  system/rigid_payload.py:76-130              RPState.integrate (:77-88), RPDynamics.forward_dynamics (:107-130)
It shares no code with csrc/ or with oracle/model.py, and every operation is np.longdouble (64-bit mantissa, asserted
below): the float64 inputs are widened once and nothing is rounded back to double on the way.

Everything is batched: a leading axis of B scenarios, then the n agents.  R (B, n, 3, 3), w (B, n, 3), xl, vl, wl
(B, 3), Rl (B, 3, 3), f_des (B, n, 3), counter (B,).

The "sm" law as the reference evaluates it (:80-95 with wd = dwd = 0): S(r, y) = |y|^r sign(y) with np.sign, so
S(r, 0) = 0; the call T(e_R, r) (:92) against T = lambda r, y (:87) puts (|r| + 1e-6)^(e_R - 1) on the diagonal, the
arguments swapped relative to the paper.

exp3.  exp(hat v) = I + a hat(v) + b hat(v)^2, a = sin t / t, b = (1 - cos t) / t^2, t = |v|.  Below t = 0.25 both are
summed from their Taylor series (14 terms: the first one left out is below 0.25^28 / 29! ~ 1e-48), above it
b = 2 sin^2(t / 2) / t^2, which has no cancellation (1 - cos t loses half the digits at small t).

polar.  The orthogonal polar factor U of X (X = U P, P symmetric positive definite; scipy.linalg.polar of :125-127)
by Newton's iteration U <- (U + U^-T) / 2 with the inverse from the adjugate, in long double, until a sweep changes no
entry by more than 4 ulp.  The result is not taken on trust: every call measures |U'U - I| and the asymmetry of U'X and
takes the smallest diagonal entry of U'X, and keeps the worst in PolarProof; tests/test_sim_reference.py asserts
them for every matrix the reference projected (U orthogonal and U'X symmetric positive definite is the polar factor,
which is unique for nonsingular X).

case() is the input generator the CPU and GPU tests share (fixed seeds, nothing redrawn): per scenario it cycles
the regimes REGIMES, see Case."""

import functools
from dataclasses import dataclass, field

import numpy as np

from distributed_aerial_transportation_amd import layout as L

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, (
    f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: the simulation-step reference needs x87 extended "
    "precision or better to stand above float64")

G = LD(9.80665)                      # scipy.constants.g, the double (system/rigid_quadrotor_payload.py:170)
STEPS_PER_PROJECTION = 20            # system/rigid_quadrotor_payload.py:14, system/rigid_payload.py:12
K_R_PD, K_W_PD = LD(0.25), LD(0.075)  # control/rqp_centralized.py:488-489 (the doubles the controller holds)
SM_R, SM_K_R, SM_L_R, SM_K_S, SM_L_S = LD(0.5), LD(1.415), LD(0.707), LD(0.113), LD(0.057)  # :492-496
SM_EPS = LD(1e-6)                    # utils/so3_tracking_controllers.py:86
SERIES_BELOW = LD(0.25)


# ------------------------------------------------------------------------------------------ small helpers
def ld(a):
    return np.asarray(a, dtype=LD)


def hat(v):
    """(..., 3) -> (..., 3, 3), hat(v) u = v x u"""
    v = ld(v)
    z = np.zeros(v.shape[:-1], LD)
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1),
                     np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def vee(M):
    """pinocchio.unSkew of a skew-symmetric matrix"""
    return np.stack([M[..., 2, 1], M[..., 0, 2], M[..., 1, 0]], -1)


def mv(M, v):
    return (M @ v[..., None])[..., 0]


def T_(M):
    return np.swapaxes(M, -1, -2)


def eye(shape=()):
    return np.broadcast_to(np.eye(3, dtype=LD), tuple(shape) + (3, 3)).copy()


def inv3(M):
    """inverse of (..., 3, 3) by the adjugate"""
    M = ld(M)
    c = np.empty(M.shape, LD)
    for i in range(3):
        for j in range(3):
            a, b = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            minor = M[..., a[0], b[0]] * M[..., a[1], b[1]] - M[..., a[0], b[1]] * M[..., a[1], b[0]]
            c[..., j, i] = minor if (i + j) % 2 == 0 else -minor
    det = M[..., 0, 0] * c[..., 0, 0] + M[..., 0, 1] * c[..., 1, 0] + M[..., 0, 2] * c[..., 2, 0]
    return c / det[..., None, None]


def exp3(v):
    """exp(hat v), (..., 3) -> (..., 3, 3); see the module docstring"""
    v = ld(v)
    t2 = np.sum(v * v, -1)
    t = np.sqrt(t2)
    a_s, b_s = np.zeros(t.shape, LD), np.zeros(t.shape, LD)
    term_a, term_b = np.ones(t.shape, LD), np.full(t.shape, LD(0.5))
    for k in range(14):  # a = sum (-t^2)^k / (2k + 1)!, b = sum (-t^2)^k / (2k + 2)!
        a_s, b_s = a_s + term_a, b_s + term_b
        term_a = -term_a * t2 / LD((2 * k + 2) * (2 * k + 3))
        term_b = -term_b * t2 / LD((2 * k + 3) * (2 * k + 4))
    big = t >= SERIES_BELOW
    ts = np.where(big, t, LD(1))
    h = np.sin(ts / 2)
    a = np.where(big, np.sin(ts) / ts, a_s)
    b = np.where(big, 2 * h * h / (ts * ts), b_s)
    K = hat(v)
    return eye(t.shape) + a[..., None, None] * K + b[..., None, None] * (K @ K)


@dataclass
class PolarProof:
    """the worst of what polar() measured on its own results"""
    count: int = 0
    orth: float = 0.0      # max |U'U - I|
    asym: float = 0.0      # max |U'X - (U'X)'|
    min_diag: float = np.inf  # min diagonal entry of U'X


def polar(X, proof: PolarProof = None):
    """orthogonal polar factor of (..., 3, 3); see the module docstring"""
    X = ld(X)
    U = X.copy()
    tol = 4 * np.finfo(LD).eps
    for _ in range(100):
        Un = (U + T_(inv3(U))) / 2
        d = np.max(np.abs(Un - U)) if U.size else LD(0)
        U = Un
        if d <= tol:
            break
    else:
        raise AssertionError("polar: Newton's iteration did not settle")
    if proof is not None and U.size:
        P = T_(U) @ X
        proof.count += int(np.prod(U.shape[:-2]))
        proof.orth = max(proof.orth, float(np.max(np.abs(T_(U) @ U - eye(U.shape[:-2])))))
        proof.asym = max(proof.asym, float(np.max(np.abs(P - T_(P)))))
        proof.min_diag = min(proof.min_diag, float(np.min(np.stack([P[..., k, k] for k in range(3)]))))
    return U


# ------------------------------------------------------------------------------------------ parameters
class Params:
    """RQPParameters (system/rigid_quadrotor_payload.py:48-84) from m (B, n), J (B, n, 3, 3), ml (B,), Jl (B, 3, 3),
    r (B, n, 3): the float64 numbers given, the derived constants in long double.  B = 1 broadcasts over a batch."""

    def __init__(self, m, J, ml, Jl, r):
        self.m, self.J, self.ml, self.Jl, self.r = ld(m), ld(J), ld(ml), ld(Jl), ld(r)
        self.n = self.r.shape[1]
        self.mT = np.sum(self.m, 1) + self.ml                                        # :70
        self.x_com = np.sum(self.r * self.m[..., None], 1) / self.mT[:, None]        # :72
        self.r_com = self.r - self.x_com[:, None, :]                                 # :74
        hx = hat(self.x_com)
        JT = self.Jl - self.ml[:, None, None] * (hx @ hx)                            # :76
        hr = hat(self.r_com)
        self.JT = JT - np.sum(self.m[..., None, None] * (hr @ hr), 1)                # :77-80
        self.JT_inv = inv3(self.JT)                                                  # :81
        self.J_inv = inv3(self.J)                                                    # :82-84

    @staticmethod
    def single(m, J, ml, Jl, r):
        """from one scenario's reference-shaped arrays: m (n,), J (3, 3, n), ml, Jl (3, 3), r (3, n)"""
        return Params(np.asarray(m)[None], np.transpose(J, (2, 0, 1))[None], np.asarray([ml]), np.asarray(Jl)[None],
                      np.asarray(r).T[None])


class RPParams:
    """RPParameters (system/rigid_payload.py:33-47): ml (B,), Jl (B, 3, 3), r (B, n, 3)"""

    def __init__(self, ml, Jl, r):
        self.ml, self.Jl, self.r = ld(ml), ld(Jl), ld(r)
        self.Jl_inv = inv3(self.Jl)


@dataclass
class State:
    """RQPState (system/rigid_quadrotor_payload.py:87-119) without the projection at construction"""
    R: np.ndarray
    w: np.ndarray
    xl: np.ndarray
    vl: np.ndarray
    Rl: np.ndarray
    wl: np.ndarray
    counter: np.ndarray
    proof: PolarProof = field(default_factory=PolarProof)

    @staticmethod
    def of(R, w, xl, vl, Rl, wl, counter=None):
        R = ld(R).copy()
        c = np.zeros(R.shape[0], np.int64) if counter is None else np.array(counter, np.int64)
        return State(R, ld(w).copy(), ld(xl).copy(), ld(vl).copy(), ld(Rl).copy(), ld(wl).copy(), c)

    def block(self):
        """the dat state blocks (B, 12 n + 18), rounded to float64"""
        B, n = self.w.shape[:2]
        x = np.empty((B, L.state_size(n)))
        parts = (("R", self.R), ("W", self.w), ("XL", self.xl), ("VL", self.vl), ("RL", self.Rl), ("WL", self.wl))
        for name, a in parts:
            flat = a.reshape(B, -1)
            x[:, L.s_off(name, n): L.s_off(name, n) + flat.shape[1]] = flat.astype(np.float64)
        return x


# ------------------------------------------------------------------------------------------ the low-level law
def rotation_from_unit_vector(q):
    """control/rqp_centralized.py:503-516, q (..., 3) -> (..., 3, 3)"""
    sin_x = -q[..., 1]
    cos_x = np.sqrt(q[..., 0] ** 2 + q[..., 2] ** 2)
    sin_y, cos_y = q[..., 0] / cos_x, q[..., 2] / cos_x
    zero = np.zeros(sin_x.shape, LD)
    c0 = np.stack([cos_y, zero, -sin_y], -1)
    c1 = np.stack([sin_x * sin_y, cos_x, cos_y * sin_x], -1)
    return np.stack([c0, c1, q], -1)  # the columns


def _S(r, y):
    return np.power(np.abs(y), r) * np.sign(y)  # utils/so3_tracking_controllers.py:83


def low_level(R, w, J, f_des, kind):
    """RQPLowLevelController.control (control/rqp_centralized.py:518-535) with the "pd" or "sm" law and wd = dwd = 0:
    (thrust (B, n), moment (B, n, 3))"""
    R, w, J, f_des = ld(R), ld(w), ld(J), ld(f_des)
    f = np.sum(f_des * R[..., :, 2], -1)                                             # :527
    qd = f_des / np.sqrt(np.sum(f_des * f_des, -1))[..., None]                       # :529
    Rd = rotation_from_unit_vector(qd)                                               # :530
    RdtR = T_(Rd) @ R
    e_R = vee(RdtR - T_(RdtR)) / 2                                                   # so3 :34, :80
    gyro = np.cross(w, mv(J, w))
    if kind == "pd":
        return f, -K_R_PD * e_R - K_W_PD * w + gyro                                  # :37-42
    assert kind == "sm", kind
    RtRd = T_(RdtR)
    tr = RtRd[..., 0, 0] + RtRd[..., 1, 1] + RtRd[..., 2, 2]
    E = (tr[..., None, None] * eye(tr.shape) - RtRd) / 2                             # :82
    s = w + SM_K_R * e_R + SM_L_R * _S(SM_R, e_R)                                    # :84
    Tdiag = np.power(np.abs(SM_R) + SM_EPS, e_R - 1)                                 # :87 called as T(e_R, r), :92
    Ew = mv(E, w)
    last = SM_K_R * mv(J, Ew) + SM_L_S * SM_R * mv(J, Tdiag * Ew)                    # (k_R J + l_s r J T) E e_W
    return f, -SM_K_S * s - SM_L_S * _S(SM_R, s) + gyro - last                       # :88-94


# ------------------------------------------------------------------------------------------ dynamics
def forward_dynamics(p: Params, s: State, f, M):
    """RQPDynamics.forward_dynamics (system/rigid_quadrotor_payload.py:173-222): (dw (B, n, 3), dvl, dwl (B, 3))"""
    f, M = ld(f), ld(M)
    dw = mv(p.J_inv, M - np.cross(s.w, mv(p.J, s.w)))                                # :192-198
    quad_force = s.R[..., :, 2] * f[..., None]                                       # :200
    dv_com = np.sum(quad_force, 1) / p.mT[:, None]                                   # :201
    dv_com[:, 2] -= G
    body = mv(T_(s.Rl)[:, None], quad_force)
    net = np.sum(np.cross(p.r_com, body), 1)                                         # :202-211
    dwl = mv(p.JT_inv, net - np.cross(s.wl, mv(p.JT, s.wl)))                         # :212-214
    hw = hat(s.wl)
    dvl = dv_com - mv(s.Rl @ (hw @ hw + hat(dwl)), np.broadcast_to(p.x_com, dwl.shape))  # :216-221
    return dw, dvl, dwl


def _project_due(s: State, rotations):
    s.counter += 1                                                                   # :145
    due = s.counter >= STEPS_PER_PROJECTION                                          # :146
    if np.any(due):
        for name in rotations:
            a = getattr(s, name)
            a[due] = polar(a[due], s.proof)                                          # :121-127
        s.counter[due] = 0


def integrate(s: State, dw, dvl, dwl, dt):
    """RQPState.integrate (system/rigid_quadrotor_payload.py:129-148), the Lie-midpoint step, in place"""
    dt = LD(dt)
    s.R = s.R @ exp3((s.w + dw * dt / 2) * dt)                                       # :137-139
    s.w = s.w + dw * dt
    s.xl = s.xl + s.vl * dt + dvl * dt ** 2 / 2                                      # :141
    s.vl = s.vl + dvl * dt
    s.Rl = s.Rl @ exp3((s.wl + dwl * dt / 2) * dt)                                   # :143
    s.wl = s.wl + dwl * dt
    _project_due(s, ("Rl", "R"))


def sim_step(p: Params, s: State, f_des, dt, kind):
    f, M = low_level(s.R, s.w, p.J, f_des, kind)
    integrate(s, *forward_dynamics(p, s, f, M), dt)
    return f, M


def rp_step(p: RPParams, s: State, f, dt):
    """RPDynamics.integrate (system/rigid_payload.py:107-130, 77-88) on the payload part of s; f (B, n, 3)"""
    f, dt = ld(f), LD(dt)
    dvl = np.sum(f, 1) / p.ml[:, None]                                               # :119, :125
    dvl[:, 2] -= G
    net = np.sum(np.cross(p.r, mv(T_(s.Rl)[:, None], f)), 1)                         # :120-123
    dwl = mv(p.Jl_inv, net - np.cross(s.wl, mv(p.Jl, s.wl)))                         # :126-128
    s.xl = s.xl + s.vl * dt + dvl * dt ** 2 / 2                                      # :81
    s.vl = s.vl + dvl * dt
    s.Rl = s.Rl @ exp3((s.wl + dwl * dt / 2) * dt)                                   # :83
    s.wl = s.wl + dwl * dt
    _project_due(s, ("Rl",))


# ------------------------------------------------------------------------------------------ the shared inputs
REGIMES = ("rest", "small", "large", "beyond", "spin", "down")
COUNTERS = (0, 7, 19, 13)  # cycled per scenario: projections on different steps inside a wavefront, 19: on the first
DT = 1e-3
STEPS = 45
LOW_LEVEL_SHAPES = ((3, 23), (5, 13), (7, 10), (16, 5))
ROLLOUT_SHAPES = ((3, 22), (5, 13), (7, 10), (11, 6), (16, 5))
PER_SCENARIO_SHAPE = (6, 11)
# (seed 1900 is not used: under "sm" its scenario 3, agent 5 reaches the sliding surface in yaw, see
# test_sim_reference.py's docstring)
PER_SCENARIO_SEED = 1901
RP_SHAPE = (3, 70)


@dataclass
class Case:
    """One batch of inputs, float64 (what the device is given).  Scenario b is in regime REGIMES[b % 6]:
      rest    R = I, w = 0, the payload at rest at the origin, f_des exactly (0, 0, fz), fz ~ U(2, 7)
      small   R = exp3(U(-0.3, 0.3)^3), w ~ U(-0.5, 0.5)^3
      large   R = exp3(angle * axis), angle ~ U(0.3, 1.2), uniform axis, w ~ U(-0.5, 0.5)^3
      beyond  as large with angle ~ U(1.2, 2.5): against f_des the attitude error passes 90 degrees
      spin    as large with w ~ U(-2, 2)^3
      down    as small, the z component of f_des negated (negative thrust)
    f_des is x, y ~ U(-3, 3), z ~ U(2, 7) per agent otherwise, so its unit vector has sqrt(q_x^2 + q_z^2) >=
    2 / sqrt(22) = 0.43 (down: the same with -z), away from the +-y axis where the reference divides by zero.  The
    payload follows scenarios.perturbed_states: xl ~ U(-1, 1)^3, vl ~ U(-0.5, 0.5)^3, Rl = exp3(U(-0.1, 0.1)^3),
    wl ~ U(-0.2, 0.2)^3.  The rotations are the long-double exp3 rounded to float64."""
    n: int
    B: int
    R: np.ndarray        # (B, n, 3, 3)
    w: np.ndarray        # (B, n, 3)
    xl: np.ndarray
    vl: np.ndarray
    Rl: np.ndarray
    wl: np.ndarray
    f_des: np.ndarray    # (B, n, 3)
    counters: np.ndarray  # (B,) int32
    m: np.ndarray        # (Bp, n): Bp = 1 (shared parameters) or B
    J: np.ndarray        # (Bp, n, 3, 3)
    ml: np.ndarray       # (Bp,)
    Jl: np.ndarray       # (Bp, 3, 3)
    r: np.ndarray        # (Bp, n, 3)
    per_scenario: bool

    def regime(self, b):
        return REGIMES[b % len(REGIMES)]

    def rest(self):
        return np.arange(self.B) % len(REGIMES) == 0

    def state(self, counters=True):
        return State.of(self.R, self.w, self.xl, self.vl, self.Rl, self.wl, self.counters if counters else None)

    def params(self):
        return Params(self.m, self.J, self.ml, self.Jl, self.r)

    def blocks(self):
        return self.state().block()

    def f_des_3n(self):
        """(B, 3, n), as BatchedController.low_level and rollout take it"""
        return np.ascontiguousarray(self.f_des.transpose(0, 2, 1))

    def system_params(self, b):
        """scenario b's system.RQPParameters (what system.pack_params packs)"""
        from distributed_aerial_transportation_amd import system

        k = b if self.per_scenario else 0
        return system.RQPParameters(self.m[k].copy(), np.ascontiguousarray(self.J[k].transpose(1, 2, 0)),
                                    float(self.ml[k]), self.Jl[k].copy(), np.ascontiguousarray(self.r[k].T))

    def param_blocks(self):
        """the parameter block(s) of system.pack_params: (P,) shared, (B, P) per scenario"""
        from distributed_aerial_transportation_amd import scenarios, system

        col = scenarios.collision(self.n)
        if not self.per_scenario:
            return system.pack_params(self.system_params(0), col)
        return np.stack([system.pack_params(self.system_params(b), col) for b in range(self.B)])


def _rot(rng, lo, hi):
    axis = rng.normal(size=3)
    return axis / np.linalg.norm(axis) * rng.uniform(lo, hi)


@functools.lru_cache(maxsize=None)
def case(n, B, seed, per_scenario=False) -> Case:
    from distributed_aerial_transportation_amd import scenarios

    rng = np.random.default_rng(seed)
    rv, w = np.zeros((B, n, 3)), np.zeros((B, n, 3))
    xl, vl, rvl, wl = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, 3))
    f_des = np.zeros((B, n, 3))
    for b in range(B):
        reg = REGIMES[b % len(REGIMES)]
        f_des[b, :, :2] = rng.uniform(-3, 3, (n, 2))
        f_des[b, :, 2] = rng.uniform(2, 7, n)
        if reg == "rest":
            f_des[b, :, :2] = 0.0
            continue
        xl[b], vl[b] = rng.uniform(-1, 1, 3), rng.uniform(-0.5, 0.5, 3)
        rvl[b], wl[b] = rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.2, 0.2, 3)
        w[b] = rng.uniform(-2, 2, (n, 3)) if reg == "spin" else rng.uniform(-0.5, 0.5, (n, 3))
        for i in range(n):
            if reg in ("small", "down"):
                rv[b, i] = rng.uniform(-0.3, 0.3, 3)
            else:
                rv[b, i] = _rot(rng, *((1.2, 2.5) if reg == "beyond" else (0.3, 1.2)))
        if reg == "down":
            f_des[b, :, 2] *= -1.0
    m, J, ml, Jl, r = scenarios.geometry(n)
    if per_scenario:
        Jb = np.stack([np.transpose(J, (2, 0, 1)) * rng.uniform(0.7, 1.4, n)[:, None, None] for _ in range(B)])
        mlb = rng.uniform(0.15, 0.30, B)
        Jlb = np.stack([Jl * np.diag(rng.uniform(0.8, 1.2, 3)) for _ in range(B)])
        mb, rb = np.tile(m, (B, 1)), np.tile(r.T, (B, 1, 1))
    else:
        Jb, mlb, Jlb, mb, rb = np.transpose(J, (2, 0, 1))[None], np.array([ml]), Jl[None], m[None], r.T[None]
    counters = np.array([COUNTERS[b % len(COUNTERS)] for b in range(B)], dtype=np.int32)
    return Case(n, B, exp3(rv).astype(np.float64), w, xl, vl, exp3(rvl).astype(np.float64), wl, f_des, counters,
                mb, Jb, mlb, Jlb, rb, per_scenario)


def low_level_cases():
    """(n, B, seed, per_scenario) of the k_low_level checks"""
    return [(n, B, 1000 + n, False) for n, B in LOW_LEVEL_SHAPES] + [PER_SCENARIO_SHAPE + (PER_SCENARIO_SEED, True)]


def rollout_cases():
    """(n, B, seed, per_scenario) of the k_rollout_agents checks"""
    return [(n, B, 2000 + n, False) for n, B in ROLLOUT_SHAPES] + [PER_SCENARIO_SHAPE + (PER_SCENARIO_SEED, True)]


@functools.lru_cache(maxsize=None)
def low_level_reference(n, B, seed, per_scenario, kind):
    """(thrust (B, n), moment (B, n, 3)) of the case, long double"""
    c = case(n, B, seed, per_scenario)
    return low_level(c.R, c.w, c.params().J, c.f_des, kind)


@functools.lru_cache(maxsize=None)
def rollout_reference(n, B, seed, per_scenario, kind, steps=STEPS) -> State:
    """the case's state after `steps` steps of DT under its f_des, from its staggered counters"""
    c = case(n, B, seed, per_scenario)
    p, s = c.params(), c.state()
    for _ in range(steps):
        sim_step(p, s, c.f_des, DT, kind)
    return s


@dataclass
class RPCase:
    """k_rp_rollout's inputs: n = 3 actuators, the payload Rl = exp3(U(-0.5, 0.5)^3), xl ~ U(-1, 1)^3, vl, wl ~
    U(-0.5, 0.5)^3, forces x, y ~ U(-1, 1), z ~ U(0, 4), the staggered counters; the actuator part of the state block
    (which rp_step must leave alone) holds attitudes exp3(U(-1, 1)^3) and rates U(-1, 1)^3."""
    n: int
    B: int
    blocks: np.ndarray   # (B, 12 n + 18)
    f: np.ndarray        # (B, n, 3)
    counters: np.ndarray
    ml: float
    Jl: np.ndarray
    r: np.ndarray        # (n, 3)

    def state(self):
        n, x = self.n, self.blocks
        o = L.s_off("XL", n)
        return State.of(x[:, :9 * n].reshape(-1, n, 3, 3), x[:, 9 * n:12 * n].reshape(-1, n, 3), x[:, o:o + 3],
                        x[:, o + 3:o + 6], x[:, o + 6:o + 15].reshape(-1, 3, 3), x[:, o + 15:o + 18], self.counters)

    def params(self):
        return RPParams(np.array([self.ml]), self.Jl[None], self.r[None])


@functools.lru_cache(maxsize=None)
def rp_case(seed=3000) -> RPCase:
    from distributed_aerial_transportation_amd import rigid_payload as rp

    n, B = RP_SHAPE
    rng = np.random.default_rng(seed)
    p, _, _ = rp.rp_setup(n)
    s = State.of(exp3(rng.uniform(-1, 1, (B, n, 3))).astype(np.float64), rng.uniform(-1, 1, (B, n, 3)),
                 rng.uniform(-1, 1, (B, 3)), rng.uniform(-0.5, 0.5, (B, 3)),
                 exp3(rng.uniform(-0.5, 0.5, (B, 3))).astype(np.float64), rng.uniform(-0.5, 0.5, (B, 3)))
    f = np.concatenate([rng.uniform(-1, 1, (B, n, 2)), rng.uniform(0, 4, (B, n, 1))], 2)
    counters = np.array([COUNTERS[b % len(COUNTERS)] for b in range(B)], dtype=np.int32)
    return RPCase(n, B, s.block(), f, counters, p.ml, p.Jl, np.ascontiguousarray(p.r.T))


@functools.lru_cache(maxsize=None)
def rp_reference(seed=3000, steps=STEPS) -> State:
    c = rp_case(seed)
    p, s = c.params(), c.state()
    for _ in range(steps):
        rp_step(p, s, c.f, DT)
    return s
