"""The tracked closed loop in the oracle, shared by tests/golden/make_track.py (which writes ref_track.npz), by
tests/test_track_fixture.py (which replays its first steps) and by tests/test_gpu_tracking.py (which reads it).

A case is one controller of the oracle (oracle/controllers.py) flying the reference's circle
(test/control/test_rqpcontrollers.py:24-48: radius 1 m, height 1 m, 0.5 rad/s, gains 1, no clamp,
dwl_des = (sin t, cos t, pi / 12)) from the rest state without a forest, dt = 1 ms, a control step every 10 steps:
per HL step the law at t = i dt from the oracle's state, the controller, then 10 steps of the "pd" low-level law and
the oracle's dynamics (oracle/model.py).  The law is written out here, on the oracle's State, so the fixture depends
on the oracle alone."""
import numpy as np

DT, HL_EVERY = 1e-3, 10
# case: (controller, n, HL steps)
CASES = {"cadmm3": ("cadmm", 3, 40), "cadmm6": ("cadmm", 6, 20), "dd3": ("dd", 3, 40), "cent3": ("centralized", 3, 40)}
MAX_ITER = 100
REPLAY = 5  # HL steps test_track_fixture.py replays


def law(s, t):
    """(dvl_des, dwl_des) of the reference's circle at time t from the oracle state s"""
    rad, hgt, w = 1.0, 1.0, 0.5
    c, sn = np.cos(w * t), np.sin(w * t)
    x_ref = np.array([rad * c, rad * sn, hgt])
    v_ref = np.array([-rad * w * sn, rad * w * c, 0.0])
    a_ref = np.array([-rad * w ** 2 * c, -rad * w ** 2 * sn, 0.0])
    return a_ref - (s.vl - v_ref) - (s.xl - x_ref), np.array([np.sin(t), np.cos(t), np.pi / 12])


def pack(s):
    """the oracle state as a dat state block (csrc/dat_layout.h DAT_S_*)"""
    n = s.n
    return np.concatenate([np.transpose(s.R, (2, 0, 1)).reshape(-1), s.w.T.reshape(-1), s.xl, s.vl, s.Rl.reshape(-1),
                           s.wl])


def controller(kind, n):
    import oracle.controllers as oc
    from oracle import scenarios as osc

    p, r = osc.params(n), osc.col_radius(n)
    return p, {"cadmm": lambda: oc.CADMM(p, r), "dd": lambda: oc.DD(p, r, None, DT),
               "centralized": lambda: oc.Centralized(p, r)}[kind]()


def run(name, tol, steps=None):
    """The case's loop at IPM tolerance tol: dict of acc (K, 6), f_des (K, 3, n), iters (K,), err (K, MAX_ITER; NaN
    padded), state (K, 12n + 18: after each HL period), start (12n + 18)."""
    import oracle.controllers as oc
    import oracle.ipm as oi
    from oracle import model as om
    from oracle import scenarios as osc

    kind, n, K = CASES[name]
    K = K if steps is None else steps
    orig = oi.solve_qp
    oc.solve_qp = lambda *a, **k: orig(*a, **{**k, "tol": tol})
    try:
        p, ctl = controller(kind, n)
        s = osc.rest_state(n)
        out = {"start": pack(s), "acc": np.zeros((K, 6)), "f_des": np.zeros((K, 3, n)),
               "iters": np.zeros(K, dtype=np.int16), "err": np.full((K, MAX_ITER), np.nan),
               "state": np.zeros((K, 12 * n + 18))}
        for k in range(K):
            acc = law(s, (k * HL_EVERY) * DT)
            f_des, stat = ctl.control(s, acc)
            out["acc"][k] = np.concatenate(acc)
            out["f_des"][k] = f_des
            out["iters"][k] = stat.iter
            out["err"][k, : len(stat.err_seq)] = stat.err_seq
            for _ in range(HL_EVERY):
                f, M = om.low_level_control(p, s, f_des, "pd")
                dw, dvl, dwl = om.forward_dynamics(p, s, f, M)
                s.integrate(dw, dvl, dwl, DT)
            out["state"][k] = pack(s)
    finally:
        oc.solve_qp = orig
    return out


def sensitivities(r11, r10):
    """The oracle against itself, 1e-10 against 1e-11, per HL step: sens_f, the f_des change relative to the step's
    largest force component (NaN from the first step on whose pass count moves: the loops part there), count_moves,
    and state_spread, the largest state difference over the loop."""
    K = r11["iters"].shape[0]
    sf, cm = np.full(K, np.nan), np.zeros(K, dtype=bool)
    for k in range(K):
        if r11["iters"][k] != r10["iters"][k]:
            cm[k:] = True
            break
        sf[k] = float(np.max(np.abs(r10["f_des"][k] - r11["f_des"][k])) / max(1.0, np.max(np.abs(r11["f_des"][k]))))
    return sf, cm, float(np.max(np.abs(r10["state"] - r11["state"])))


class Case:
    def __init__(self, d, name):
        self.name = name
        self.kind, self.n, self.K = CASES[name]
        for k in ("start", "acc", "f_des", "iters", "err", "state", "sens_f", "count_moves", "state_spread"):
            setattr(self, k, d[f"{name}_{k}"])
