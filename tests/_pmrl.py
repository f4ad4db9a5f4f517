"""The point-mass rigid-link fixture (tests/golden/ref_pmrl.npz, written by make_pmrl.py) as the blocks the
host build and the device take, shared by test_pmrl_host.py and test_gpu_pmrl.py."""
import functools

import numpy as np

from tests._golden import load

CASES = ((3, 23), (6, 11), (7, 10), (16, 5))
# The fixture's own margin: its generator reruns every case with LU in place of the reference's Cholesky and
# asserts that no stored state moves by more than 1e-12; it measured <= 9e-16 (45 steps) and 7.4e-15 (400 steps).
TOL_STATE = 1e-10   # absolute, every stored state
TOL_ACC = 1e-11     # of max(1, |.|_inf), the accelerations and tensions


class Case:
    """one (n, B) case: prm (B, P), x0 (B, S), c0 (B,), f (nf, B, 3, n), and the reference's records"""

    def __init__(self, d, n, B):
        from distributed_aerial_transportation_amd import pmrl

        self.n, self.B, self.d = n, B, d
        self.dt, self.steps = float(d["dt"]), int(d["steps"])
        self.keep, self.acc_at = [int(k) for k in d["keep"]], [int(k) for k in d["acc_at"]]
        g = lambda k: d[f"c{n}_{k}"]  # noqa: E731
        self.g = g
        self.f = g("f")
        self.nf = self.f.shape[0]
        self.params = [pmrl.PMRLParameters(g("m")[b], float(d["ml"]), d["Jl"], g("r")[b], g("L")[b]) for b in range(B)]
        self.prm = np.stack([pmrl.pack_pmrl_params(p) for p in self.params])
        self.s0 = [pmrl.PMRLState(g("q")[b], g("dq")[b], g("xl")[b], g("vl")[b], g("Rl")[b], g("wl")[b])
                   for b in range(B)]
        self.x0 = np.stack([pmrl.pack_pmrl_state(s) for s in self.s0])
        self.c0 = g("counter").astype(np.int32)

    def ref_state(self, j, b):
        """the reference's state after step keep[j] of scenario b"""
        from distributed_aerial_transportation_amd import pmrl

        g = self.g
        return pmrl.PMRLState(g("s_q")[j, b], g("s_dq")[j, b], g("s_xl")[j, b], g("s_vl")[j, b], g("s_Rl")[j, b],
                              g("s_wl")[j, b], project=False)

    def ref_block(self, j):
        """... of every scenario, as state blocks (B, S), and the counters"""
        from distributed_aerial_transportation_amd import pmrl

        return (np.stack([pmrl.pack_pmrl_state(self.ref_state(j, b)) for b in range(self.B)]),
                self.g("s_counter")[j].astype(np.int32))

    def acc_state(self, j, b):
        """the state the reference's accelerations acc_at[j] were taken at: the start, or a kept state"""
        k = self.acc_at[j]
        return self.s0[b] if k == 0 else self.ref_state(self.keep.index(k), b)

    def acc_force(self, j):
        """the force set of step acc_at[j], (B, 3, n)"""
        return self.f[self.acc_at[j] // (self.steps // self.nf)]


@functools.lru_cache(maxsize=None)
def case(n):
    d = load("ref_pmrl.npz")
    B = dict(CASES)[n]
    return Case(d, n, B)


def rel(a, b):
    """|a - b|_inf / max(1, |b|_inf)"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, float(np.max(np.abs(b)))))


def check_acc(tag, got, c, j, b):
    """accelerations and tensions ((ddq, dvl, dwl), T) of scenario b against the reference's record acc_at[j]"""
    (ddq, dvl, dwl), T = got
    g = c.g
    for name, x, ref in (("ddq", ddq, g("a_ddq")[j, b]), ("dvl", dvl, g("a_dvl")[j, b]), ("dwl", dwl, g("a_dwl")[j, b]),
                         ("T", T, g("a_T")[j, b])):
        e = rel(x, ref)
        assert e <= TOL_ACC, (tag, c.n, b, c.acc_at[j], name, e)


def recipe():
    """the reference's own n = 3 recipe: (params, start state, dt, forces (steps, 3, 3), every, kept states)"""
    from distributed_aerial_transportation_amd import pmrl

    d = load("ref_pmrl.npz")
    p = pmrl.PMRLParameters(d["rec_m"], float(d["ml"]), d["Jl"], d["rec_r"], d["rec_L"])
    q0 = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, 3))
    s0 = pmrl.PMRLState(q0, np.zeros((3, 3)), np.zeros(3), np.zeros(3), np.eye(3), np.zeros(3))
    f = np.repeat(d["rec_f"][:, :, None], 3, axis=2)
    kept = [pmrl.PMRLState(d["rec_q"][k], d["rec_dq"][k], d["rec_xl"][k], d["rec_vl"][k], d["rec_Rl"][k],
                           d["rec_wl"][k], project=False) for k in range(d["rec_q"].shape[0])]
    return p, s0, float(d["dt"]), f, int(d["rec_every"]), kept
