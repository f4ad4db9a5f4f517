"""Fixture of the point-mass rigid-link system: runs the reference's own PMRLDynamics
(system/point_mass_rigid_link.py) behind the stubs of ``refstubs.py`` and writes ``ref_pmrl.npz``.

    python tests/golden/make_pmrl.py            (DAT_REFERENCE: the reference checkout, as make_golden.py's REF)

Cases (n, B): (3, 23), (6, 11), (7, 10), (16, 5) -- at one lane per link and floor(64/n) scenarios per 64-lane
block: one idle lane with two blocks, four idle lanes with a partial second block, one idle lane with a partial
second block, a full wavefront with a partial second block.  Per scenario, seeded: m in [0.3, 0.8], L in [0.7, 1.3],
r on an ellipse (scenario 0 of n = 3: the reference's own r), ml and Jl the reference's; q tilted <= 0.3 rad from e3,
|dq|, |vl|, |wl| <= 0.5; the projection counter starts at b % 20, so the polar projections of a wavefront's scenarios
fall on different steps.  Run: dt = 5e-3, 45 steps under a 9-set force schedule around hover, each set held 5 steps.

Stored per case (prefix c<n>_): the parameters, the initial states and counters, the schedule f (9, B, 3, n); the
states and counters after steps 1, 20, 21, 40, 45; (ddq, dvl, dwl, T) and the reference's own
inverse_dynamics_error at steps 0 and 40 (the states before step 0 and after step 40, under the set of that step).
And the first 400 steps of the reference's own n = 3 recipe (test/system/test_pmrldynamics.py:9-49, a new force at
every step): its parameters, the force of every step (the same for the three robots) and the states every 100 steps.

Sensitivity guard: every case is run again with the module's ``solve`` replaced by ``np.linalg.solve`` (LU, not
Cholesky); no stored state may move by more than 1e-12, so the bounds the tests hold the device to (1e-10) stand
well above what the order of the reference's own arithmetic decides.  A case that fails gets gentler inputs, never
a looser bound.
"""

from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DAT_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import refstubs  # noqa: E402

refstubs.install()
for _name in ("matplotlib", "matplotlib.pyplot"):  # the recipe's module imports it for its plot only
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "test", "system"))

import system.point_mass_rigid_link as pmrl  # noqa: E402
import test_pmrldynamics as recipe  # noqa: E402

from oracle.model import exp3  # noqa: E402

CASES = ((3, 23), (6, 11), (7, 10), (16, 5))
DT, STEPS, NF = 5e-3, 45, 9
KEEP = (1, 20, 21, 40, 45)
ACC_AT = (0, 40)
ML, JL = 0.225, np.diag([2.1, 1.87, 3.97]) * 1e-2
G = 9.80665
GUARD = 1e-12


def _ball(rng, radius):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v) * radius * rng.uniform(0.2, 1.0)


def inputs(n, B, seed):
    rng = np.random.default_rng(seed)
    d = dict(m=np.empty((B, n)), L=np.empty((B, n)), r=np.empty((B, 3, n)), q=np.empty((B, 3, n)),
             dq=np.empty((B, 3, n)), xl=np.empty((B, 3)), vl=np.empty((B, 3)), Rl=np.empty((B, 3, 3)),
             wl=np.empty((B, 3)), counter=(np.arange(B) % 20).astype(np.int32), f=np.empty((NF, B, 3, n)))
    for b in range(B):
        d["m"][b] = rng.uniform(0.3, 0.8, n)
        d["L"][b] = rng.uniform(0.7, 1.3, n)
        th = 2 * np.pi * (np.arange(n) + rng.uniform(-0.2, 0.2, n)) / n
        d["r"][b] = np.stack([0.5 * np.cos(th), 0.35 * np.sin(th), np.zeros(n)])
        tilt, az = rng.uniform(0, 0.3, n), rng.uniform(0, 2 * np.pi, n)
        d["q"][b] = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)])
        d["dq"][b] = np.stack([_ball(rng, 0.5) for _ in range(n)], axis=1)
        d["xl"][b] = rng.uniform(-1, 1, 3)
        d["vl"][b] = _ball(rng, 0.5)
        d["Rl"][b] = exp3(_ball(rng, 0.3))
        d["wl"][b] = _ball(rng, 0.5)
        hover = (d["m"][b] + ML / n) * G
        for k in range(NF):
            d["f"][k, b] = np.stack([np.zeros(n), np.zeros(n), hover]) + rng.uniform(-0.15, 0.15, (3, n)) * hover
    # inputs on a grid of 2^-12 (Rl apart, a rotation): the file compresses, and the reference projects q and dq itself
    for k in d:
        if k not in ("Rl", "counter"):
            d[k] = np.round(d[k] * 4096.0) / 4096.0
    if n == 3:
        d["r"][0] = recipe._pmrl_nrobot_parameters(3).r
    return d


def run_case(n, B, d):
    """the reference over the case: states after KEEP, accelerations at ACC_AT"""
    out = dict(s_q=np.empty((len(KEEP), B, 3, n)), s_dq=np.empty((len(KEEP), B, 3, n)), s_xl=np.empty((len(KEEP), B, 3)),
               s_vl=np.empty((len(KEEP), B, 3)), s_Rl=np.empty((len(KEEP), B, 3, 3)), s_wl=np.empty((len(KEEP), B, 3)),
               s_counter=np.empty((len(KEEP), B), dtype=np.int32), a_ddq=np.empty((len(ACC_AT), B, 3, n)),
               a_dvl=np.empty((len(ACC_AT), B, 3)), a_dwl=np.empty((len(ACC_AT), B, 3)),
               a_T=np.empty((len(ACC_AT), B, n)), a_err=np.empty((len(ACC_AT), B)))
    for b in range(B):
        p = pmrl.PMRLParameters(d["m"][b].copy(), ML, JL.copy(), d["r"][b].copy(), d["L"][b].copy())
        s = pmrl.PMRLState(d["q"][b].copy(), d["dq"][b].copy(), d["xl"][b].copy(), d["vl"][b].copy(),
                           d["Rl"][b].copy(), d["wl"][b].copy())
        s._counter = int(d["counter"][b])
        dyn = pmrl.PMRLDynamics(p, s, DT)
        for k in range(STEPS):
            f = d["f"][k // (STEPS // NF), b]
            if k in ACC_AT:
                j = ACC_AT.index(k)
                (ddq, dvl, dwl), T = dyn.forward_dynamics(f.copy())
                out["a_ddq"][j, b], out["a_dvl"][j, b], out["a_dwl"][j, b], out["a_T"][j, b] = ddq, dvl, dwl, T
                out["a_err"][j, b] = pmrl.PMRLDynamics.inverse_dynamics_error(dyn.state, p, f, T, (ddq, dvl, dwl))
            dyn.integrate(f.copy())
            if k + 1 in KEEP:
                j, st = KEEP.index(k + 1), dyn.state
                out["s_q"][j, b], out["s_dq"][j, b], out["s_xl"][j, b] = st.q, st.dq, st.xl
                out["s_vl"][j, b], out["s_Rl"][j, b], out["s_wl"][j, b] = st.vl, st.Rl, st.wl
                out["s_counter"][j, b] = st._counter
    return out


def run_recipe(steps=400, every=100):
    n = 3
    p = recipe._pmrl_nrobot_parameters(n)
    dyn = pmrl.PMRLDynamics(p, recipe._pmrl_nrobots_init_state(n), DT)
    t_seq = np.arange(0, 10, DT)
    f_seq = np.empty((steps, 3))
    keep = {k: [] for k in ("q", "dq", "xl", "vl", "Rl", "wl")}
    for i in range(steps):
        f = recipe._pmrl_nrobot_force_trajectory(p, t_seq[i], n)
        assert np.array_equal(f, np.tile(f[:, :1], (1, n)))
        f_seq[i] = f[:, 0]
        dyn.integrate(f)
        if (i + 1) % every == 0:
            for k in keep:
                keep[k].append(np.array(getattr(dyn.state, k)))
    out = {"rec_" + k: np.stack(v) for k, v in keep.items()}
    out.update(rec_f=f_seq, rec_m=p.m, rec_L=p.L, rec_r=p.r, rec_every=np.int32(every))
    return out


def _lu_solve(a, b, **kw):
    return np.linalg.solve(a, b)


def main():
    data = dict(dt=DT, steps=np.int32(STEPS), keep=np.array(KEEP, dtype=np.int32), acc_at=np.array(ACC_AT, dtype=np.int32),
                ml=ML, Jl=JL, cases=np.array(CASES, dtype=np.int32))
    chol_solve = pmrl.solve
    for n, B in CASES:
        d = inputs(n, B, 1000 + n)
        out = run_case(n, B, d)
        pmrl.solve = _lu_solve
        try:
            alt = run_case(n, B, d)
        finally:
            pmrl.solve = chol_solve
        moved = max(float(np.max(np.abs(out[k] - alt[k]))) for k in out if k.startswith("s_") and k != "s_counter")
        spread = max(float(np.max(np.abs(out[k] - alt[k]))) for k in ("a_ddq", "a_dvl", "a_dwl", "a_T"))
        print(f"n = {n:2d}, B = {B:2d}: LU against Cholesky moves the states by {moved:.2e}, the accelerations and "
              f"tensions by {spread:.2e}; the reference's dynamics error <= {out['a_err'].max():.2e}; "
              f"|state| <= {max(float(np.max(np.abs(out[k]))) for k in out if k.startswith('s_') and k != 's_counter'):.2f}")
        assert moved <= GUARD, (n, B, moved)
        for k, v in d.items():
            data[f"c{n}_{k}"] = v
        for k, v in out.items():
            data[f"c{n}_{k}"] = v
    rec = run_recipe()
    pmrl.solve = _lu_solve
    try:
        alt = run_recipe()
    finally:
        pmrl.solve = chol_solve
    moved = max(float(np.max(np.abs(rec[k] - alt[k]))) for k in rec)
    print(f"n = 3 recipe, 400 steps: LU against Cholesky moves the states by {moved:.2e}")
    assert moved <= GUARD, moved
    data.update(rec)
    path = os.path.join(HERE, "ref_pmrl.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
