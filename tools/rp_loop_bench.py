"""Timing of the rigid payload's closed loop (profiles/tracking.md): the reference's 2,000-step loop of
test/control/test_rpcentralized.py:main resident on the device (rigid_payload.RPClosedLoop: k_cent + k_rp_advance per
step) against the same loop driven step by step from Python (RPCentralizedController.control + RPDynamics.integrate
with the law in numpy: three host round trips per step), and the resident loop's time per step at a large batch.

    python tools/rp_loop_bench.py resident | stepwise | batch [B]

Each mode prints one JSON line.  `stepwise` needs nothing of the tracking feature, so it also runs on an older build
of the library (DAT_LIB_PATH)."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])

STEPS, DT = 2000, 1e-2


def resident():
    from distributed_aerial_transportation_amd import rigid_payload as rp

    p, _, s0 = rp.rp_setup(3)
    rp.RPClosedLoop(p, s0, DT).run(10)  # (module load, first launches)
    loop = rp.RPClosedLoop(p, s0, DT)
    t0 = time.perf_counter()
    loop.run(STEPS)
    x = loop.state.xl
    t1 = time.perf_counter()
    return {"mode": "resident", "steps": STEPS, "wall_s": t1 - t0, "xl": x.tolist()}


def stepwise():
    from distributed_aerial_transportation_amd import rigid_payload as rp

    p, col, s0 = rp.rp_setup(3)
    ctl = rp.RPCentralizedController(p, col, s0, DT)
    dyn = rp.RPDynamics(p, s0, DT)
    rad, hgt, fr = 1.0, 1.0, 0.5

    def step(k):
        t = k * DT
        s = dyn.state
        x_ref = np.array([rad * np.cos(fr * t), rad * np.sin(fr * t), hgt])
        v_ref = np.array([-rad * fr * np.sin(fr * t), rad * fr * np.cos(fr * t), 0.0])
        a_ref = np.array([-rad * fr ** 2 * np.cos(fr * t), -rad * fr ** 2 * np.sin(fr * t), 0.0])
        acc = (a_ref - (s.vl - v_ref) - (s.xl - x_ref), np.array([np.sin(t), np.cos(t), np.pi / 12]))
        dyn.integrate(ctl.control(s, acc))

    t0 = time.perf_counter()
    for k in range(STEPS):
        step(k)
    x = dyn.state.xl
    t1 = time.perf_counter()
    return {"mode": "stepwise", "steps": STEPS, "wall_s": t1 - t0, "xl": x.tolist()}


def batch(B):
    from distributed_aerial_transportation_amd import rigid_payload as rp
    from distributed_aerial_transportation_amd import tracking

    p, _, s0 = rp.rp_setup(3)
    rng = np.random.default_rng(0)
    rec = np.stack([tracking.circle_record(t0=t) for t in rng.uniform(0.0, 12.0, B)])
    loop = rp.RPClosedLoop(p, [s0] * B, DT, track=rec)
    loop.run(20)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        loop.run(100)
        times.append((time.perf_counter() - t0) / 100)
    return {"mode": "batch", "B": B, "n": 3, "ms_per_step": [1e3 * t for t in times]}


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "resident"
    out = {"resident": resident, "stepwise": stepwise}[mode]() if mode != "batch" else batch(
        int(sys.argv[2]) if len(sys.argv) > 2 else 65536)
    print(json.dumps(out))
