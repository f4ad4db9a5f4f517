#!/usr/bin/env python
"""Time of the point-mass rigid-link rollout (dat_pmrl_rollout, k_pmrl_rollout) against the quadrotor-payload
rollout (dat_rollout, k_rollout_agents: the kernel whose lane mapping it shares) at the same shape, by default
10 steps, n = 6, B = 65,536, in one process.  Run on a GPU machine:

    python tools/pmrl_bench.py [--n 6] [--batch 65536] [--steps 10] [--reps 7] [--write profiles/pmrl_rollout.md]

Both entry points are synchronous calls on the handle's own stream, so a call is timed whole, between two HIP events
recorded around it (the second after the call's stream synchronise).  dat_pmrl_rollout's call carries the upload of
its force set (B x 3n doubles), dat_rollout's (f_des = NULL) carries none: beside the whole calls the tool therefore
gives the kernels' own time for `steps` steps as the difference between a call of 11 x steps and a call of steps
steps, over 10 -- uploads, launch and synchronise cancel.  Medians over --reps repetitions after one warm-up of each
shape; the two entry points alternate.  Prints one JSON line; --write replaces the "Timing" section of the profile
note with the figures (the resource report above it stays).
"""

import argparse
import ctypes
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Events:
    def __init__(self):
        self.hip = hip = ctypes.CDLL("libamdhip64.so")
        vp = ctypes.c_void_p
        hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
        hip.hipEventRecord.argtypes = [vp, vp]
        hip.hipEventSynchronize.argtypes = [vp]
        hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
        self.e0, self.e1 = vp(), vp()
        self.ok(hip.hipEventCreate(ctypes.byref(self.e0)))
        self.ok(hip.hipEventCreate(ctypes.byref(self.e1)))

    @staticmethod
    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def ms(self, call):
        """device-clock time [ms] from before `call` to after its return (the call ends in a stream synchronise)"""
        hip = self.hip
        self.ok(hip.hipEventRecord(self.e0, None))
        self.ok(hip.hipEventSynchronize(self.e0))
        call()
        self.ok(hip.hipEventRecord(self.e1, None))
        self.ok(hip.hipEventSynchronize(self.e1))
        out = ctypes.c_float()
        self.ok(hip.hipEventElapsedTime(ctypes.byref(out), self.e0, self.e1))
        return float(out.value)


def pmrl_engine(n, B, dt, rng):
    from distributed_aerial_transportation_amd import pmrl
    from distributed_aerial_transportation_amd.control import BatchedController

    th = 2 * np.pi * np.arange(n) / n
    r = np.stack([0.5 * np.cos(th), 0.35 * np.sin(th), np.zeros(n)])
    p = pmrl.PMRLParameters(np.full(n, 0.5), 0.225, np.diag([2.1, 1.87, 3.97]) * 1e-2, r, np.ones(n))
    eng = BatchedController("centralized", n, B, pmrl.pack_pmrl_params(p), dt=dt)
    q = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, n))
    x = pmrl.pack_pmrl_state(pmrl.PMRLState(q, np.zeros((3, n)), np.zeros(3), np.zeros(3), np.eye(3), np.zeros(3)))
    hover = (0.5 + 0.225 / n) * 9.80665
    f = np.zeros((B, 3, n))
    f[:, 2, :] = hover
    f += rng.uniform(-0.05, 0.05, f.shape) * hover
    return eng, np.tile(x, (B, 1)), f


def rqp_engine(n, B, dt):
    from distributed_aerial_transportation_amd import scenarios, system
    from distributed_aerial_transportation_amd.control import BatchedController

    p, col, s = scenarios.rqp_setup(n)
    prm = system.pack_params(p, col)
    eng = BatchedController("centralized", n, B, prm, dt=dt)
    feq = prm[system.L.p_off("FEQ", n): system.L.p_off("FEQ", n) + 3 * n].reshape(n, 3).T
    return eng, np.tile(system.pack_state(s), (B, 1)), np.tile(feq[None], (B, 1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--write", default=None, help="profile note whose Timing section to replace")
    a = ap.parse_args()
    n, B, K, dt = a.n, a.batch, a.steps, 5e-3

    from distributed_aerial_transportation_amd import _lib as L

    pm, pm_x, pm_f = pmrl_engine(n, B, dt, np.random.default_rng(0))
    rq, rq_x, rq_f = rqp_engine(n, B, dt)
    ev = Events()
    zeros = np.zeros(B, dtype=np.int32)
    rq.rollout(1, rq_f)  # f_des on the device; the timed calls pass NULL

    def run_pmrl(steps):
        pm.set_state(pm_x, zeros)
        return ev.ms(lambda: pm.pmrl_rollout(steps, pm_f))

    def run_rqp(steps):
        rq.set_state(rq_x, zeros)
        return ev.ms(lambda: rq.rollout(steps))

    for steps in (K, 11 * K):  # warm-up of every timed shape
        run_pmrl(steps)
        run_rqp(steps)
    t = {"pmrl": {K: [], 11 * K: []}, "rollout": {K: [], 11 * K: []}}
    for _ in range(a.reps):
        for steps in (K, 11 * K):
            t["pmrl"][steps].append(run_pmrl(steps))
            t["rollout"][steps].append(run_rqp(steps))
    med = {k: {s: statistics.median(v) for s, v in d.items()} for k, d in t.items()}
    name = "unknown"
    try:
        import torch

        name = torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName
    except Exception:  # noqa: BLE001 -- the name is a label only
        pass
    out = {
        "device": name, "n": n, "batch": B, "steps": K, "dt": dt, "reps": a.reps,
        "pmrl_call_ms": med["pmrl"][K], "rollout_call_ms": med["rollout"][K],
        "pmrl_kernel_ms": (med["pmrl"][11 * K] - med["pmrl"][K]) / 10.0,
        "rollout_kernel_ms": (med["rollout"][11 * K] - med["rollout"][K]) / 10.0,
        "pmrl_call_ms_all": t["pmrl"][K], "rollout_call_ms_all": t["rollout"][K],
        "lib": os.path.basename(L.LIB_PATH),
    }
    print(json.dumps(out))
    if a.write:
        sec = (
            "## Timing\n\n"
            f"Measured by `tools/pmrl_bench.py` on {name}: {K} steps, n = {n}, B = {B:,}, dt = {dt}, medians of "
            f"{a.reps} repetitions after a warm-up, both entry points alternating in one process.\n\n"
            "| | whole call [ms] | kernel, " + f"{K} steps [ms] |\n|---|---|---|\n"
            f"| `dat_pmrl_rollout` (uploads its force set, B x 3n doubles) | {out['pmrl_call_ms']:.3f} | "
            f"{out['pmrl_kernel_ms']:.3f} |\n"
            f"| `dat_rollout` (f_des already on the device), the yardstick | {out['rollout_call_ms']:.3f} | "
            f"{out['rollout_kernel_ms']:.3f} |\n\n"
            f"Whole call: HIP events around the synchronous call.  Kernel: (call of {11 * K} steps - call of {K} "
            "steps) / 10, in which upload, launch and synchronise cancel.  Spread of the whole calls: "
            f"pmrl {min(t['pmrl'][K]):.3f} - {max(t['pmrl'][K]):.3f} ms, rollout {min(t['rollout'][K]):.3f} - "
            f"{max(t['rollout'][K]):.3f} ms.\n"
        )
        path = a.write if os.path.isabs(a.write) else os.path.join(ROOT, a.write)
        src = open(path).read() if os.path.exists(path) else "# k_pmrl_rollout\n\n"
        src = re.sub(r"## Timing\n.*?(?=\n## |\Z)", lambda m: sec, src, flags=re.S) if "## Timing\n" in src else src + "\n" + sec
        with open(path, "w") as fh:
            fh.write(src)
    pm.close()
    rq.close()


if __name__ == "__main__":
    main()
