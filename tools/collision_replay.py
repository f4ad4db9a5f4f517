"""Collisions of the sustained C4 loop (bench.py sustained_loop: 65,536 scenarios, 1,000 HL steps) on the GPU:
which scenarios collide and at which step, and a fixture of the earliest ones for the oracle replay
(tests/test_collision_replay.py): each scenario's state `lead` steps before its first collision, and the GPU's own
replay from there with the warm state reset (the replay's start in the oracle as well) -- per step f_des, ADMM
iterations, min env distance and the collision flag.  The 65,536-scenario loop runs device-resident
(dat_closed_loop) with the recorder open (dat_log_*): its summary tier gives the collision flags of pass 1, its
full tier on the picked scenarios their states of pass 2; nothing is stepped from the host.

    python tools/collision_replay.py out.npz [--steps 1000] [--count 4] [--lead 3] [--after 2]   # on the GPU box
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 6
B = 65536
CHUNK = 100  # HL steps per read of the recorder


def engine(forests, sf, states):
    import bench
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    eng = BatchedController("cadmm", N, len(sf), scenarios.params_block(N))
    eng.set_qp_tolerance(1e-10)
    eng.set_forests(forests, sf)
    eng.reset_warm_start()
    eng.set_state(states, np.zeros(len(sf), dtype=np.int32))
    if len(sf) == B:
        eng.set_sub_batches(bench.auto_sub_batches(B))
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--count", type=int, default=4)
    ap.add_argument("--lead", type=int, default=3)
    ap.add_argument("--after", type=int, default=2)
    args = ap.parse_args()
    import bench

    sf, states, forests = bench.bench_states(N, B, 0, 1, 64, "path", None)
    # pass 1: the device-resident loop with the recorder's summary tier (dat_log_*), read out every CHUNK HL
    # steps: the scenarios' collision flags per step, nothing stepped from the host
    eng = engine(forests, sf, states)
    first = np.full(B, -1)
    hits = np.zeros(B, dtype=np.int64)
    t0 = time.time()
    eng.log_begin([], hl_capacity=CHUNK, summary=True)
    for k0 in range(0, args.steps, CHUNK):
        eng.closed_loop(min(CHUNK, args.steps - k0))
        col = eng.log_read()["sum_collision"]  # (HL steps of the chunk, B)
        eng.log_clear()
        new = col.any(axis=0) & (first < 0)
        first[new] = k0 + col[:, new].argmax(axis=0)
        hits += col.sum(axis=0)
        print(f"step {k0 + len(col)}: {int((first >= 0).sum())} scenarios collided so far ({time.time() - t0:.0f} s)",
              flush=True)
    eng.close()
    ids = np.flatnonzero(first >= 0)
    print(f"{len(ids)} scenarios collide ({int(hits.sum())} scenario-steps); first collisions at steps "
          f"{sorted(set(first[ids].tolist()))[:20]}", flush=True)
    if len(ids) == 0:
        np.savez_compressed(args.path, ids=ids)
        return
    pick = ids[np.argsort(first[ids], kind="stable")[:args.count]]
    s0 = first[pick] - args.lead
    # pass 2: the same loop (deterministic) up to each picked scenario's start step with the full tier open on
    # the picked scenarios, every simulation step logged: the state at HL instant k is the one after step
    # 10 k - 1, the polar-projection counter there (10 k) % 20 (it starts at 0 and wraps at 20)
    order = np.argsort(pick)
    eng = engine(forests, sf, states)
    st0 = np.zeros((len(pick), states.shape[1]))
    st0[s0 <= 0] = states[pick[s0 <= 0]]
    c0 = ((10 * np.maximum(s0, 0)) % 20).astype(np.int32)
    eng.log_begin(pick[order], log_every=1, hl_capacity=CHUNK)
    for k0 in range(0, int(s0.max()), CHUNK):
        eng.closed_loop(min(CHUNK, int(s0.max()) - k0))
        out = eng.log_read()
        eng.log_clear()
        for q in np.flatnonzero((s0 > k0) & (s0 <= k0 + len(out["f_des"]))):
            at = int(np.flatnonzero(out["step_index"] == 10 * s0[q] - 1)[0])
            st0[q] = out["state"][at, int(np.flatnonzero(order == q)[0])]
    eng.close()
    # the GPU replay from st0 with the warm state reset
    K = args.lead + 1 + args.after
    eng = engine(forests, sf[pick], st0)
    eng.set_state(st0, c0)
    f = np.zeros((K, len(pick), 3, N))
    it = np.zeros((K, len(pick)), dtype=np.int32)
    md = np.zeros((K, len(pick)))
    col = np.zeros((K, len(pick)), dtype=bool)
    for k in range(K):
        r = eng.control()
        f[k], it[k], md[k], col[k] = r.f_des, r.iters, r.min_env_dist, r.collision
        eng.rollout(10)
    eng.close()
    for q, s in enumerate(pick):
        print(f"scenario {int(s)} (forest {int(sf[s])}): first collision at step {int(first[s])}, {int(hits[s])} "
              f"collided steps; replay from step {int(s0[q])}, warm state reset: collision at replay steps "
              f"{np.flatnonzero(col[:, q]).tolist()}, min dist {md[:, q].round(6).tolist()}, iters {it[:, q].tolist()}",
              flush=True)
    np.savez_compressed(args.path, ids=pick, forest=sf[pick], first=first[pick], hits=hits[pick], s0=s0, st0=st0,
                        c0=c0, f_des=f, iters=it, min_env_dist=md, collision=col, n_collided=len(ids),
                        scenario_steps=int(hits.sum()))


if __name__ == "__main__":
    main()
