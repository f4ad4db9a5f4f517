"""Episodes in the resident loop, measured (profiles/episodes.md): bench.py's C4 workload (n = 6 C-ADMM, seeded forests,
path start, one sub-batch) on one GPU.

1. overhead: `--steps` HL steps from the same checkpoint with episodes closed and with episodes open under rules that
   never fire (the kernels with the episode flag run, nothing ends), alternating, `--rounds` rounds in one process;
   the overhead in multiples of the closed runs' spread (max - min), and the two end states compared bitwise.
2. the long loop: `--long-steps` HL steps from the start states, plain and with stall_steps / on_collision episodes
   (pool: the start states' own checkpoint, wrap), per block of `--block` steps the ms per step and the episodes
   ended per reason.

    python tools/episode_bench.py --batch 65536 --out episodes.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(eng, steps):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.closed_loop(steps)
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    import bench
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--n", type=int, default=6)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--long-steps", type=int, default=1000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--stall-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, B = args.n, args.batch
    sf, st, forests = bench.bench_states(n, B, 0, 1, 64, "path", None)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    res = {"batch": B, "n": n, "steps": args.steps, "rounds": args.rounds}
    try:
        eng.set_forests(forests, sf)
        eng.set_state(st, np.zeros(B, dtype=np.int32))
        start = eng.checkpoint()
        eng.closed_loop(args.warmup)
        ck = eng.checkpoint()
        # ---- 1: the overhead of open episodes that never fire
        closed, opened, same = [], [], True
        for _ in range(args.rounds):
            eng.restore(ck)
            closed.append(timed(eng, args.steps))
            ref = eng.get_state()[0]
            eng.episodes_begin(ck, on_collision=False)  # (loads record s into slot s: the same start)
            opened.append(timed(eng, args.steps))
            assert eng.episodes_counts()["ended"]["total"] == 0
            eng.episodes_end()
            same = same and np.array_equal(ref, eng.get_state()[0])
        spread = max(closed) - min(closed)
        over = float(np.mean(opened) - np.mean(closed))
        res["overhead"] = {"closed_ms_per_step": closed, "open_ms_per_step": opened, "closed_spread_ms": spread,
                           "overhead_ms": over, "overhead_in_spreads": over / spread if spread > 0 else None,
                           "end_states_equal": bool(same)}
        print(json.dumps(res["overhead"]), flush=True)
        # ---- 2: the long loop, plain and with episodes
        rows = {}
        for name in ("plain", "episodes"):
            eng.restore(start)
            if name == "episodes":
                eng.episodes_begin(start, stall_steps=args.stall_steps, on_collision=True,
                                   capacity=min(4 * B, 1 << 22))
            blocks, prev = [], None
            for b0 in range(0, args.long_steps, args.block):
                k = min(args.block, args.long_steps - b0)
                eng.reset_counters()
                row = {"hl_steps": f"{b0}-{b0 + k - 1}", "ms_per_step": timed(eng, k)}
                w = eng.work()
                row["collisions"], row["tail_routed"] = int(w.get("collisions", 0)), int(w.get("tail_routed", 0))
                if name == "episodes":
                    c = eng.episodes_counts()
                    row["ended"] = {r: v - (prev["ended"][r] if prev else 0) for r, v in c["ended"].items()}
                    row["lost"] = c["lost"]
                    prev = c
                    eng.episodes_clear()
                blocks.append(row)
                print(name, json.dumps(row), flush=True)
            if name == "episodes":
                eng.episodes_end()
            rows[name] = blocks
        res["long"] = rows
    finally:
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
