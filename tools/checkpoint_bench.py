#!/usr/bin/env python
"""Save and restore time of a checkpoint (BatchedController.checkpoint / restore) of one batch, by default the C4
batch (65,536 scenarios, C-ADMM, n = 6), against a plain device-to-device hipMemcpyAsync of the same byte count and
against the call's own copy between the staging buffer and the host blob (dat_get_checkpoint_ms).  Prints one JSON
line.  Run on a GPU machine:

    python tools/checkpoint_bench.py [--mode cadmm] [--n 6] [--batch 65536] [--reps 5]
"""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def d2d_memcpy_ms(nbytes, reps):
    """device time [ms] of hipMemcpyAsync(device -> device) of nbytes, per repetition (after one warm-up)"""
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipMemsetAsync.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, vp]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipFree.argtypes = [vp]

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(ctypes.byref(src), nbytes))
    ok(hip.hipMalloc(ctypes.byref(dst), nbytes))
    ok(hip.hipMemsetAsync(src, 1, nbytes, None))
    ok(hip.hipEventCreate(ctypes.byref(e0)))
    ok(hip.hipEventCreate(ctypes.byref(e1)))
    out = []
    for _ in range(reps + 1):
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, None))  # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = ctypes.c_float()
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        out.append(ms.value)
    hip.hipFree(src)
    hip.hipFree(dst)
    return out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="cadmm")
    ap.add_argument("--n", type=int, default=6)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    B, n = a.batch, a.n
    eng = BatchedController(a.mode, n, B, scenarios.params_block(n))
    eng.set_state(scenarios.perturbed_states(n, B, np.random.default_rng(0)), np.zeros(B, dtype=np.int32))
    eng.closed_loop(1)
    perm = np.random.default_rng(1).permutation(B).astype(np.int32)

    def timed(call):
        rows = []
        for _ in range(a.reps + 1):  # (the first call grows the staging buffer)
            t = time.perf_counter()
            r = call()
            wall = (time.perf_counter() - t) * 1e3
            rows.append((wall,) + eng.checkpoint_ms())
        return r, [min(x[k] for x in rows[1:]) for k in range(3)]

    ck, save = timed(lambda: eng.checkpoint())
    _, save_perm = timed(lambda: eng.checkpoint(perm))
    _, load = timed(lambda: eng.restore(ck))
    _, load_perm = timed(lambda: eng.restore(ck, records=perm))
    one = ck.select([0])
    _, fork = timed(lambda: eng.restore(one, records=np.zeros(B, dtype=np.int32)))
    nbytes = len(ck.tobytes()) - 64
    d2d = min(d2d_memcpy_ms(nbytes, a.reps))
    blob = np.frombuffer(ck.tobytes(), dtype=np.uint8)
    host = []
    for _ in range(a.reps):
        t = time.perf_counter()
        blob.copy()
        host.append((time.perf_counter() - t) * 1e3)
    keys = ("wall_ms", "kernel_ms", "copy_ms")
    out = {"mode": a.mode, "n": n, "batch": B, "record_words": ck.words, "blob_bytes": nbytes + 64,
           "d2d_memcpy_ms": d2d, "d2d_memcpy_GBps": 2 * nbytes / d2d / 1e6, "host_memcpy_ms": min(host)}
    for name, row in (("save", save), ("save_permuted", save_perm), ("restore", load), ("restore_permuted", load_perm),
                      ("fork_one_into_all", fork)):
        out[name] = dict(zip(keys, (round(v, 4) for v in row)))
        out[name]["kernel_share_of_d2d"] = round(d2d / row[1], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
