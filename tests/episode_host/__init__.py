"""ctypes loader for the TEST-ONLY host build of the episode rule (see episode_host.hip)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libdat_episode_host.so")
SRC = os.path.join(HERE, "episode_host.hip")
ROOT = os.path.dirname(os.path.dirname(HERE))
CORE = os.path.join(ROOT, "distributed_aerial_transportation_amd", "csrc")


class Rules(ctypes.Structure):
    """dat_episode_rules (include/dat.h)"""

    _fields_ = [("goal_x", ctypes.c_double), ("bound", ctypes.c_double), ("max_steps", ctypes.c_int),
                ("stall_steps", ctypes.c_int), ("on_collision", ctypes.c_int), ("wrap", ctypes.c_int)]


def build(force=False):
    deps = [SRC, os.path.join(ROOT, "include", "dat.h")] + [os.path.join(CORE, f) for f in
                                                           ("dat_episode.hpp", "dat_core.hpp", "dat_layout.h")]
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        # the library's floating-point rule (_lib.HIPFLAGS): contraction within a source expression only
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on",
                               "--offload-arch=gfx950", SRC, "-o", LIB])
    return LIB


_lib = None
D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
    return _lib


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def steps(rules, max_iter, xl, vl, iters, col, mind):
    """rules: K dicts (goal_x, bound, max_steps, stall_steps, on_collision); xl, vl (K, T, 3); iters, col, mind
    (K, T): K episodes of T control steps from fresh accumulators.  Returns reason (K, T), acc (K, T, 5) =
    (steps, iter_sum, iter_max, full_steps, stall_run) and the smallest distance (K, T) after every step."""
    xl, vl, mind = _f(xl), _f(vl), _f(mind)
    iters, col = _i(iters), _i(col)
    K, T = iters.shape
    assert lib().eh_acc_ints() == 12
    arr = (Rules * K)()
    for k, r in enumerate(rules):
        arr[k] = Rules(float(r["goal_x"]), float(r["bound"]), int(r["max_steps"]), int(r["stall_steps"]),
                       int(r["on_collision"]), 1)
    reason = np.zeros((K, T), dtype=np.int32)
    acc = np.zeros((K, T, 5), dtype=np.int32)
    md = np.zeros((K, T))
    lib().eh_steps(arr, int(max_iter), K, T, xl.ctypes.data_as(D), vl.ctypes.data_as(D), iters.ctypes.data_as(I),
                   col.ctypes.data_as(I), mind.ctypes.data_as(D), reason.ctypes.data_as(I), acc.ctypes.data_as(I),
                   md.ctypes.data_as(D))
    return reason, acc, md


def records(s, j, B, P, wrap):
    """(record, idle) of slot s[k]'s j[k]-th episode in a batch of B and a pool of P"""
    s, j = _i(s), _i(j)
    rec = np.zeros(s.shape[0], dtype=np.int32)
    idle = np.zeros(s.shape[0], dtype=np.int32)
    lib().eh_records(s.ctypes.data_as(I), j.ctypes.data_as(I), s.shape[0], int(B), int(P), int(bool(wrap)),
                     rec.ctypes.data_as(I), idle.ctypes.data_as(I))
    return rec, idle.astype(bool)
