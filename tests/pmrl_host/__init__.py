"""ctypes loader for the TEST-ONLY host build of the point-mass rigid-link step (see pmrl_host.hip)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libdat_pmrl_host.so")
SRC = os.path.join(HERE, "pmrl_host.hip")
CORE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "distributed_aerial_transportation_amd", "csrc")


def build(force=False):
    deps = [SRC] + [os.path.join(CORE, f) for f in ("dat_pmrl_step.hpp", "dat_core.hpp", "dat_layout.h")]
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                               SRC, "-o", LIB])
    return LIB


_lib = None
D = ctypes.POINTER(ctypes.c_double)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
    return _lib


def p(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(D)


def forward(prm, n, st, f):
    """pmrl_forward at the state block st under f (3, n): (ddq (3, n), dvl, dwl), T"""
    ddq, dvl, dwl, T = np.zeros((n, 3)), np.zeros(3), np.zeros(3), np.zeros(n)
    lib().ph_forward(p(prm), n, p(st), p(np.asarray(f, float).T), ddq.ctypes.data_as(D), dvl.ctypes.data_as(D),
                     dwl.ctypes.data_as(D), T.ctypes.data_as(D))
    return (ddq.T.copy(), dvl, dwl), T


def steps(prm, n, st, counter, f, dt, count=1):
    """`count` calls of pmrl_step under f (3, n) held: (state block, counter)"""
    st = np.array(st, dtype=np.float64)
    c = ctypes.c_int(int(counter))
    lib().ph_steps(p(prm), n, st.ctypes.data_as(D), ctypes.byref(c), p(np.asarray(f, float).T), ctypes.c_double(dt),
                   int(count))
    return st, c.value


def system(prm, n, st, f):
    """the reduced 6 x 6 system at the state: (S (6, 6), G y (6))"""
    S, Gy = np.zeros(21), np.zeros(6)
    lib().ph_system(p(prm), n, p(st), p(np.asarray(f, float).T), S.ctypes.data_as(D), Gy.ctypes.data_as(D))
    full = np.zeros((6, 6))
    full[np.triu_indices(6)] = S
    return full + np.triu(full, 1).T, Gy
