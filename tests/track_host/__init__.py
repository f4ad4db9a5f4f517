"""ctypes loader for the TEST-ONLY host build of the trajectory-tracking law (see track_host.hip)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libdat_track_host.so")
SRC = os.path.join(HERE, "track_host.hip")
CORE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "distributed_aerial_transportation_amd", "csrc")


def build(force=False):
    deps = [SRC] + [os.path.join(CORE, f) for f in ("dat_track.hpp", "dat_core.hpp", "dat_layout.h")]
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        # the library's floating-point rule (_lib.HIPFLAGS): contraction within a source expression only
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on",
                               "--offload-arch=gfx950", SRC, "-o", LIB])
    return LIB


_lib = None
D = ctypes.POINTER(ctypes.c_double)
Q = ctypes.POINTER(ctypes.c_longlong)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
    return _lib


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(D)


def _ticks(tick, count):
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(tick, dtype=np.int64), (count,)))
    return t, t.ctypes.data_as(Q)


def references(rec, tick, dt):
    """(x_ref, v_ref, a_ref), (K, 3) each, of records (K, TRACK_SIZE) at the simulation steps tick (K,)"""
    rec = _f(np.atleast_2d(rec))
    K = rec.shape[0]
    t, tp = _ticks(tick, K)
    xr, vr, ar = np.zeros((K, 3)), np.zeros((K, 3)), np.zeros((K, 3))
    lib().th_references(_p(rec), tp, ctypes.c_double(dt), K, _p(xr), _p(vr), _p(ar))
    return xr, vr, ar


def desired(states, n, rec, tick, dt):
    """acc (K, 6) of the state blocks states (K, 12n + 18) under records (K, TRACK_SIZE) at the steps tick (K,)"""
    st = _f(np.atleast_2d(states))
    K, S = st.shape
    rec = _f(np.broadcast_to(np.atleast_2d(rec), (K, np.atleast_2d(rec).shape[1])))
    t, tp = _ticks(tick, K)
    acc = np.zeros((K, 6))
    lib().th_desired(_p(st), int(n), int(S), _p(rec), tp, ctypes.c_double(dt), K, _p(acc))
    return acc


def desired_forest(states, n, mountain, x_offset=1.5):
    st = _f(np.atleast_2d(states))
    K, S = st.shape
    m = _f(mountain)
    acc = np.zeros((K, 6))
    lib().th_desired_forest(_p(st), int(n), int(S), _p(m), ctypes.c_double(x_offset), K, _p(acc))
    return acc


def bad_field(rec):
    return int(lib().th_bad_field(_p(_f(rec))))
