"""ctypes binding of libdat.so (the C-ABI in include/dat.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU is visible,
the controllers raise.  ``build()`` compiles the library in-tree for gfx950 with hipcc.
"""

from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
LIB_PATH = os.path.join(PKG, "libdat.so")
CSRC = os.path.join(PKG, "csrc")
# The library's translation units, compiled in parallel: every .hip under csrc/ -- the host units dat.hip (handle, step
# chain, schedules, C-ABI) and dat_h_*.hip (log, episodes, checkpoints), the kernel units dat_k_*.hip
# (csrc/dat_launch.hpp lists them), dat_cent.hip (k_cent<n>), dat_comm.hip (RCCL metric collectives) -- but the unity
# file, which is the host and kernel units as one unit for development builds (tools/build_var.sh).
UNITY = os.path.join(CSRC, "dat_unity.hip")
SRCS = tuple(sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip") and f != os.path.basename(UNITY)))
OBJ_DIR = os.path.join(PKG, "build")
# -ffp-contract=on: multiply-adds fused within a source expression only (not across statements, which
# depends on the inlining context): an inlined function computes the same bits at every call site and in
# every kernel (k_cadmm / k_cadmm_tail run the same agent-QP passes, dat_qp.hpp).  C4 A/B: k_cadmm 3.53 ->
# 3.55 ms per step.
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on"]
# what the source hash covers: every file under csrc/ (by listing it: a new header cannot be left out) and the C-ABI
DEPS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))) + [
    os.path.join(REPO, "include", "dat.h")]

MODE_CENTRALIZED, MODE_CADMM, MODE_DD = 0, 1, 2
QP_OPTIMAL, QP_INACCURATE, QP_INFEASIBLE, QP_FAILED = 0, 1, 2, 3
LL_KINDS = {"pd": 0, "sm": 1}
PLANTS = {"rqp": 0, "rp": 1}  # DAT_PLANT_*


class DatError(RuntimeError):
    pass


class Config(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("mode", ctypes.c_int),
        ("n", ctypes.c_int),
        ("batch", ctypes.c_int),
        ("dt", ctypes.c_double),
        ("hl_every", ctypes.c_int),
        ("max_iter", ctypes.c_int),
        ("res_tol", ctypes.c_double),
        ("use_total_res", ctypes.c_int),
        ("rho0", ctypes.c_double),
        ("tau_incr", ctypes.c_double),
        ("rho_max", ctypes.c_double),
        ("record_err", ctypes.c_int),
    ]


class EpisodeRules(ctypes.Structure):
    """dat_episode_rules (include/dat.h)"""

    _fields_ = [
        ("goal_x", ctypes.c_double),
        ("bound", ctypes.c_double),
        ("max_steps", ctypes.c_int),
        ("stall_steps", ctypes.c_int),
        ("on_collision", ctypes.c_int),
        ("wrap", ctypes.c_int),
    ]


def source_hash() -> str:
    """sha256 of the library's sources (the build stamp next to libdat.so records the one it was built from)."""
    h = hashlib.sha256()
    for d in DEPS:
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


STAMP = LIB_PATH + ".srchash"


def _stamp() -> str | None:
    if os.path.exists(LIB_PATH) and os.path.exists(STAMP):
        with open(STAMP) as f:
            return f.read().strip()
    return None


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile libdat.so (gfx950) next to this file unless it exists and was built from the current
    sources (content hash, not file times: a copied tree keeps its stamp).  Concurrent callers (the
    ranks bench.py spawns) serialise on a file lock; objects go to per-process names and the library
    is moved into place atomically, so a process that loads it never sees a partial file."""
    import fcntl

    want = source_hash()
    if not force and _stamp() == want:
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    with open(os.path.join(OBJ_DIR, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not force and _stamp() == want:  # built by another process while this one waited
            return LIB_PATH
        tag = f"{os.getpid()}"
        objs = [os.path.join(OBJ_DIR, f"{os.path.basename(src)}.{tag}.o") for src in SRCS]
        tmp_lib = f"{LIB_PATH}.{tag}.tmp"
        cmds = [["hipcc"] + HIPFLAGS + ["-c", src, "-o", o] for src, o in zip(SRCS, objs)]
        procs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for c in cmds]
        errs = []
        try:
            for c, pr in zip(cmds, procs):
                _, err = pr.communicate()
                if pr.returncode != 0:
                    errs.append("hipcc failed: " + " ".join(c) + "\n" + err[-4000:])
        finally:
            for pr in procs:  # never leave a compiler behind
                if pr.poll() is None:
                    pr.kill()
                    pr.wait()
        try:
            if errs:
                raise DatError("\n".join(errs))
            link = ["hipcc"] + HIPFLAGS + ["-shared"] + objs + ["-lrccl", "-o", tmp_lib]
            r = subprocess.run(link, capture_output=True, text=True)
            if r.returncode != 0:
                raise DatError("hipcc link failed:\n" + r.stderr[-4000:])
            os.replace(tmp_lib, LIB_PATH)
            with open(STAMP + f".{tag}", "w") as f:
                f.write(want + "\n")
            os.replace(STAMP + f".{tag}", STAMP)
        finally:
            for o in objs + [tmp_lib]:
                if os.path.exists(o):
                    os.remove(o)
        if verbose:
            for c in cmds + [link]:
                print(" ".join(c))
    return LIB_PATH


_lib = None

D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int)
U8 = ctypes.POINTER(ctypes.c_uint8)
LL = ctypes.POINTER(ctypes.c_longlong)
H = ctypes.c_void_p

EXPORTS = {
    "dat_default_config": (None, [ctypes.POINTER(Config)]),
    "dat_create": (ctypes.c_int, [ctypes.POINTER(Config), ctypes.POINTER(H)]),
    "dat_destroy": (ctypes.c_int, [H]),
    "dat_last_error": (ctypes.c_char_p, []),
    "dat_device_count": (ctypes.c_int, []),
    "dat_set_params": (ctypes.c_int, [H, D, ctypes.c_int]),
    "dat_set_forests": (ctypes.c_int, [H, ctypes.c_int, I, D, I, D]),
    "dat_set_tolerance": (ctypes.c_int, [H, ctypes.c_double, ctypes.c_int]),
    "dat_set_max_iter": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_set_qp_tolerance": (ctypes.c_int, [H, ctypes.c_double]),
    "dat_reset_warm_start": (ctypes.c_int, [H]),
    "dat_set_state": (ctypes.c_int, [H, D, I]),
    "dat_get_state": (ctypes.c_int, [H, D, I]),
    "dat_checkpoint_bytes": (ctypes.c_int, [H, ctypes.c_int, LL]),
    "dat_checkpoint_save": (ctypes.c_int, [H, I, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong]),
    "dat_checkpoint_load": (ctypes.c_int, [H, ctypes.c_void_p, ctypes.c_longlong, I, I, ctypes.c_int]),
    "dat_get_checkpoint_ms": (ctypes.c_int, [H, D, D]),
    "dat_control_step": (ctypes.c_int, [H, D, D, D, I, I, D, U8, D]),
    "dat_rollout": (ctypes.c_int, [H, ctypes.c_int, D]),
    "dat_closed_loop": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_control_steps": (ctypes.c_int, [H, ctypes.c_int, D, D, I, I]),
    "dat_set_tracking": (ctypes.c_int, [H, D, ctypes.c_int]),
    "dat_set_clock": (ctypes.c_int, [H, ctypes.c_longlong]),
    "dat_get_clock": (ctypes.c_int, [H, LL]),
    "dat_set_plant": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_set_sub_batches": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_set_advance_overlap": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_set_step_pipeline": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_set_fused_advance": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_get_fused_launches": (ctypes.c_int, [H, LL, LL]),
    "dat_get_stream_count": (ctypes.c_int, [H]),
    "dat_get_advance_counts": (ctypes.c_int, [H, LL, LL]),
    "dat_debug_advance_split": (ctypes.c_int, [H, U8]),
    "dat_debug_get_env_class": (ctypes.c_int, [H, D, D, I, I]),
    "dat_get_step_marks": (ctypes.c_int, [H, D, ctypes.c_int]),
    "dat_get_counters": (ctypes.c_int, [H, LL, LL, LL, LL, D]),
    "dat_get_class_counters": (ctypes.c_int, [H, ctypes.c_int, LL, LL, LL, D]),
    "dat_get_class_occupancy": (ctypes.c_int, [H, ctypes.c_int, LL, LL]),
    "dat_reset_counters": (ctypes.c_int, [H]),
    "dat_synchronize": (ctypes.c_int, [H]),
    "dat_set_persistent_blocks": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_cadmm_slots": (ctypes.c_int, [H, ctypes.c_int, I]),
    "dat_debug_row_modes": (ctypes.c_int, [H, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dat_debug_tail_rule": (ctypes.c_int, [H, ctypes.c_int, ctypes.c_int]),
    "dat_cadmm_row_mode": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dat_env_rows": (ctypes.c_int, [H, D, D, I, U8, D]),
    "dat_solve_agent_qp_batch": (ctypes.c_int, [H, ctypes.c_int, I, I, D, D, D, D, D, D, I, I, U8, D]),
    "dat_solve_agent_qp_rows_batch": (ctypes.c_int, [H, ctypes.c_int, I, I, D, D, D, D, D, D, D, I, D, I, I, U8, D,
                                                     U8]),
    "dat_set_low_level": (ctypes.c_int, [H, ctypes.c_int]),
    "dat_get_kernel_ms": (ctypes.c_int, [H, D]),
    "dat_get_inband_exits": (ctypes.c_int, [H, LL, LL]),
    "dat_get_refinement_counters": (ctypes.c_int, [H, LL, LL]),
    "dat_get_robust_redos": (ctypes.c_int, [H, LL]),
    "dat_get_tail_counters": (ctypes.c_int, [H, LL]),
    "dat_get_collision_stats": (ctypes.c_int, [H, LL, D]),
    "dat_get_agent_qp_ms": (ctypes.c_int, [H, D]),
    "dat_rp_rollout": (ctypes.c_int, [H, ctypes.c_int, D]),
    "dat_pmrl_rollout": (ctypes.c_int, [H, ctypes.c_int, D, ctypes.c_int]),
    "dat_pmrl_forward": (ctypes.c_int, [H, D, D, D, D, D]),
    "dat_low_level_control": (ctypes.c_int, [H, D, D, D]),
    "dat_log_begin": (ctypes.c_int, [H, I, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dat_log_counts": (ctypes.c_int, [H, LL, LL, LL]),
    "dat_log_read_hl": (ctypes.c_int, [H, ctypes.c_int, ctypes.c_int, D, I, I, D, U8, D, D, D]),
    "dat_log_read_steps": (ctypes.c_int, [H, ctypes.c_int, ctypes.c_int, LL, D, D, D, D, D]),
    "dat_log_read_summary": (ctypes.c_int, [H, ctypes.c_int, ctypes.c_int, I, D, U8]),
    "dat_log_clear": (ctypes.c_int, [H]),
    "dat_log_end": (ctypes.c_int, [H]),
    "dat_episode_default_rules": (None, [ctypes.POINTER(EpisodeRules)]),
    "dat_episode_begin": (ctypes.c_int, [H, ctypes.POINTER(EpisodeRules), ctypes.c_void_p, ctypes.c_longlong,
                                         ctypes.c_int]),
    "dat_episode_counts": (ctypes.c_int, [H, LL, LL, LL, LL]),
    "dat_episode_read": (ctypes.c_int, [H, ctypes.c_int, ctypes.c_int, I, I, I, I, LL, LL, I, I, I, I, I, D, D, D]),
    "dat_episode_clear": (ctypes.c_int, [H]),
    "dat_episode_end": (ctypes.c_int, [H]),
    "dat_episode_slots": (ctypes.c_int, [H, I, I, I, I]),
    "dat_get_episode_respawns": (ctypes.c_int, [H, LL, LL, LL]),
    "dat_comm_unique_id": (ctypes.c_int, [U8]),
    "dat_comm_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, U8, ctypes.POINTER(H)]),
    "dat_comm_destroy": (ctypes.c_int, [H]),
    "dat_comm_allgather": (ctypes.c_int, [H, D, ctypes.c_longlong, D]),
    "dat_comm_allreduce": (ctypes.c_int, [H, D, ctypes.c_longlong, ctypes.c_int]),
    "dat_comm_barrier": (ctypes.c_int, [H]),
    "dat_comm_last_error": (ctypes.c_char_p, []),
}


def lib() -> ctypes.CDLL:
    """Load libdat.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        path = os.environ.get("DAT_LIB_PATH", LIB_PATH)  # development: A/B a differently compiled build
        if not os.path.exists(path):
            raise DatError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = ctypes.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            if path != LIB_PATH and not hasattr(L, name):
                continue  # an older A/B build lacks a later export; the in-tree build must have them all
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise DatError(lib().dat_last_error().decode())


def ptr(a, ctype=D):
    if a is None:
        return None
    return a.ctypes.data_as(ctype)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)
