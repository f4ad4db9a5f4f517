"""Controllers on top of libdat.so -- the reference's controller API, batched and drop-in.

Batched engine
  ``BatchedController(mode, n, batch, params, col, ...)``: one HIP handle driving B independent
  scenarios; ``control(states, acc_des)`` runs one high-level step for all of them on the GPU.

Drop-in single-scenario classes (same constructor and per-step interface as the reference):
  ``RQPCentralizedController``  control/rqp_centralized.py:27-455
  ``RQPCADMMController``        control/rqp_cadmm.py:510-688
  ``RQPDDController``           control/rqp_dd.py:558-764
  each: ``__init__(params, col, state, dt, env=None, verbose=False)``,
        ``control(state, acc_des) -> (f_des (3, n), SolverStatistics)``,
        ``get_force_cone_angle_bound()``, ``get_dist_eps()``,
        ``set_force_err_tolerance(tol[, use_total_res])``, ``set_max_iter(k)`` (C-ADMM / DD).
  ``RQPLowLevelController(so3_controller_type, params, max_f_ang)``: control/rqp_centralized.py:457-535
        ("pd" or "sm" SO(3) law) on the GPU; ``BatchedController.set_low_level`` selects the law of the
        device rollout (SO(3) law + rigid-body dynamics + Lie integration).
The QPs are solved by the HIP kernels; the reference's Clarabel per-call solve time becomes the
GPU kernel time of the step (``SolverStatistics.solve_time``).
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Any, List, Optional, Tuple

import numpy as np

from . import _lib as L
from . import layout
from .system import (RQPCollision, RQPParameters, RQPState, _skew, equilibrium_forces, pack_mountain, pack_params,
                     pack_state)

MODES = {"centralized": L.MODE_CENTRALIZED, "consensus-admm": L.MODE_CADMM, "cadmm": L.MODE_CADMM,
         "dual-decomposition": L.MODE_DD, "dd": L.MODE_DD}


@dataclass
class SolverStatistics:
    """control/rqp_centralized.py:18-24."""

    iter: int
    solve_time: float
    collision: bool
    min_env_dist: float
    err_seq: Optional[List[float]] = None


@dataclass
class StepResult:
    """Batched outputs of one high-level step (leading axis: scenario)."""

    f_des: np.ndarray           # (B, 3, n)
    iters: np.ndarray           # (B,)
    qp_status: np.ndarray       # (B, n)
    min_env_dist: np.ndarray    # (B,)
    collision: Optional[np.ndarray]  # (B,) bool (None: not computed, control_steps)
    err_seq: Optional[np.ndarray] = None  # (B, max_iter + 1), NaN padded
    gpu_ms: float = 0.0


class Checkpoint:
    """Checkpoint records of ``count`` scenarios of one controller type (``mode``: DAT_MODE_*) and team size ``n``:
    the blob of dat_checkpoint_save (include/dat.h; layout: csrc/dat_layout.h, DAT_CK_*).  Each record holds the
    scenario's state and polar counter, f_des, the previous step's pass counts and the controller's warm state.
    Host data only: ``BatchedController.checkpoint`` makes one, ``BatchedController.restore`` writes records back
    into scenarios of any handle of the same mode and n."""

    # the record's arrays under the reference's names, with their shapes per scenario (n -> shape), agent-major
    _NAMES = {"state": ("state", lambda n: (layout.state_size(n),)), "fdes": ("f_des", lambda n: (n, 3)),
              "cf": ("f", lambda n: (n, n, 3)), "cfbar": ("f_mean", lambda n: (n, 3)),
              "clam": ("lambda_f", lambda n: (n, n, 3)), "dlamF": ("lambda_F", lambda n: (n, 3)),
              "dlamM": ("lambda_M", lambda n: (n, 3)), "dprev": ("prev", lambda n: (n, 9)),
              "pf": ("prev_f", lambda n: (n, 3))}

    def __init__(self, data, copy: bool = True) -> None:
        """data: a blob (bytes-like, or a contiguous numpy array); copy=False adopts a writable array as it is."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
        if copy or not buf.flags.writeable:
            buf = np.array(buf, dtype=np.uint8, copy=True)
        H = layout.CK_H
        if buf.size < layout.CK_HEADER_BYTES:
            raise ValueError(f"checkpoint: {buf.size} bytes are shorter than the {layout.CK_HEADER_BYTES}-byte header")
        hdr = buf[: layout.CK_HEADER_BYTES]
        if int(hdr[H["MAGIC"]: H["MAGIC"] + 8].view(np.uint64)[0]) != layout.CK_MAGIC:
            raise ValueError("checkpoint: bad magic (not a checkpoint)")
        version, mode, n, words = (int(v) for v in hdr[H["VERSION"]: H["VERSION"] + 16].view(np.int32))
        count = int(hdr[H["COUNT"]: H["COUNT"] + 8].view(np.int64)[0])
        if version != layout.CK_VERSION:
            raise ValueError(f"checkpoint: format version {version}, this package reads version {layout.CK_VERSION}")
        if mode not in layout.CK_MODES:
            raise ValueError(f"checkpoint: bad mode {mode}")
        if not 3 <= n <= 16:
            raise ValueError(f"checkpoint: bad n = {n}")
        if words != layout.ck_words(mode, n):
            raise ValueError(f"checkpoint: {words} words per record, mode {mode} at n = {n} has "
                             f"{layout.ck_words(mode, n)}")
        if hdr[H["PAD"]:].any():
            raise ValueError("checkpoint: header padding is not zero")
        if count < 0 or buf.size != layout.CK_HEADER_BYTES + count * words * 8:
            raise ValueError(f"checkpoint: {buf.size} bytes, the header's {count} records take "
                             f"{layout.CK_HEADER_BYTES + count * words * 8}")
        self.mode, self.n, self.count, self.words = mode, n, count, words
        self._buf = buf

    @staticmethod
    def header(mode: int, n: int, count: int) -> np.ndarray:
        """The 64-byte header of a blob of `count` records."""
        H = layout.CK_H
        hdr = np.zeros(layout.CK_HEADER_BYTES, dtype=np.uint8)
        hdr[H["MAGIC"]: H["MAGIC"] + 8].view(np.uint64)[0] = layout.CK_MAGIC
        hdr[H["VERSION"]: H["VERSION"] + 16].view(np.int32)[:] = (layout.CK_VERSION, mode, n, layout.ck_words(mode, n))
        hdr[H["COUNT"]: H["COUNT"] + 8].view(np.int64)[0] = count
        return hdr

    def records(self) -> np.ndarray:
        """(count, words) float64 view of the records."""
        return self._buf[layout.CK_HEADER_BYTES:].view(np.float64).reshape(self.count, self.words)

    def tobytes(self) -> bytes:
        return self._buf.tobytes()

    @classmethod
    def frombytes(cls, data) -> "Checkpoint":
        return cls(data)

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(self._buf.data)

    @classmethod
    def load(cls, path) -> "Checkpoint":
        with open(path, "rb") as f:
            return cls(f.read())

    def select(self, indices) -> "Checkpoint":
        """A new checkpoint of the records `indices`, in that order; an index may repeat (replication)."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.count):
            raise IndexError(f"checkpoint: record index out of range [0, {self.count})")
        body = np.ascontiguousarray(self.records()[idx]).view(np.uint8).reshape(-1)
        return Checkpoint(np.concatenate([self.header(self.mode, self.n, idx.size), body]), copy=False)

    def arrays(self) -> dict:
        """Views into the records, leading axis the record: state (12n + 18), counter, f_des (n, 3), iters, ipmx
        (int32; the previous step's ADMM / DD passes and slowest IPM count) and the mode's warm state in the device's
        agent-major layout -- C-ADMM f (n, n, 3) with f[i] agent i's copy, f_mean (n, 3), lambda_f (n, n, 3); DD
        lambda_F, lambda_M (n, 3), prev (n, 9) = per agent (f_i, F_i, M_i); centralized prev_f (n, 3)."""
        rec, n = self.records(), self.n
        out = {}
        for arr, (off, words) in layout.ck_fields(self.mode, n).items():
            name, shape = self._NAMES[arr]
            out[name] = rec[:, off: off + words].reshape((self.count,) + shape(n))
        ints = rec.view(np.int32).reshape(self.count, 2 * self.words)
        for arr, k in layout.CK_INTS.items():
            out[arr] = ints[:, 2 * layout.ck_ints(n) + k]
        return out


class BatchedController:
    """B independent scenarios of one controller type on one GPU."""

    def __init__(self, mode, n: int, batch: int, params: np.ndarray, *, per_scenario_params: bool = False,
                 dt: float = 1e-3, hl_every: int = 10, device: int = 0, max_iter: int = 100, res_tol: float = 1e-2,
                 use_total_res: bool = True, record_err: bool = False, rho0: float = 1.0, tau_incr: float = 1.0,
                 rho_max: float = 2.0) -> None:
        self.mode = MODES[mode] if isinstance(mode, str) else int(mode)
        self.n, self.batch = n, batch
        lib = L.lib()
        cfg = L.Config()
        lib.dat_default_config(cfg)
        cfg.device, cfg.mode, cfg.n, cfg.batch = device, self.mode, n, batch
        cfg.dt, cfg.hl_every, cfg.max_iter, cfg.res_tol = dt, hl_every, max_iter, res_tol
        cfg.use_total_res, cfg.record_err = int(use_total_res), int(record_err)
        cfg.rho0, cfg.tau_incr, cfg.rho_max = rho0, tau_incr, rho_max
        self.cfg = cfg
        h = L.H()
        L.check(lib.dat_create(cfg, h))
        self._h = h
        self._lib = lib
        params = L.f64(params)
        if per_scenario_params:
            assert params.shape == (batch, layout.param_size(n)), params.shape
        else:
            assert params.shape == (layout.param_size(n),), params.shape
        self.params = params
        L.check(lib.dat_set_params(h, L.ptr(params), int(per_scenario_params)))

    # -- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.dat_destroy(self._h)
            self._h = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    # -- configuration
    def set_forests(self, forests: list, scenario_forest: Optional[np.ndarray] = None) -> None:
        """forests: list of objects with tree_pos (T, 3) and mountain constants; [] removes the env."""
        if not forests:
            L.check(self._lib.dat_set_forests(self._h, 0, None, None, None, None))
            return
        offs = np.zeros(len(forests) + 1, dtype=np.int32)
        for k, f in enumerate(forests):
            offs[k + 1] = offs[k] + f.tree_pos.shape[0]
        trees = L.f64(np.concatenate([f.tree_pos for f in forests]))
        mountains = L.f64(np.stack([pack_mountain(f) for f in forests]))
        sf = None if scenario_forest is None else L.i32(scenario_forest)
        if sf is not None:
            assert sf.shape == (self.batch,)
        L.check(self._lib.dat_set_forests(self._h, len(forests), L.ptr(offs, L.I), L.ptr(trees),
                                          None if sf is None else L.ptr(sf, L.I), L.ptr(mountains)))

    def set_force_err_tolerance(self, tol: float, use_total_res: bool = True) -> None:
        L.check(self._lib.dat_set_tolerance(self._h, float(tol), int(use_total_res)))
        self.cfg.res_tol, self.cfg.use_total_res = tol, int(use_total_res)

    def set_max_iter(self, max_iter: int) -> None:
        L.check(self._lib.dat_set_max_iter(self._h, int(max_iter)))
        self.cfg.max_iter = max_iter

    def set_qp_tolerance(self, tol: float) -> None:
        """IPM stopping tolerance of every QP (default 1e-10; 1e-8 is Clarabel's default, which the
        reference runs with: control/rqp_cadmm.py:492). Must lie in [1e-12, 1e-7]."""
        L.check(self._lib.dat_set_qp_tolerance(self._h, float(tol)))

    def set_persistent_blocks(self, blocks: int) -> None:
        """C-ADMM / DD: resident k_cadmm / k_dd workgroups draining the scenario queues (0: default)."""
        L.check(self._lib.dat_set_persistent_blocks(self._h, int(blocks)))

    def cadmm_slots(self, batch: Optional[int] = None) -> int:
        """Scenario slots per k_cadmm wavefront for a (sub-)batch of `batch` scenarios (dat_cadmm_slots)."""
        g = ctypes.c_int()
        L.check(self._lib.dat_cadmm_slots(self._h, int(self.batch if batch is None else batch), ctypes.byref(g)))
        return g.value

    def debug_row_modes(self, modes: Optional[Tuple[int, int, int]]) -> None:
        """dat_debug_row_modes (tests): run k_cadmm with the row modes (m0, m1, m2) of env classes 0-2 instead of the
        rule's; None returns to the rule.  A triple k_cadmm is not built for raises DatError."""
        m0, m1, m2 = (-1, -1, -1) if modes is None else (int(m) for m in modes)
        L.check(self._lib.dat_debug_row_modes(self._h, m0, m1, m2))

    def debug_tail_rule(self, tail_prev: Optional[int] = None, tail_pass: Optional[int] = None) -> None:
        """dat_debug_tail_rule (tests): the tail rule with (tail_prev, tail_pass) instead of the library's pair; None
        returns to it."""
        pair = (-1, -1) if tail_prev is None or tail_pass is None else (int(tail_prev), int(tail_pass))
        L.check(self._lib.dat_debug_tail_rule(self._h, *pair))

    def reset_warm_start(self) -> None:
        L.check(self._lib.dat_reset_warm_start(self._h))

    # -- the tracking law, the clock and the plant (dat_set_tracking, dat_set_clock, dat_set_plant)
    def set_tracking(self, records: Optional[np.ndarray]) -> None:
        """Select the trajectory-tracking law (tracking.py) wherever the device computes a desired acceleration:
        records (TRACK_SIZE,) for every scenario or (B, TRACK_SIZE) per scenario; None restores the forest law.
        Independent of set_forests.  A record the law rejects raises DatError and changes nothing."""
        if records is None:
            L.check(self._lib.dat_set_tracking(self._h, None, 0))
            return
        rec = L.f64(records)
        if rec.shape not in ((layout.TRACK_SIZE,), (self.batch, layout.TRACK_SIZE)):
            raise ValueError(f"set_tracking: records of shape {rec.shape}, expected ({layout.TRACK_SIZE},) or "
                             f"({self.batch}, {layout.TRACK_SIZE})")
        L.check(self._lib.dat_set_tracking(self._h, L.ptr(rec), int(rec.ndim == 2)))

    def set_clock(self, clock: int) -> None:
        """The handle's clock in simulation steps (>= 0): the tracking law's time is clock * dt."""
        L.check(self._lib.dat_set_clock(self._h, int(clock)))

    @property
    def clock(self) -> int:
        """Simulation steps since the handle was made (or set_clock): closed_loop, rollout and rp_rollout advance it."""
        c = ctypes.c_longlong()
        L.check(self._lib.dat_get_clock(self._h, ctypes.byref(c)))
        return c.value

    def set_plant(self, plant: str) -> None:
        """What closed_loop rolls out: "rqp" (default, the quadrotor-payload system) or "rp" (the rigid payload under
        the controller's forces; centralized handles, no log)."""
        if plant not in L.PLANTS:
            raise NotImplementedError(plant)
        L.check(self._lib.dat_set_plant(self._h, L.PLANTS[plant]))

    # -- state
    def set_state(self, states: np.ndarray, counters: Optional[np.ndarray] = None) -> None:
        states = L.f64(states)
        assert states.shape == (self.batch, layout.state_size(self.n))
        c = None if counters is None else L.i32(counters)
        L.check(self._lib.dat_set_state(self._h, L.ptr(states), None if c is None else L.ptr(c, L.I)))

    def get_state(self):
        st = np.empty((self.batch, layout.state_size(self.n)))
        c = np.empty(self.batch, dtype=np.int32)
        L.check(self._lib.dat_get_state(self._h, L.ptr(st), L.ptr(c, L.I)))
        return st, c

    # -- checkpoints (dat_checkpoint_*): scenarios with their controllers' warm state
    def checkpoint(self, scenarios=None) -> Checkpoint:
        """The records of `scenarios` (any indices in [0, batch), repeats allowed; None: all, in order)."""
        if scenarios is None:
            sc, count = None, self.batch
        else:
            sc = L.i32(np.asarray(scenarios).reshape(-1))
            count = sc.shape[0]
        nb = ctypes.c_longlong()
        L.check(self._lib.dat_checkpoint_bytes(self._h, count, ctypes.byref(nb)))
        buf = np.empty(nb.value, dtype=np.uint8)
        L.check(self._lib.dat_checkpoint_save(self._h, L.ptr(sc, L.I), count, buf.ctypes.data_as(ctypes.c_void_p),
                                              nb.value))
        return Checkpoint(buf, copy=False)

    def restore(self, ckpt, records=None, scenarios=None) -> None:
        """Write record records[k] of `ckpt` (a Checkpoint, or a blob's bytes) into scenario scenarios[k].  records
        may repeat (a fork), scenarios must be distinct; None: 0..count-1, count being the length of the list
        given, else the checkpoint's.  Scenarios not named are untouched; the next closed_loop / control computes
        desired acceleration and env rows from the restored states, as after set_state.  The blob is checked
        against the handle first (mode, n, sizes, indices): a DatError names the cause, nothing was written."""
        data = ckpt._buf if isinstance(ckpt, Checkpoint) else np.frombuffer(bytes(ckpt), dtype=np.uint8)
        rec = None if records is None else L.i32(np.asarray(records).reshape(-1))
        sc = None if scenarios is None else L.i32(np.asarray(scenarios).reshape(-1))
        if rec is not None and sc is not None and rec.shape != sc.shape:
            raise ValueError(f"restore: {rec.shape[0]} records for {sc.shape[0]} scenarios")
        if rec is not None or sc is not None:
            count = (rec if rec is not None else sc).shape[0]
        elif isinstance(ckpt, Checkpoint):
            count = ckpt.count
        else:  # (a raw blob: its own record count, if it has one to read; the library checks the rest)
            H = layout.CK_H["COUNT"]
            count = int(data[H: H + 8].view(np.int64)[0]) if data.size >= H + 8 else 0
            count = min(max(count, 0), self.batch)
        L.check(self._lib.dat_checkpoint_load(self._h, data.ctypes.data_as(ctypes.c_void_p), data.size,
                                              L.ptr(rec, L.I), L.ptr(sc, L.I), count))

    def checkpoint_ms(self) -> Tuple[float, float]:
        """Device time [ms] of the last checkpoint's / restore's (copy kernel, host copy) -- dat_get_checkpoint_ms."""
        k, c = ctypes.c_double(), ctypes.c_double()
        L.check(self._lib.dat_get_checkpoint_ms(self._h, ctypes.byref(k), ctypes.byref(c)))
        return k.value, c.value

    # -- steps
    def control(self, states: Optional[np.ndarray] = None, acc_des: Optional[np.ndarray] = None) -> StepResult:
        B, n = self.batch, self.n
        st = None if states is None else L.f64(states)
        acc = None if acc_des is None else L.f64(acc_des)
        if st is not None:
            assert st.shape == (B, layout.state_size(n))
        if acc is not None:
            assert acc.shape == (B, 6)
        f = np.empty((B, 3 * n))
        it = np.empty(B, dtype=np.int32)
        qs = np.empty((B, n), dtype=np.int32)
        md = np.empty(B)
        col = np.empty(B, dtype=np.uint8)
        err = np.empty((B, self.cfg.max_iter + 1)) if self.cfg.record_err else None
        _, _, _, ms0 = self.counters()
        L.check(self._lib.dat_control_step(self._h, L.ptr(st), L.ptr(acc), L.ptr(f), L.ptr(it, L.I), L.ptr(qs, L.I),
                                           L.ptr(md), L.ptr(col, L.U8), L.ptr(err)))
        _, _, _, ms1 = self.counters()
        return StepResult(f.reshape(B, n, 3).transpose(0, 2, 1), it, qs, md, col.astype(bool), err, ms1 - ms0)

    def set_low_level(self, so3_controller_type: str) -> None:
        """Low-level law of rollout / closed_loop: "pd" (default) or "sm" (control/rqp_centralized.py:468-482)."""
        if so3_controller_type not in L.LL_KINDS:
            raise NotImplementedError(so3_controller_type)
        L.check(self._lib.dat_set_low_level(self._h, L.LL_KINDS[so3_controller_type]))

    def low_level(self, f_des: Optional[np.ndarray] = None):
        """RQPLowLevelController.control at the current states: (thrust (B, n), moment (B, 3, n))."""
        B, n = self.batch, self.n
        fd = None
        if f_des is not None:
            fd = L.f64(np.asarray(f_des, float).reshape(B, 3, n).transpose(0, 2, 1).reshape(B, 3 * n))
        f = np.empty((B, n))
        M = np.empty((B, n, 3))
        L.check(self._lib.dat_low_level_control(self._h, L.ptr(fd), L.ptr(f), L.ptr(M)))
        return f, M.transpose(0, 2, 1)

    def rollout(self, steps: int, f_des: Optional[np.ndarray] = None) -> None:
        fd = None
        if f_des is not None:
            fd = L.f64(np.asarray(f_des).transpose(0, 2, 1).reshape(self.batch, 3 * self.n))
        L.check(self._lib.dat_rollout(self._h, int(steps), L.ptr(fd)))

    def rp_rollout(self, steps: int, f: Optional[np.ndarray] = None) -> None:
        """Rigid-payload dynamics (dat_rp_rollout) with forces f (B, 3, n) held for `steps` steps."""
        fd = None
        if f is not None:
            fd = L.f64(np.asarray(f).transpose(0, 2, 1).reshape(self.batch, 3 * self.n))
        L.check(self._lib.dat_rp_rollout(self._h, int(steps), L.ptr(fd)))

    def pmrl_rollout(self, steps: int, f: np.ndarray) -> None:
        """Point-mass rigid-link dynamics (dat_pmrl_rollout): `steps` steps under the force schedule f, (B, 3, n)
        held throughout or (nf, B, 3, n) with steps % nf == 0 and each set held steps / nf steps."""
        f = np.asarray(f, float)
        if f.ndim == 3:
            f = f[None]
        assert f.ndim == 4 and f.shape[1:] == (self.batch, 3, self.n), f.shape
        fd = L.f64(f.transpose(0, 1, 3, 2).reshape(f.shape[0], self.batch, 3 * self.n))
        L.check(self._lib.dat_pmrl_rollout(self._h, int(steps), L.ptr(fd), int(f.shape[0])))

    def pmrl_forward(self, f: np.ndarray):
        """PMRLDynamics.forward_dynamics at the current states (dat_pmrl_forward) under the thrusts f (B, 3, n):
        ((ddq (B, 3, n), dvl (B, 3), dwl (B, 3)), T (B, n)).  The states are left alone."""
        B, n = self.batch, self.n
        f = np.asarray(f, float)
        assert f.shape == (B, 3, n), f.shape
        fd = L.f64(f.transpose(0, 2, 1).reshape(B, 3 * n))
        ddq, dvl, dwl, T = np.empty((B, n, 3)), np.empty((B, 3)), np.empty((B, 3)), np.empty((B, n))
        L.check(self._lib.dat_pmrl_forward(self._h, L.ptr(fd), L.ptr(ddq), L.ptr(dvl), L.ptr(dwl), L.ptr(T)))
        return (ddq.transpose(0, 2, 1).copy(), dvl, dwl), T

    def set_sub_batches(self, count: int) -> None:
        """dat_set_sub_batches: closed_loop on `count` sub-batches with one stream each (C-ADMM)."""
        L.check(self._lib.dat_set_sub_batches(self._h, int(count)))

    def set_advance_overlap(self, on: bool) -> None:
        """dat_set_advance_overlap: the closed loop's early advance of finished scenarios beside the drain."""
        L.check(self._lib.dat_set_advance_overlap(self._h, int(bool(on))))

    def set_step_pipeline(self, on: bool) -> None:
        """dat_set_step_pipeline: the next step's drain of the advanced scenarios starts beside the ramp-down."""
        L.check(self._lib.dat_set_step_pipeline(self._h, int(bool(on))))

    def set_fused_advance(self, on: bool) -> None:
        """dat_set_fused_advance: a pass's rollout, desired acceleration and env rows in one launch (k_advance)."""
        L.check(self._lib.dat_set_fused_advance(self._h, int(bool(on))))

    def fused_launches(self) -> Tuple[int, int]:
        """dat_get_fused_launches: launches of (k_advance, k_bucket_scatter) since the handle was made."""
        a, s = ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_get_fused_launches(self._h, ctypes.byref(a), ctypes.byref(s)))
        return a.value, s.value

    def stream_count(self) -> int:
        """dat_get_stream_count: streams the handle holds at the moment."""
        m = self._lib.dat_get_stream_count(self._h)
        if m < 0:
            L.check(m)
        return m

    def advance_counts(self) -> Tuple[int, int]:
        """Scenario-steps advanced by the (early, late) pass of the advance overlap since the last reset."""
        e, l = ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_get_advance_counts(self._h, ctypes.byref(e), ctypes.byref(l)))
        return e.value, l.value

    def debug_advance_split(self, early_mask) -> None:
        """dat_debug_advance_split (tests): a fixed early / late split by mask; None clears it."""
        if early_mask is None:
            L.check(self._lib.dat_debug_advance_split(self._h, None))
            return
        m = np.ascontiguousarray(np.asarray(early_mask) != 0, dtype=np.uint8)
        if m.shape != (self.batch,):
            raise ValueError("early_mask must have one entry per scenario")
        L.check(self._lib.dat_debug_advance_split(self._h, L.ptr(m, L.U8)))

    def debug_env_class(self):
        """dat_debug_get_env_class (tests): the env rows the last control step's k_cadmm consumed, as env_rows
        reports them -- (lhs (B, n, 10, 3), rhs (B, n, 10), nrow (B, n)) -- and the scenarios' env class (B,)."""
        B, n = self.batch, self.n
        lhs = np.empty((B, n, layout.NENV, 3))
        rhs = np.empty((B, n, layout.NENV))
        nr = np.empty((B, n), dtype=np.int32)
        cls = np.empty(B, dtype=np.int32)
        L.check(self._lib.dat_debug_get_env_class(self._h, L.ptr(lhs), L.ptr(rhs), L.ptr(nr, L.I), L.ptr(cls, L.I)))
        return lhs, rhs, nr, cls

    def closed_loop(self, hl_steps: int) -> None:
        L.check(self._lib.dat_closed_loop(self._h, int(hl_steps)))

    # -- episodes (dat_episode_*): scenarios end and respawn from a pool inside closed_loop
    def episodes_begin(self, pool=None, goal_x: Optional[float] = None, max_steps: int = 0, stall_steps: int = 0,
                       on_collision: bool = True, bound: Optional[float] = None, wrap: bool = True,
                       capacity: Optional[int] = None) -> None:
        """Open episodes: from now on closed_loop ends a scenario's episode, after its control step and before its
        rollout, for the lowest reason that fires -- DIVERGED (a non-finite word of xl / vl, or max |xl_c| > bound),
        COLLISION (on_collision), GOAL (xl_x >= goal_x), STALL (stall_steps consecutive control steps at
        max_iter + 1 passes; not on centralized handles), TIME_LIMIT (max_steps control steps) -- records the outcome
        and overwrites the scenario with a record of `pool` instead of rolling it out.  pool: a Checkpoint (or a
        blob's bytes) of P records, uploaded once; None: a checkpoint of the whole batch taken now.  Slot s first
        runs record s mod P (loaded here), then (s + j B) mod P for its j-th respawn; with wrap=False a slot whose
        next index would reach P goes idle (it runs on and records nothing further).  capacity: outcome records the
        table holds (default 4 x batch).  control and rollout do not evaluate episodes.  Not with a log, the "rp"
        plant or tracking records; restore raises while episodes are open."""
        ck = self.checkpoint() if pool is None else pool
        data = ck._buf if isinstance(ck, Checkpoint) else np.frombuffer(bytes(ck), dtype=np.uint8)
        r = L.EpisodeRules()
        self._lib.dat_episode_default_rules(r)
        if goal_x is not None:
            r.goal_x = float(goal_x)
        if bound is not None:
            r.bound = float(bound)
        r.max_steps, r.stall_steps = int(max_steps), int(stall_steps)
        r.on_collision, r.wrap = int(bool(on_collision)), int(bool(wrap))
        cap = 4 * self.batch if capacity is None else int(capacity)
        L.check(self._lib.dat_episode_begin(self._h, r, data.ctypes.data_as(ctypes.c_void_p), data.size, cap))

    def episodes_counts(self) -> dict:
        """ended: episodes ended per reason since episodes_begin (a dict by reason name, and "total"); held: records
        in the table; lost: records dropped beyond its capacity since the last episodes_clear; idle: idle slots."""
        e = np.zeros(layout.EP_NREASON, dtype=np.int64)
        h, lo, i = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_episode_counts(self._h, L.ptr(e, L.LL), ctypes.byref(h), ctypes.byref(lo),
                                             ctypes.byref(i)))
        ended = {k: int(e[v]) for k, v in layout.EP_REASONS.items() if v}
        ended["total"] = int(e.sum())
        return {"ended": ended, "held": h.value, "lost": lo.value, "idle": i.value}

    def episodes_read(self, allow_lost: bool = False) -> dict:
        """The outcome records held, sorted by (end tick, slot): slot, episode, record, reason (layout.EP_REASONS),
        start_tick, end_tick, steps, iter_sum, iter_max, full_steps (steps at max_iter + 1 passes), stall_run (int
        arrays), min_env_dist, xl, vl (K, 3): the state the episode's last control step saw.  Raises DatError where
        records were lost to the table's capacity, unless allow_lost."""
        c = self.episodes_counts()
        if c["lost"] > 0 and not allow_lost:
            raise L.DatError(f"episodes_read: {c['lost']} outcome records were lost to the table's capacity "
                             f"({c['held']} held): open the episodes with a larger capacity or read and clear more often")
        K = c["held"]
        names = ("slot", "episode", "record", "reason", "steps", "iter_sum", "iter_max", "full_steps", "stall_run")
        o = {k: np.zeros(K, dtype=np.int32) for k in names}
        o.update(start_tick=np.zeros(K, dtype=np.int64), end_tick=np.zeros(K, dtype=np.int64),
                 min_env_dist=np.zeros(K), xl=np.zeros((K, 3)), vl=np.zeros((K, 3)))
        L.check(self._lib.dat_episode_read(
            self._h, 0, K, L.ptr(o["slot"], L.I), L.ptr(o["episode"], L.I), L.ptr(o["record"], L.I),
            L.ptr(o["reason"], L.I), L.ptr(o["start_tick"], L.LL), L.ptr(o["end_tick"], L.LL), L.ptr(o["steps"], L.I),
            L.ptr(o["iter_sum"], L.I), L.ptr(o["iter_max"], L.I), L.ptr(o["full_steps"], L.I),
            L.ptr(o["stall_run"], L.I), L.ptr(o["min_env_dist"]), L.ptr(o["xl"]), L.ptr(o["vl"])))
        order = np.lexsort((o["slot"], o["end_tick"]))
        return {k: v[order] for k, v in o.items()}

    def episodes_clear(self) -> None:
        """Empty the outcome table and zero `lost`; totals, idle slots and the running episodes stay."""
        L.check(self._lib.dat_episode_clear(self._h))

    def episodes_end(self) -> None:
        """Close the episodes: closed_loop is the plain loop again (the scenarios stay as they are)."""
        L.check(self._lib.dat_episode_end(self._h))

    def episodes_slots(self) -> dict:
        """Per slot: record (the pool record its running episode started from), episodes (finished), steps (control
        steps of the running episode), idle."""
        o = {k: np.zeros(self.batch, dtype=np.int32) for k in ("record", "episodes", "steps", "idle")}
        L.check(self._lib.dat_episode_slots(self._h, L.ptr(o["record"], L.I), L.ptr(o["episodes"], L.I),
                                            L.ptr(o["steps"], L.I), L.ptr(o["idle"], L.I)))
        o["idle"] = o["idle"].astype(bool)
        return o

    def episodes_respawns(self) -> Tuple[int, int, int]:
        """(respawns by the early pass: 0 by construction, respawns by every other pass, ending scenarios the early
        gate left to the rest pass) since episodes_begin -- dat_get_episode_respawns."""
        e, r, d = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_get_episode_respawns(self._h, ctypes.byref(e), ctypes.byref(r), ctypes.byref(d)))
        return e.value, r.value, d.value

    # -- the closed loop's log (dat_log_*): closed_loop records into HBM, log_read copies the records out
    def log_begin(self, scenarios=None, log_every: Optional[int] = None, hl_capacity: int = 100,
                  summary: bool = False) -> None:
        """Open a log: closed_loop then keeps, for `scenarios` (strictly increasing indices; None: all, []: none),
        an HL record per control step and a step record at every simulation step i with i % log_every == 0
        (log_every: the reference's log_freq, default hl_every), and with summary=True the per-step iters,
        min_env_dist and collision of all scenarios.  The buffers hold hl_capacity HL steps; a closed_loop call
        that would pass it raises DatError (log_read, log_clear, then go on).  control, control_steps, rollout,
        rp_rollout, pmrl_rollout and pmrl_forward are not recorded."""
        if scenarios is None:
            sc, count = None, self.batch
        else:
            sc = L.i32(np.asarray(scenarios).reshape(-1))
            count = sc.shape[0]
        le = int(self.cfg.hl_every if log_every is None else log_every)
        L.check(self._lib.dat_log_begin(self._h, L.ptr(sc, L.I) if count else None, count, le, int(hl_capacity),
                                        int(summary)))
        self._log = (np.arange(self.batch, dtype=np.int32) if sc is None else sc, bool(summary))

    def log_counts(self) -> tuple:
        """(HL records held, step records held, log clock in simulation steps) -- dat_log_counts."""
        k, s, c = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_log_counts(self._h, ctypes.byref(k), ctypes.byref(s), ctypes.byref(c)))
        return k.value, s.value, c.value

    def log_read(self) -> dict:
        """The records held, time-major numpy arrays (R recorded scenarios, K HL records, Ks step records):
        scenarios (R,); HL: f_des (K, R, 3, n), iters (K, R), qp_status (K, R, n), min_env_dist (K, R), collision
        (K, R) bool, x_ref, v_ref (K, R, 3), solve_ms (K,) (NaN with sub-batch streams); steps: step_index (Ks,),
        thrust (Ks, R, n), moment (Ks, R, 3, n), state (Ks, R, 12n + 18), x_err, v_err (Ks, R); with the summary
        tier: sum_iters, sum_min_env_dist, sum_collision (K, B)."""
        if getattr(self, "_log", None) is None:
            raise L.DatError("log_read: no log open")
        scen, summary = self._log
        n, B, R = self.n, self.batch, scen.shape[0]
        K, Ks, _ = self.log_counts()
        f = np.empty((K, R, n, 3))
        it = np.empty((K, R), dtype=np.int32)
        qs = np.empty((K, R, n), dtype=np.int32)
        md = np.empty((K, R))
        col = np.empty((K, R), dtype=np.uint8)
        xr, vr, ms = np.empty((K, R, 3)), np.empty((K, R, 3)), np.empty(K)
        L.check(self._lib.dat_log_read_hl(self._h, 0, K, L.ptr(f), L.ptr(it, L.I), L.ptr(qs, L.I), L.ptr(md),
                                          L.ptr(col, L.U8), L.ptr(xr), L.ptr(vr), L.ptr(ms)))
        si = np.empty(Ks, dtype=np.int64)
        th, mo = np.empty((Ks, R, n)), np.empty((Ks, R, n, 3))
        st = np.empty((Ks, R, layout.state_size(n)))
        xe, ve = np.empty((Ks, R)), np.empty((Ks, R))
        L.check(self._lib.dat_log_read_steps(self._h, 0, Ks, L.ptr(si, L.LL), L.ptr(th), L.ptr(mo), L.ptr(st),
                                             L.ptr(xe), L.ptr(ve)))
        out = {"scenarios": scen.copy(), "f_des": f.transpose(0, 1, 3, 2), "iters": it, "qp_status": qs,
               "min_env_dist": md, "collision": col.astype(bool), "x_ref": xr, "v_ref": vr, "solve_ms": ms,
               "step_index": si, "thrust": th, "moment": mo.transpose(0, 1, 3, 2), "state": st, "x_err": xe,
               "v_err": ve}
        if summary:
            sit = np.empty((K, B), dtype=np.int32)
            smd = np.empty((K, B))
            sco = np.empty((K, B), dtype=np.uint8)
            L.check(self._lib.dat_log_read_summary(self._h, 0, K, L.ptr(sit, L.I), L.ptr(smd), L.ptr(sco, L.U8)))
            out.update(sum_iters=sit, sum_min_env_dist=smd, sum_collision=sco.astype(bool))
        return out

    def log_clear(self) -> None:
        """Empty the log's buffers and keep its clock (dat_log_clear)."""
        L.check(self._lib.dat_log_clear(self._h))

    def log_end(self) -> None:
        """Close the log and free its buffers (dat_log_end)."""
        L.check(self._lib.dat_log_end(self._h))
        self._log = None

    def control_steps(self, acc_seq: np.ndarray) -> StepResult:
        """dat_control_steps: acc_seq (K, B, 6) -> K fused control steps of every scenario from the resident
        states (C-ADMM / DD without a forest); the result holds the last step's outputs.  The fused path
        evaluates no environment rows: min_env_dist is NaN and collision None (not computed)."""
        acc_seq = L.f64(acc_seq)
        K = acc_seq.shape[0]
        assert acc_seq.shape[1:] == (self.batch, 6), acc_seq.shape
        f = np.zeros((self.batch, 3 * self.n))
        it = np.zeros(self.batch, dtype=np.int32)
        qs = np.zeros((self.batch, self.n), dtype=np.int32)
        L.check(self._lib.dat_control_steps(self._h, int(K), L.ptr(acc_seq), L.ptr(f), L.ptr(it, L.I),
                                            L.ptr(qs, L.I)))
        return StepResult(f.reshape(self.batch, self.n, 3).transpose(0, 2, 1).copy(), it, qs,
                          np.full(self.batch, np.nan), None)

    def step_marks(self) -> np.ndarray:
        """Host clock marks [ms] of the last closed_loop call (dat_get_step_marks): its start, then each
        HL step's control-kernel completion.  With sub-batch streams (set_sub_batches > 1) only the run's
        start and end: np.diff gives one whole-run time, not per-step times."""
        m = self._lib.dat_get_step_marks(self._h, None, 0)
        if m < 0:
            L.check(m)
        out = np.zeros(m)
        self._lib.dat_get_step_marks(self._h, L.ptr(out), m)
        return out

    def env_rows(self):
        B, n = self.batch, self.n
        lhs = np.empty((B, n, layout.NENV, 3))
        rhs = np.empty((B, n, layout.NENV))
        nr = np.empty((B, n), dtype=np.int32)
        col = np.empty((B, n), dtype=np.uint8)
        md = np.empty((B, n))
        L.check(self._lib.dat_env_rows(self._h, L.ptr(lhs), L.ptr(rhs), L.ptr(nr, L.I), L.ptr(col, L.U8), L.ptr(md)))
        return lhs, rhs, nr, col.astype(bool), md

    def solve_agent_qps(self, scenario, agent, acc_des, lam=None, rho=None, f_mean=None, c=None, env_lhs=None,
                        env_rhs=None, nenv=None) -> dict:
        """Raw batched agent QPs (dat_solve_agent_qp_batch): RQPPrimalSolver.solve of C-ADMM
        (control/rqp_cadmm.py:482-501; lam, f_mean (K, 3, n), rho (K,)) or DD (control/rqp_dd.py:475-505;
        c (K, 9) = (c_fi, c_Fi, c_Mi)) at the handle's current states.  Returns x ((K, 3, n) C-ADMM copies
        f, or (K, 9) DD (f_i, F_i, M_i)), status, ipm_iters, collision, min_env_dist.

        env_lhs=, env_rhs= (dat_solve_agent_qp_rows_batch): the caller's env rows lhs . dvl >= rhs instead of the
        forest query -- K arrays (k_i, 3) and (k_i,), k_i <= 10, or compacted blocks (K, 10, 3) and (K, 10) with
        nenv (K,).  The result then also holds certified (K,): the Farkas certificate on the dvl rows decided the
        item (status INFEASIBLE, 0 IPM iterations); collision is False and min_env_dist +inf."""
        n = self.n
        sc, ag = L.i32(np.atleast_1d(scenario)), L.i32(np.atleast_1d(agent))
        K = sc.shape[0]
        acc = L.f64(acc_des).reshape(K, 6)
        dd = self.mode == L.MODE_DD
        if dd:
            cc = L.f64(c).reshape(K, 9)
            la = rh = fm = None
            x = np.empty((K, 9))
        else:
            cc = None
            la = L.f64(np.asarray(lam, float).reshape(K, 3, n).transpose(0, 2, 1).reshape(K, 3 * n))
            fm = L.f64(np.asarray(f_mean, float).reshape(K, 3, n).transpose(0, 2, 1).reshape(K, 3 * n))
            rh = L.f64(np.broadcast_to(np.asarray(rho, float), (K,)))
            x = np.empty((K, 3 * n))
        st = np.empty(K, dtype=np.int32)
        it = np.empty(K, dtype=np.int32)
        col = np.empty(K, dtype=np.uint8)
        md = np.empty(K)
        cert = None
        if env_lhs is None:
            assert env_rhs is None and nenv is None
            L.check(self._lib.dat_solve_agent_qp_batch(self._h, K, L.ptr(sc, L.I), L.ptr(ag, L.I), L.ptr(acc),
                                                       L.ptr(la), L.ptr(rh), L.ptr(fm), L.ptr(cc), L.ptr(x),
                                                       L.ptr(st, L.I), L.ptr(it, L.I), L.ptr(col, L.U8), L.ptr(md)))
        else:
            if nenv is None:
                assert len(env_lhs) == K and len(env_rhs) == K
                ne = L.i32([np.asarray(r, float).reshape(-1).shape[0] for r in env_rhs])
                assert ne.max(initial=0) <= layout.NENV
                el, er = np.zeros((K, layout.NENV, 3)), np.zeros((K, layout.NENV))
                for k in range(K):
                    el[k, :ne[k]] = np.asarray(env_lhs[k], float).reshape(ne[k], 3)
                    er[k, :ne[k]] = np.asarray(env_rhs[k], float).reshape(ne[k])
            else:
                ne = L.i32(nenv).reshape(K)
                el, er = L.f64(env_lhs).reshape(K, layout.NENV, 3), L.f64(env_rhs).reshape(K, layout.NENV)
            cert = np.zeros(K, dtype=np.uint8)
            L.check(self._lib.dat_solve_agent_qp_rows_batch(self._h, K, L.ptr(sc, L.I), L.ptr(ag, L.I), L.ptr(acc),
                                                            L.ptr(la), L.ptr(rh), L.ptr(fm), L.ptr(cc), L.ptr(el),
                                                            L.ptr(er), L.ptr(ne, L.I), L.ptr(x), L.ptr(st, L.I),
                                                            L.ptr(it, L.I), L.ptr(col, L.U8), L.ptr(md),
                                                            L.ptr(cert, L.U8)))
        if not dd:
            x = x.reshape(K, n, 3).transpose(0, 2, 1)
        out = {"x": x, "status": st, "ipm_iters": it, "collision": col.astype(bool), "min_env_dist": md}
        if cert is not None:
            out["certified"] = cert.astype(bool)
        return out

    def counters(self):
        """(agent-QP solves, IPM iterations, HL steps, summed HL kernel ms) since the last reset."""
        w = self.work()
        return w["qp_solves"], w["ipm_iters"], w["hl_steps"], w["hl_kernel_ms"]

    def work(self) -> dict:
        """Device work counters since the last reset (dat_get_counters)."""
        q, it, rw, hs, ms = (ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(),
                             ctypes.c_double())
        L.check(self._lib.dat_get_counters(self._h, ctypes.byref(q), ctypes.byref(it), ctypes.byref(rw),
                                           ctypes.byref(hs), ctypes.byref(ms)))
        ib, lo = ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_get_inband_exits(self._h, ctypes.byref(ib), ctypes.byref(lo)))
        rp, rc = ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_get_refinement_counters(self._h, ctypes.byref(rp), ctypes.byref(rc)))
        rr = ctypes.c_longlong()
        if hasattr(self._lib, "dat_get_robust_redos"):  # absent only from an older A/B build (DAT_LIB_PATH)
            L.check(self._lib.dat_get_robust_redos(self._h, ctypes.byref(rr)))
        out = {"qp_solves": q.value, "ipm_iters": it.value, "ipm_row_iters": rw.value, "hl_steps": hs.value,
               "hl_kernel_ms": ms.value, "inband_exits": ib.value, "inband_beyond_clarabel_tol": lo.value,
               "refine_passes": rp.value, "refine_corrections": rc.value, "robust_redos": rr.value}
        if hasattr(self._lib, "dat_get_tail_counters"):  # absent only from an older A/B build (DAT_LIB_PATH)
            tc = (ctypes.c_longlong * 6)()
            L.check(self._lib.dat_get_tail_counters(self._h, tc))
            out.update(tail_passes=tc[0], tail_critical_ipm_iters=tc[1], tail_routed=tc[2], certified_infeasible=tc[3],
                       stall_exits=tc[4], warm_starts=tc[5])
            col, md = ctypes.c_longlong(), ctypes.c_double()
            L.check(self._lib.dat_get_collision_stats(self._h, ctypes.byref(col), ctypes.byref(md)))
            out.update(collisions=col.value, min_env_dist=md.value)
        return out

    def agent_qp_ms(self) -> float:
        """Device time of the last solve_agent_qps launch (dat_get_agent_qp_ms)."""
        ms = ctypes.c_double()
        L.check(self._lib.dat_get_agent_qp_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def class_work(self, env_class: int) -> dict:
        """C-ADMM only: work counters, summed kernel time and SIMD occupancy of one env class (0:
        scenarios whose agent QPs carry no env CBF row in the step; 1, 2, 3: at most 2, 5, 10 env rows
        per agent QP) -- dat_get_class_counters, dat_get_class_occupancy."""
        q, it, rw, ms = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
        L.check(self._lib.dat_get_class_counters(self._h, int(env_class), ctypes.byref(q), ctypes.byref(it),
                                                 ctypes.byref(rw), ctypes.byref(ms)))
        sl, wp = ctypes.c_longlong(), ctypes.c_longlong()
        L.check(self._lib.dat_get_class_occupancy(self._h, int(env_class), ctypes.byref(sl), ctypes.byref(wp)))
        return {"qp_solves": q.value, "ipm_iters": it.value, "ipm_row_iters": rw.value, "kernel_ms": ms.value,
                "slot_ipm_iters": sl.value, "wave_admm_iters": wp.value}

    def kernel_ms(self) -> float:
        """Summed device time of k_cadmm / k_dd since the last counter reset (dat_get_kernel_ms)."""
        ms = ctypes.c_double()
        L.check(self._lib.dat_get_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def reset_counters(self) -> None:
        L.check(self._lib.dat_reset_counters(self._h))

    def synchronize(self) -> None:
        L.check(self._lib.dat_synchronize(self._h))


# ================================================================================================
# drop-in single-scenario controllers
# ================================================================================================
class _DropIn:
    _mode = None

    def __init__(self, params: RQPParameters, col: RQPCollision, state: RQPState, dt: float, env: Any = None,
                 verbose: bool = False, device: int = 0) -> None:
        assert params.n >= 3
        self.n = params.n
        self.params, self.col, self.dt, self.env, self.verbose = params, col, dt, env, verbose
        self.max_f_ang = np.pi / 6.0
        self.dist_eps = 0.1
        self.vision_radius = col.collision_radius + 5.0
        self._eng = BatchedController(self._mode, self.n, 1, pack_params(params, col), dt=dt, device=device,
                                      record_err=self._mode != L.MODE_CENTRALIZED)
        if env is not None:
            self._eng.set_forests([env])

    def control(self, state, acc_des):
        acc = np.concatenate([np.asarray(acc_des[0], float), np.asarray(acc_des[1], float)])[None]
        r = self._eng.control(pack_state(state)[None], acc)
        f = r.f_des[0]
        if self._mode == L.MODE_CENTRALIZED:
            return f, SolverStatistics(-1, r.gpu_ms * 1e-3, bool(r.collision[0]), float(r.min_env_dist[0]))
        it = int(r.iters[0])
        err = r.err_seq[0][: max(it - 1, 0)].tolist() if r.err_seq is not None else []
        err = [e for e in err if e == e]
        return f, SolverStatistics(it, r.gpu_ms * 1e-3, bool(r.collision[0]), float(r.min_env_dist[0]), err)

    def set_qp_tolerance(self, tol: float) -> None:
        """Extension (no reference counterpart): IPM stopping tolerance, 1e-8 = Clarabel's default."""
        self._eng.set_qp_tolerance(tol)

    def _warm(self) -> dict:
        """The scenario's checkpoint record (Checkpoint.arrays of a one-scenario checkpoint), record axis dropped."""
        return {k: v[0] for k, v in self._eng.checkpoint([0]).arrays().items()}

    def get_force_cone_angle_bound(self) -> float:
        return self.max_f_ang

    def get_dist_eps(self) -> float:
        return self.dist_eps


class RQPCentralizedController(_DropIn):
    _mode = L.MODE_CENTRALIZED

    @property
    def prev_f(self) -> np.ndarray:
        """(3, n): the solution held on a non-OPTIMAL solve (control/rqp_centralized.py prev_f), read-only."""
        return self._warm()["prev_f"].T.copy()


class RQPCADMMController(_DropIn):
    _mode = L.MODE_CADMM

    # The warm state the reference keeps as attributes (control/rqp_cadmm.py:569-580), read from the device through a
    # one-scenario checkpoint; read-only (BatchedController.restore writes warm state).
    @property
    def f(self) -> np.ndarray:
        """(3, n, n): f[:, :, i] is agent i's copy."""
        return self._warm()["f"].transpose(2, 1, 0).copy()

    @property
    def f_mean(self) -> np.ndarray:
        return self._warm()["f_mean"].T.copy()

    @property
    def lambda_f(self) -> np.ndarray:
        """(3, n, n): lambda_f[:, :, i] is agent i's multiplier."""
        return self._warm()["lambda_f"].transpose(2, 1, 0).copy()

    def set_force_err_tolerance(self, tol: float, use_total_res: bool = True) -> None:
        self._eng.set_force_err_tolerance(tol, use_total_res)

    def set_max_iter(self, max_iter: int) -> None:
        self._eng.set_max_iter(max_iter)


class RQPDDController(_DropIn):
    _mode = L.MODE_DD

    # control/rqp_dd.py:618-632, read from the device through a one-scenario checkpoint; read-only.  f, F, M: the
    # agents' held solutions (f_i, F_i, M_i), each (3, n) with column i agent i's.
    @property
    def f(self) -> np.ndarray:
        return self._warm()["prev"][:, 0:3].T.copy()

    @property
    def F(self) -> np.ndarray:
        return self._warm()["prev"][:, 3:6].T.copy()

    @property
    def M(self) -> np.ndarray:
        return self._warm()["prev"][:, 6:9].T.copy()

    @property
    def lambda_F(self) -> np.ndarray:
        return self._warm()["lambda_F"].T.copy()

    @property
    def lambda_M(self) -> np.ndarray:
        return self._warm()["lambda_M"].T.copy()

    def set_force_err_tolerance(self, tol: float) -> None:
        self._eng.set_force_err_tolerance(tol, True)

    def set_max_iter(self, max_iter: int) -> None:
        self._eng.set_max_iter(max_iter)


class _PrimalSolver:
    """One agent's QP solver with the reference's per-call interface and status handling, solved by
    k_agent_qp through dat_solve_agent_qp_batch.  ``idx`` is the reference's Index(i, is_leader) or a
    plain agent number; agent 0 is the leader (control/rqp_cadmm.py:553-555; set_leader after
    construction does not change the cost weights)."""

    _mode = None

    def __init__(self, params: RQPParameters, col: RQPCollision, idx: Any, state: RQPState, dt: float,
                 env: Any = None, verbose: bool = False, device: int = 0) -> None:
        assert params.n >= 3
        self.n = params.n
        self.i = int(getattr(idx, "i", idx))
        self.verbose = verbose
        self.params = params
        self._eng = BatchedController(self._mode, self.n, 1, pack_params(params, col), dt=dt, device=device)
        if env is not None:
            self._eng.set_forests([env])
        self.f_eq = equilibrium_forces(params)
        self.collision, self.min_env_dist = False, col.collision_radius + 5.0
        self._set_warm_start()

    def _run(self, state, acc_des, **kw):
        self._eng.set_state(pack_state(state)[None])
        acc = np.concatenate([np.asarray(acc_des[0], float), np.asarray(acc_des[1], float)])[None]
        r = self._eng.solve_agent_qps([0], [self.i], acc, **kw)
        self.collision, self.min_env_dist = bool(r["collision"][0]), float(r["min_env_dist"][0])
        if self.verbose and r["status"][0] != L.QP_OPTIMAL:
            print(f"Problem not solved to optimality, status: {int(r['status'][0])}")
        # solve_time [s]: the device time of the QP kernel, as Clarabel's solver_stats.solve_time is the
        # solver's own time (control/rqp_cadmm.py:500)
        return r, self._eng.agent_qp_ms() * 1e-3


class RQPCADMMPrimalSolver(_PrimalSolver):
    """control/rqp_cadmm.py:26-507: solve(state, acc_des, lambda_f, cadmm_rho, f_mean) ->
    (f (3, n), solve_time, collision, min_env_dist).  Exception -> f_eq (:491-494); non-OPTIMAL ->
    previous solution (:496-499).  The reference's default cadmm_rho = 0 (:487) is used only by its
    constructor's warm-up solve (:131-140), where the copies f_j, j != i, are not unique (that solve only seeds
    Clarabel's warm start); here cadmm_rho defaults to the controller's initial penalty rho0 = 1
    (control/rqp_cadmm.py:564), and an explicit rho <= 0 raises ValueError instead of silently solving another
    QP."""

    _mode = L.MODE_CADMM

    def _set_warm_start(self) -> None:
        self.prev_f = self.f_eq.copy()

    RHO0 = 1.0  # RQPCADMMController.rho0 (control/rqp_cadmm.py:564)

    def solve(self, state, acc_des, lambda_f=None, cadmm_rho: Optional[float] = None, f_mean=None):
        n = self.n
        if cadmm_rho is None:
            cadmm_rho = self.RHO0
        if not float(cadmm_rho) > 0.0:
            raise ValueError(f"cadmm_rho must be > 0 (got {cadmm_rho}): at rho = 0 the agent QP's copies f_j, "
                             "j != i, are not unique (the reference uses rho = 0 only for its constructor's "
                             "warm-up solve, control/rqp_cadmm.py:131-140)")
        lam = np.zeros((3, n)) if lambda_f is None else np.asarray(lambda_f, float)
        fm = np.zeros((3, n)) if f_mean is None else np.asarray(f_mean, float)
        r, t = self._run(state, acc_des, lam=lam[None], rho=[cadmm_rho], f_mean=fm[None])
        st = int(r["status"][0])
        if st == L.QP_FAILED:
            self.prev_f = self.f_eq.copy()
        elif st == L.QP_OPTIMAL:
            self.prev_f = r["x"][0].copy()
        return self.prev_f, t, self.collision, self.min_env_dist


class RQPDDPrimalSolver(_PrimalSolver):
    """control/rqp_dd.py:27-511: solve(state, acc_des, c_fi, c_Fi, c_Mi) -> (f_i, F_i, M_i, solve_time,
    collision, min_env_dist).  Exception -> (f_eq,i, sum f_eq - f_eq,i, -JT^-1 hat(r_com,i) f_eq,i)
    (:484-489); non-OPTIMAL -> previous solution."""

    _mode = L.MODE_DD

    def _set_warm_start(self) -> None:
        p, i = self.params, self.i
        self.prev_fi = self.f_eq[:, i].copy()
        self.prev_Fi = np.sum(self.f_eq, axis=1) - self.prev_fi
        self.prev_Mi = -p.JT_inv @ _skew(p.r_com[:, i]) @ self.prev_fi

    def solve(self, state, acc_des, c_fi=np.zeros(3), c_Fi=np.zeros(3), c_Mi=np.zeros(3)):
        c = np.concatenate([np.asarray(c_fi, float), np.asarray(c_Fi, float), np.asarray(c_Mi, float)])
        r, t = self._run(state, acc_des, c=c[None])
        st = int(r["status"][0])
        if st == L.QP_FAILED:
            self._set_warm_start()
        elif st == L.QP_OPTIMAL:
            x = r["x"][0]
            self.prev_fi, self.prev_Fi, self.prev_Mi = x[:3].copy(), x[3:6].copy(), x[6:].copy()
        return self.prev_fi, self.prev_Fi, self.prev_Mi, t, self.collision, self.min_env_dist


class RQPLowLevelController:
    """control/rqp_centralized.py:457-535: RQPLowLevelController(so3_controller_type, params, max_f_ang)
    .control(state, f_des) -> (f (n,), M (3, n)); "pd" or "sm" SO(3) law, evaluated on the GPU
    (k_low_level).  Unknown types raise NotImplementedError like the reference (:483-484)."""

    def __init__(self, so3_controller_type: str, params: RQPParameters, max_f_ang: float, device: int = 0) -> None:
        if so3_controller_type not in L.LL_KINDS:
            raise NotImplementedError(so3_controller_type)
        self.n = params.n
        self.cos_max_f_ang = np.cos(max_f_ang)
        col = RQPCollision(np.zeros((1, 3)), np.zeros((1, 3)))  # the LL law reads only J
        self._eng = BatchedController(L.MODE_CADMM, self.n, 1, pack_params(params, col), device=device)
        self._eng.set_low_level(so3_controller_type)

    def control(self, state, f_des: np.ndarray):
        f_des = np.asarray(f_des, float)
        assert f_des.shape == (3, state.n)
        assert all(f_des[2, :] > 0.0)
        self._eng.set_state(pack_state(state)[None])
        f, M = self._eng.low_level(f_des[None])
        return f[0], M[0]


class RQPClosedLoop:
    """One scenario's closed loop on the GPU (example/rqp_example.py:120-131): HL control every
    ``hl_rel_freq`` steps from the given desired accelerations, SO(3) PD low level and dynamics
    at every step.  ``step(acc_des)`` advances one high-level period."""

    def __init__(self, controller: _DropIn, state: RQPState, hl_rel_freq: int = 10) -> None:
        self.ctrl = controller
        self.hl = hl_rel_freq
        self.ctrl._eng.set_state(pack_state(state)[None], np.zeros(1, dtype=np.int32))

    def step(self, acc_des=None):
        eng = self.ctrl._eng
        acc = None
        if acc_des is not None:
            acc = np.concatenate([np.asarray(acc_des[0], float), np.asarray(acc_des[1], float)])[None]
        r = eng.control(None, acc)
        eng.rollout(self.hl)
        return r

    @property
    def state(self) -> RQPState:
        st, _ = self.ctrl._eng.get_state()
        return RQPState.unpack(st[0], self.ctrl.n)


__all__ = ["BatchedController", "Checkpoint", "StepResult", "SolverStatistics", "RQPCentralizedController", "RQPCADMMController",
           "RQPDDController", "RQPClosedLoop", "RQPCADMMPrimalSolver", "RQPDDPrimalSolver", "RQPLowLevelController"]
