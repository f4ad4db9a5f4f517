"""The reference's forest example on the GPU, with its log format and statistics printout.

``simulate`` reproduces example/rqp_example.py:main (:83-165) -- HL control every ``hl_rel_freq``
steps from the forest desired-acceleration law (:33-59), the LL SO(3) law and the dynamics at every
step -- with every piece on the device (k_desired, the controller kernels, k_low_level, k_rollout),
and returns the ``logs`` dict of :141-165 with the same keys, element types and logging instants:

    n, dt, T, hl_rel_freq, log_freq, num_trees, tree_pos, controller_type,
    state_seq (RQPStateData after step i), x_err_seq, v_err_seq (|x_ref - xl|, |v_ref - vl| after step i),
    f_des_seq (3, n), iter_seq (not for centralized), solve_time_seq [s], min_env_dist_seq,
    w_seq ((f (n,), M (3, n)) applied at step i),      logged at i % log_freq == 0

so example/rqp_plots.py (:494-521) can read a GPU run (``save_logs`` writes the pickle it loads).
``simulate_batch`` runs B scenarios at once (different forests / start states) and returns one such
dict per scenario.  ``print_stats`` is ``_print_stats`` (:62-80) with the same format.
"""

from __future__ import annotations

import pickle
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import layout, scenarios, tracking
from .env_forest import Forest
from .system import RQPState, pack_state

CONTROLLER_TYPES = ("centralized", "dual-decomposition", "consensus-admm")
LAWS = ("forest", "circle")


@dataclass
class RQPStateData:
    """example/rqp_example.py:23-30."""

    R: np.ndarray
    w: np.ndarray
    xl: np.ndarray
    vl: np.ndarray
    Rl: np.ndarray
    wl: np.ndarray


def compute_aggregate_statistics(a: np.ndarray):
    """utils/math_utils.py:63-73: min, max, avg, std along axis 0."""
    return np.min(a, axis=0), np.max(a, axis=0), np.mean(a, axis=0), np.std(a, axis=0)


def print_stats(iter: List[int], solve_time: List[float]) -> None:  # noqa: A002 -- the reference's name
    """example/rqp_example.py:62-80."""
    if len(iter) > 0:
        s = compute_aggregate_statistics(np.array(iter))
        print(f"Solver iterations: min: {s[0]:5.2f}, max: {s[1]:5.2f}, avg: {s[2]:5.2f}, std: {s[3]:5.2f}")
    if len(solve_time) > 0:
        s = compute_aggregate_statistics(np.array(solve_time))
        print(f"Solver solve time (ms): min: {s[0] * 1e3:7.3f}, max: {s[1] * 1e3:7.3f}, avg: {s[2] * 1e3:7.3f}, "
              f"std: {s[3] * 1e3:7.3f}")


def save_logs(logs: dict, file_name: str) -> None:
    """The pickle example/rqp_example.py:167-170 writes (logs/rqp_forest_<controller_type>.pkl)."""
    with open(file_name, "wb") as f:
        pickle.dump(logs, f)


def references(xl: np.ndarray, forest) -> tuple:
    """x_ref, v_ref of _desired_acceleration_forest (example/rqp_example.py:36-48) for positions xl (B, 3)."""
    xl = np.atleast_2d(xl)
    x_ref = np.zeros_like(xl)
    x_ref[:, 0] = xl[:, 0] + 1.5
    nrm = np.linalg.norm(xl[:, :2] - np.asarray(forest.mountain_center), axis=1)
    inside = nrm < forest.mountain_radius
    x_ref[:, 2] = 1.5
    x_ref[inside, 2] = (np.sqrt(forest.mountain_sphere_radius ** 2 - nrm[inside] ** 2) - forest.mountain_center_depth
                        + 1.5)
    v_ref = np.tile([0.5, 0.0, 0.0], (xl.shape[0], 1))
    return x_ref, v_ref


LOG_ARRAYS_HL = ("f_des", "iters", "min_env_dist", "solve_ms")
LOG_ARRAYS_STEP = ("thrust", "moment", "state", "x_err", "v_err")


def logs_from_arrays(headers: List[dict], arrays: dict, n: int) -> List[dict]:
    """The reference's logs dicts (example/rqp_example.py:141-160) from the time-major arrays of
    ``BatchedController.log_read`` (several reads concatenated along axis 0): headers[r] holds the run's
    constants of recorded scenario r (n, dt, T, ..., controller_type), arrays the keys LOG_ARRAYS_HL
    ((K, R, ...), solve_ms (K,)) and LOG_ARRAYS_STEP ((Ks, R, ...)).  Pure: every field is sliced out of the
    whole arrays at once; only the per-record objects the format asks for (a list entry, an RQPStateData) are
    made one by one."""
    st = np.asarray(arrays["state"])
    Ks, R = st.shape[:2]
    o = {k: layout.s_off(k, n) for k in ("R", "W", "XL", "VL", "RL", "WL")}
    Rq = st[..., o["R"]:o["R"] + 9 * n].reshape(Ks, R, n, 3, 3).transpose(1, 0, 3, 4, 2).copy()
    wq = st[..., o["W"]:o["W"] + 3 * n].reshape(Ks, R, n, 3).transpose(1, 0, 3, 2).copy()
    xl = st[..., o["XL"]:o["XL"] + 3].transpose(1, 0, 2).copy()
    vl = st[..., o["VL"]:o["VL"] + 3].transpose(1, 0, 2).copy()
    Rl = st[..., o["RL"]:o["RL"] + 9].reshape(Ks, R, 3, 3).transpose(1, 0, 2, 3).copy()
    wl = st[..., o["WL"]:o["WL"] + 3].transpose(1, 0, 2).copy()
    # scenario-major copies: logs[r]'s entries are views of row r
    f_des = np.swapaxes(np.asarray(arrays["f_des"]), 0, 1).copy()
    thrust = np.swapaxes(np.asarray(arrays["thrust"]), 0, 1).copy()
    moment = np.swapaxes(np.asarray(arrays["moment"]), 0, 1).copy()
    iters = np.asarray(arrays["iters"]).T
    min_env_dist = np.asarray(arrays["min_env_dist"], float).T.tolist()
    x_err = np.asarray(arrays["x_err"], float).T.tolist()
    v_err = np.asarray(arrays["v_err"], float).T.tolist()
    solve_time = (np.asarray(arrays["solve_ms"], float) * 1e-3).tolist()
    logs = []
    for r in range(R):
        lg = dict(headers[r])
        lg["state_seq"] = [RQPStateData(*s) for s in zip(Rq[r], wq[r], xl[r], vl[r], Rl[r], wl[r])]
        lg["x_err_seq"] = x_err[r]
        lg["v_err_seq"] = v_err[r]
        lg["f_des_seq"] = list(f_des[r])
        lg["iter_seq"] = iters[r][iters[r] != -1].tolist()  # centralized: no iteration count (:126-127)
        lg["solve_time_seq"] = list(solve_time)
        lg["min_env_dist_seq"] = min_env_dist[r]
        lg["w_seq"] = list(zip(thrust[r], moment[r]))
        logs.append(lg)
    return logs


def _simulate_resident(eng, headers: List[dict], n: int, hl_steps: int, log_freq: int, record, chunk_hl: int,
                       hl_rel_freq: int, dt: float, progress: bool) -> List[dict]:
    """The loop on dat_closed_loop, recorded on the device: chunks of chunk_hl HL steps, each read out and cleared."""
    chunk_hl = max(1, min(int(chunk_hl), hl_steps))
    eng.log_begin(record, log_every=log_freq, hl_capacity=chunk_hl)
    parts = []
    done = 0
    while done < hl_steps or not parts:
        k = min(chunk_hl, hl_steps - done)
        eng.closed_loop(k)
        parts.append(eng.log_read())
        eng.log_clear()
        done += k
        if progress:
            print(f"t = {done * hl_rel_freq * dt:.2f} s", flush=True)
    eng.log_end()
    arrays = {k: np.concatenate([p[k] for p in parts]) for k in LOG_ARRAYS_HL + LOG_ARRAYS_STEP}
    return logs_from_arrays([headers[b] for b in parts[0]["scenarios"]], arrays, n)


def simulate_batch(controller_type: str, states: np.ndarray, forests: list, scenario_forest=None, n: int = 3,
                   T: float = 100.0, dt: float = 1e-3, hl_rel_freq: int = 10, log_freq: Optional[int] = None,
                   so3_controller_type: str = "pd", params: Optional[np.ndarray] = None, device: int = 0,
                   progress: bool = False, resident: bool = False, record=None, chunk_hl: int = 100,
                   law: str = "forest", track: Optional[np.ndarray] = None) -> List[dict]:
    """B closed loops of example/rqp_example.py:main on one GPU; states (B, 12n + 18) (packed
    RQPState), forests[scenario_forest[b]] the forest of scenario b.  Returns one logs dict per scenario.

    resident=True runs the loop on the device-resident closed loop (dat_closed_loop) and has it record the logs
    in HBM (dat_log_*): nothing is copied per step, the records are read every chunk_hl HL steps.  record: the
    scenarios whose dicts are returned (strictly increasing indices; default all).  The resident loop runs whole
    HL periods: a step count that is no multiple of hl_rel_freq raises ValueError.  The default (resident=False)
    drives the loop from the host step by step and returns every scenario's dict.

    law: "forest" (example/rqp_example.py:33-59) or "circle", the reference's trajectory-tracking law
    (test/control/test_rqpcontrollers.py:24-48; tracking.py) at t = i dt, with `track` its records ((TRACK_SIZE,) or
    (B, TRACK_SIZE); default the reference's circle); forests may then be empty.  Both paths honour it, and the logs'
    x_err_seq / v_err_seq are taken against the law's own references."""
    from .control import BatchedController

    if controller_type not in CONTROLLER_TYPES:
        raise NotImplementedError(controller_type)
    if law not in LAWS:
        raise NotImplementedError(law)
    log_freq = hl_rel_freq if log_freq is None else log_freq
    states = np.atleast_2d(np.asarray(states, float))
    B = states.shape[0]
    sf = np.zeros(B, dtype=np.int32) if scenario_forest is None else np.asarray(scenario_forest, dtype=np.int32)
    prm = scenarios.params_block(n) if params is None else params
    if resident and len(np.arange(0, T, dt)) % hl_rel_freq != 0:
        raise ValueError(f"resident=True runs whole HL periods: {len(np.arange(0, T, dt))} steps (T / dt) is no "
                         f"multiple of hl_rel_freq = {hl_rel_freq}")
    eng = BatchedController(controller_type, n, B, prm, dt=dt, hl_every=hl_rel_freq, device=device)
    eng.set_forests(forests, sf if forests else None)
    rec = None
    if law == "circle":
        rec = tracking.circle_record() if track is None else np.asarray(track, float)
        eng.set_tracking(rec)
    elif not forests:
        raise ValueError('law="forest" needs the forests its references are taken from')
    trees = [(forests[sf[b]].num_trees, forests[sf[b]].tree_pos) if forests else (0, np.zeros((0, 3))) for b in range(B)]
    eng.set_low_level(so3_controller_type)
    eng.set_state(states, np.zeros(B, dtype=np.int32))
    steps = len(np.arange(0, T, dt))  # t_seq = np.arange(0, T, dt) (:107)
    if resident:
        headers = [dict(n=n, dt=dt, T=T, hl_rel_freq=hl_rel_freq, log_freq=log_freq,
                        num_trees=trees[b][0], tree_pos=trees[b][1],
                        controller_type=controller_type) for b in range(B)]
        try:
            return _simulate_resident(eng, headers, n, steps // hl_rel_freq, log_freq, record, chunk_hl, hl_rel_freq,
                                      dt, progress)
        finally:
            eng.close()
    logs = [dict(n=n, dt=dt, T=T, hl_rel_freq=hl_rel_freq, log_freq=log_freq,
                 num_trees=trees[b][0], tree_pos=trees[b][1], controller_type=controller_type,
                 state_seq=[], x_err_seq=[], v_err_seq=[], f_des_seq=[], iter_seq=[], solve_time_seq=[],
                 min_env_dist_seq=[], w_seq=[]) for b in range(B)]
    x_ref = v_ref = None
    i = 0
    while i < steps:
        if i % hl_rel_freq == 0:
            x, _ = eng.get_state()
            x_ref = np.empty((B, 3))
            v_ref = np.empty((B, 3))
            if rec is not None:  # the tracked references at the HL instant (the device's clock reads i)
                x_ref[:], v_ref[:], _ = tracking.references(rec, i * dt)
            else:
                for f in np.unique(sf):
                    idx = np.nonzero(sf == f)[0]
                    x_ref[idx], v_ref[idx] = references(x[idx, 12 * n:12 * n + 3], forests[f])
            r = eng.control(None, None)  # desired acceleration on device (:102-103), then control (:104)
            for b in range(B):
                lg = logs[b]
                lg["f_des_seq"].append(r.f_des[b].copy())
                if r.iters[b] != -1:
                    lg["iter_seq"].append(int(r.iters[b]))
                lg["solve_time_seq"].append(r.gpu_ms * 1e-3)
                lg["min_env_dist_seq"].append(float(r.min_env_dist[b]))
        if i % log_freq == 0:
            fw, Mw = eng.low_level(None)  # the wrench integrated at step i (:111-112)
            eng.rollout(1)
            x, _ = eng.get_state()
            for b in range(B):
                s = RQPState.unpack(x[b], n)
                lg = logs[b]
                lg["w_seq"].append((fw[b].copy(), Mw[b].copy()))
                lg["x_err_seq"].append(float(np.linalg.norm(x_ref[b] - s.xl)))
                lg["v_err_seq"].append(float(np.linalg.norm(v_ref[b] - s.vl)))
                lg["state_seq"].append(RQPStateData(s.R, s.w, s.xl, s.vl, s.Rl, s.wl))
            i += 1
            continue
        # advance to the next control or log instant
        nxt = min(steps, (i // hl_rel_freq + 1) * hl_rel_freq, (i // log_freq + 1) * log_freq)
        eng.rollout(nxt - i)
        i = nxt
        if progress and i % 5000 == 0:
            print(f"t = {i * dt:.0f} s", flush=True)
    eng.close()
    return logs


def simulate(controller_type: str = "dual-decomposition", n: int = 3, T: float = 100.0, dt: float = 1e-3,
             hl_rel_freq: int = 10, log_freq: Optional[int] = None, env=None, state: Optional[RQPState] = None,
             so3_controller_type: str = "pd", device: int = 0, verbose: bool = True, resident: bool = False,
             law: str = "forest", track: Optional[np.ndarray] = None) -> dict:
    """example/rqp_example.py:main on the GPU for one scenario (rqp_setup(n) start state, Forest()
    environment -- pass env = Forest.seeded(s) for a reproducible layout); prints the statistics of
    :140 and returns the logs dict of :141-165.  resident, law, track: as in simulate_batch; under law="circle" no
    forest is made unless env is given."""
    forests = [Forest() if env is None else env] if law == "forest" or env is not None else []
    if state is None:
        _, _, state = scenarios.rqp_setup(n)
    logs = simulate_batch(controller_type, pack_state(state)[None], forests, None, n=n, T=T, dt=dt,
                          hl_rel_freq=hl_rel_freq, log_freq=log_freq, so3_controller_type=so3_controller_type,
                          device=device, resident=resident, law=law, track=track)[0]
    if verbose:
        print_stats(logs["iter_seq"], logs["solve_time_seq"])
    return logs


def monte_carlo(controller_type: str, n: int, starts: np.ndarray, forests: list, rules: dict, batch: int,
                scenario_forest=None, chunk_hl: int = 50, max_hl: int = 100000, dt: float = 1e-3,
                hl_rel_freq: int = 10, params: Optional[np.ndarray] = None, device: int = 0,
                progress: bool = False) -> dict:
    """A Monte Carlo campaign over the P initial conditions starts (P, 12n + 18) on `batch` slots of one GPU, on
    the device-resident loop with episodes (BatchedController.episodes_begin): every start is flown once, from a
    fresh controller, until a rule of `rules` (episodes_begin's keywords: goal_x, max_steps, stall_steps,
    on_collision, bound) ends it; the slot then takes the next start.  forests[scenario_forest[s]] is the forest
    of slot s (default: the first for every slot; [] for none).  The loop runs in calls of chunk_hl HL steps, the
    outcome table read and cleared after each, until every slot is idle (at most max_hl HL steps: the rules must
    end every episode, else RuntimeError).  Returns the outcome table of episodes_read, concatenated and sorted
    by (end tick, slot), with "hl_steps" the HL steps run; record k of the table is starts[record[k]]."""
    from .control import BatchedController

    if controller_type not in CONTROLLER_TYPES:
        raise NotImplementedError(controller_type)
    starts = np.atleast_2d(np.asarray(starts, float))
    P = starts.shape[0]
    if "wrap" in rules:
        raise ValueError("monte_carlo runs every start once: wrap is not a rule of the campaign")
    prm = scenarios.params_block(n) if params is None else params
    eng = BatchedController(controller_type, n, batch, prm, dt=dt, hl_every=hl_rel_freq, device=device)
    try:
        sf = np.zeros(batch, dtype=np.int32) if scenario_forest is None else np.asarray(scenario_forest, np.int32)
        eng.set_forests(forests, sf if forests else None)
        # the pool: P records with the constructor's warm state (the handle's, untouched so far) and the starts
        pool = eng.checkpoint(np.zeros(P, dtype=np.int32))
        arr = pool.arrays()
        arr["state"][:] = starts
        arr["counter"][:] = 0
        eng.episodes_begin(pool, wrap=False, capacity=batch * chunk_hl, **rules)
        parts, done = [], 0
        while eng.episodes_counts()["idle"] < batch:
            if done >= max_hl:
                raise RuntimeError(f"monte_carlo: {max_hl} HL steps run and {eng.episodes_counts()['idle']} of "
                                   f"{batch} slots idle: the rules do not end every episode")
            eng.closed_loop(chunk_hl)
            done += chunk_hl
            parts.append(eng.episodes_read())
            eng.episodes_clear()
            if progress:
                print(f"{done} HL steps: {eng.episodes_counts()}", flush=True)
        eng.episodes_end()
    finally:
        eng.close()
    keys = parts[0].keys() if parts else ()
    out = {k: np.concatenate([p[k] for p in parts]) for k in keys}
    if parts:
        order = np.lexsort((out["slot"], out["end_tick"]))
        out = {k: v[order] for k, v in out.items()}
    out["hl_steps"] = done
    return out


__all__ = ["RQPStateData", "simulate", "simulate_batch", "print_stats", "save_logs", "compute_aggregate_statistics",
           "references", "logs_from_arrays", "monte_carlo"]
