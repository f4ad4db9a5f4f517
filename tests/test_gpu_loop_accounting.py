"""The closed loop's bookkeeping, in each of its schedules (serial, sub-batches, advance overlap) and controller
modes: the step count, the host clock marks, the device times, the advance counts and the log's solve_ms entries
after closed_loop(3) and again after closed_loop(2).  What the loop computes is compared bitwise between the
schedules elsewhere (test_gpu_advance_overlap.py, test_gpu_drain.py, test_gpu_closed_loop_log.py); here only the
accounting around it.  Small shapes: n = 3, 7 scenarios (sub-batches of 1, 2, 2, 2 with four streams) or 5.
"""

import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3
# id: (mode, B, forest, overlap switch, sub-batches)
CASES = {
    "cadmm_overlap": ("cadmm", 7, True, True, 1),
    "cadmm_serial": ("cadmm", 7, True, False, 1),
    "cadmm_sub2": ("cadmm", 7, True, True, 2),
    "cadmm_sub4": ("cadmm", 7, True, True, 4),
    "cadmm_no_forest": ("cadmm", 7, False, False, 1),
    "dd": ("dd", 5, False, True, 1),
    "centralized": ("centralized", 5, False, True, 1),
}


def _engine(mode, B, forest):
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios

    rng = np.random.default_rng(5)
    eng = BatchedController(mode, N, B, scenarios.params_block(N))
    if forest:
        forests, sf = [Forest.seeded(0), Forest.seeded(1)], (np.arange(B) % 2).astype(np.int32)
        eng.set_forests(forests, sf)
        x0 = scenarios.forest_path_states(N, B, rng, forests, sf)
    else:
        x0 = scenarios.perturbed_states(N, B, rng)
    eng.set_state(x0, np.zeros(B, dtype=np.int32))
    return eng


@pytest.mark.parametrize("log", [False, True], ids=["nolog", "log"])
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_loop_accounting(case, log):
    mode, B, forest, overlap, sub = CASES[case]
    runs_overlap = mode == "cadmm" and overlap and sub == 1 and not log  # otherwise the serial schedule, silently
    eng = _engine(mode, B, forest)
    try:
        eng.set_sub_batches(sub)
        eng.set_advance_overlap(overlap)
        if log:
            eng.log_begin(None, hl_capacity=5)
        total = 0
        for steps in (3, 2):
            eng.closed_loop(steps)
            total += steps
            w = eng.work()
            marks = eng.step_marks()
            print(f"{case} log={log}: after {total} steps hl_kernel_ms {w['hl_kernel_ms']:.4f}, kernel_ms "
                  f"{eng.kernel_ms():.4f}, marks {marks.tolist()}, advance counts {eng.advance_counts()}")
            assert w["hl_steps"] == total
            assert marks.shape == ((steps + 1,) if sub == 1 else (2,))
            assert marks[0] == 0.0 and np.all(np.diff(marks) >= 0.0)
            assert math.isfinite(w["hl_kernel_ms"]) and w["hl_kernel_ms"] > 0.0
            if mode == "centralized":
                assert eng.kernel_ms() == 0.0
            else:
                assert math.isfinite(eng.kernel_ms()) and eng.kernel_ms() > 0.0
            early, late = eng.advance_counts()
            if runs_overlap:
                assert early >= 0 and late >= 0 and early + late == B * total
            else:
                assert (early, late) == (0, 0)
            if log:
                ms = eng.log_read()["solve_ms"]
                assert ms.shape == (total,)
                assert np.all(np.isfinite(ms) & (ms > 0.0)) if sub == 1 else np.all(np.isnan(ms))
        if log:
            eng.log_end()
    finally:
        eng.close()


def test_gpu_closed_loop_needs_params():
    """The raw C ABI: on a handle without dat_set_params the closed loop refuses, with one sub-batch and with two,
    and the handle can still be destroyed."""
    from distributed_aerial_transportation_amd import _lib as L

    lib = L.lib()
    cfg = L.Config()
    lib.dat_default_config(cfg)
    cfg.mode, cfg.n, cfg.batch = L.MODE_CADMM, N, 7
    h = L.H()
    assert lib.dat_create(cfg, ctypes.byref(h)) == 0, lib.dat_last_error()
    try:
        assert lib.dat_closed_loop(h, 1) != 0
        assert b"dat_set_params has not been called" in lib.dat_last_error()
        assert lib.dat_set_sub_batches(h, 2) == 0, lib.dat_last_error()
        assert lib.dat_closed_loop(h, 1) != 0
        assert b"dat_set_params has not been called" in lib.dat_last_error()
    finally:
        assert lib.dat_destroy(h) == 0
