"""The exclusion table (csrc/dat_modes.hpp) through the C-ABI: for every refused row, in both orders, a handle opens the
one side, attempts the other and gets DatError with the row's fragment; it then closes the first side and runs two
closed-loop steps, whose states, f_des and warm state equal, bitwise, those of a fresh handle that never made the
attempt: a refusal leaves nothing behind.  An attempt that had gone through would show: the episodes end every
scenario at its first step, the tracking records and the rigid-payload plant change the loop's arithmetic, and an
open log or open episodes answer their count queries.

C-ADMM with n = 3 and 4 scenarios in one forest; a centralized handle of the same size for the rows of the
rigid-payload plant (which is only set here, never run)."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, B, STEPS = 3, 4, 2


def _make(kind):
    from distributed_aerial_transportation_amd import BatchedController, Forest, scenarios

    rng = np.random.default_rng(5)
    eng = BatchedController(kind, N, B, scenarios.params_block(N))
    if kind == "cadmm":
        forests, sf = [Forest.seeded(0)], np.zeros(B, dtype=np.int32)
        eng.set_forests(forests, sf)
        x0 = scenarios.forest_path_states(N, B, rng, forests, sf)
    else:
        x0 = scenarios.perturbed_states(N, B, rng)
    eng.set_state(x0, np.zeros(B, dtype=np.int32))
    return eng


def _two_steps(eng):
    eng.closed_loop(STEPS)
    eng.synchronize()
    ck = eng.checkpoint()
    return eng.get_state()[0], ck.arrays()["f_des"].copy(), ck.tobytes()


@functools.lru_cache(maxsize=None)
def _fresh(kind):
    """a handle that never made an attempt, once per kind"""
    eng = _make(kind)
    try:
        out = _two_steps(eng)
    finally:
        eng.close()
    assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
    for a in out[:2]:
        a.setflags(write=False)
    return out


def _sides():
    """per feature / action: how a handle opens it (or does it), how it closes it, and the query that tells it is not
    open (None: the two closed-loop steps tell)"""
    from distributed_aerial_transportation_amd import tracking

    return {
        "log": (lambda e: e.log_begin(None, hl_capacity=4), lambda e: e.log_end(), lambda e: e.log_counts(), "no log open"),
        "episodes": (lambda e: e.episodes_begin(max_steps=1), lambda e: e.episodes_end(), lambda e: e.episodes_counts(),
                     "no episodes open"),
        "tracking": (lambda e: e.set_tracking(tracking.circle_record()), lambda e: e.set_tracking(None), None, None),
        "plant_rp": (lambda e: e.set_plant("rp"), lambda e: e.set_plant("rqp"), None, None),
        "ckpt_load": (lambda e: e.restore(e.checkpoint()), None, None, None),
    }


# every refused row in both orders (an action has one): the handle's kind, the side opened first, the side attempted,
# the fragment of the refusal
ROWS = [("cadmm", "log", "episodes", "log does not record episodes"),
        ("cadmm", "episodes", "log", "log does not record episodes"),
        ("cadmm", "episodes", "tracking", "tracking records"),
        ("cadmm", "tracking", "episodes", "tracking records"),
        ("cadmm", "episodes", "ckpt_load", "episodes are open"),
        ("centralized", "log", "plant_rp", "log does not record the rigid-payload plant"),
        ("centralized", "plant_rp", "log", "log does not record the rigid-payload plant"),
        ("centralized", "episodes", "plant_rp", "rigid-payload plant"),
        ("centralized", "plant_rp", "episodes", "rigid-payload plant")]


@pytest.mark.parametrize("kind,first,second,fragment", ROWS, ids=[f"{r[1]}-then-{r[2]}" for r in ROWS])
def test_a_refusal_leaves_nothing_behind(kind, first, second, fragment):
    from distributed_aerial_transportation_amd._lib import DatError

    sides = _sides()
    want = _fresh(kind)
    eng = _make(kind)
    try:
        sides[first][0](eng)
        with pytest.raises(DatError, match=fragment) as err:
            sides[second][0](eng)
        caller = {"log": "dat_log_begin", "episodes": "dat_episode_begin", "tracking": "dat_set_tracking",
                  "plant_rp": "dat_set_plant", "ckpt_load": "dat_checkpoint_load"}[second]
        remedy = {"log": "dat_log_end first", "episodes": "dat_episode_end first",
                  "tracking": "dat_set_tracking(NULL) first", "plant_rp": "dat_set_plant(DAT_PLANT_RQP) first"}[first]
        assert str(err.value).startswith(caller + ": ") and str(err.value).endswith(": " + remedy), str(err.value)
        _, _, query, closed = sides[second]
        if query is not None:
            with pytest.raises(DatError, match=closed):
                query(eng)
        sides[first][1](eng)
        got = _two_steps(eng)
    finally:
        eng.close()
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert got[2] == want[2]
