"""k_cadmm's row modes are compile-time parameters of its instantiations (csrc/dat_cadmm_lds.hpp: DAT_CADMM_RMS, one
k_cadmm per mode triple of env classes 0 - 2, picked by the host from the word that sizes the LDS carve), and the
drain builds a slot's shared QP data at one site.  Neither changes a bit of any result:

  * every instantiated triple -- (2, 2, 2) and (2, 2, 1), all that dat_cadmm_row_mode gives for 3 <= n <= 16 --
    computes the same bits as the default, forced through dat_debug_row_modes: a forest step of B = 131 scenarios
    (the env-row tests' scene battery, tests/_envscenes.py, tiled; all four env classes occur) on four resident
    workgroups, so G = 64 // n slots per wavefront, slots are refilled and the last wavefront is partly filled; then a
    fused two-step dat_control_steps call without a forest at B = 97 (k_cadmm0, whose instantiation follows class
    0's mode alone: the same kernel under both triples).  n = 3 (the rule's triple at G = 21 is (2, 2, 1): the
    forced (2, 2, 2) is the one that never runs there otherwise), n = 6 and n = 16 (C5's team; its triple is n = 6's,
    (2, 2, 2), at every G -- no team size has a third);
  * a triple that is not instantiated is refused by dat_debug_row_modes with an error, and the handle keeps running
    the rule's;
  * the single build site: a fused K = 3 call equals three single-step calls bitwise at n = 6, B = 97 without a
    forest -- the fused next step used to be build_shared's second call site.  (test_gpu_drain.py's
    test_gpu_fused_steps_equal_separate_steps pins the same property at n = 3, B = 40 and n = 16, B = 9; this is the
    n = 6 shape with a partly filled last wavefront.)

Compared bitwise: f_des, iters, qp_status and the lane-level work counters (agent-QP solves, IPM iterations, row
iterations, in-band accepts, refinement passes and corrections, the tail's redos, certificates, stall exits and warm
starts).  The slot-level occupancy counters depend on which scenarios share a wavefront, which the queue does not fix,
and are left out."""

import functools

import numpy as np
import pytest

from tests import _envscenes as es
from tests.test_gpu_env_rows_reference import _forest

pytestmark = pytest.mark.gpu

B_FOREST, B_PLAIN, BLOCKS = 131, 97, 4
TRIPLES = ((2, 2, 2), (2, 2, 1))  # DAT_CADMM_RMS
LANE_COUNTERS = ("qp_solves", "ipm_iters", "ipm_row_iters", "inband_exits", "inband_beyond_clarabel_tol",
                 "refine_passes", "refine_corrections", "robust_redos", "certified_infeasible", "stall_exits",
                 "warm_starts")


def _rule(n, G):
    from distributed_aerial_transportation_amd import _lib

    return tuple(_lib.lib().dat_cadmm_row_mode(n, G, c) for c in range(3))


def test_triples_are_the_rule_s():
    """every triple the rule gives for a supported team is in TRIPLES, and each of TRIPLES occurs"""
    seen = {_rule(n, G) for n in range(3, 17) for G in range(1, 64 // n + 1)}
    assert seen == set(TRIPLES), seen
    assert _rule(3, 21) == (2, 2, 1) and _rule(6, 10) == (2, 2, 2) and _rule(16, 4) == (2, 2, 2)


@functools.lru_cache(maxsize=None)
def _plain_inputs(n, K):
    from distributed_aerial_transportation_amd import scenarios

    rng = np.random.default_rng(700 + n)
    return scenarios.perturbed_states(n, B_PLAIN, rng), rng.uniform(-0.5, 0.5, (K, B_PLAIN, 6)) * 8.0


def _forest_step(n, modes):
    """one forest control step of the tiled battery; (outputs, lane counters, env classes, G)"""
    from distributed_aerial_transportation_amd import BatchedController

    cases, _ = es.battery(n)
    sf = (np.arange(B_FOREST) % len(cases)).astype(np.int32)
    eng = BatchedController("cadmm", n, B_FOREST, es.params(n))
    try:
        eng.set_forests([_forest(c.trees) for c in cases], sf)
        eng.set_persistent_blocks(BLOCKS)
        eng.set_state(np.stack([cases[k].state for k in sf]), np.zeros(B_FOREST, dtype=np.int32))
        eng.debug_row_modes(modes)
        r = eng.control(None, None)
        w = eng.work()
        cls = eng.debug_env_class()[3]
        G = eng.cadmm_slots()
        per_class = [eng.class_work(k)["qp_solves"] for k in range(4)]
    finally:
        eng.close()
    return r, {k: w[k] for k in LANE_COUNTERS}, cls, G, per_class


def _plain_steps(n, modes, K=2):
    from distributed_aerial_transportation_amd import BatchedController

    x, accs = _plain_inputs(n, K)
    eng = BatchedController("cadmm", n, B_PLAIN, es.params(n))
    try:
        eng.set_persistent_blocks(BLOCKS)
        eng.set_state(x)
        eng.debug_row_modes(modes)
        r = eng.control_steps(accs)
        w = eng.work()
    finally:
        eng.close()
    return r, {k: w[k] for k in LANE_COUNTERS}


def _same(what, got, want):
    (r, w), (r0, w0) = got, want
    for a in ("f_des", "iters", "qp_status"):
        x, y = getattr(r, a), getattr(r0, a)
        assert x.tobytes() == y.tobytes(), (what, a, np.argwhere(x != y)[:5].tolist())
    assert w == w0, (what, w, w0)


@pytest.mark.parametrize("n", [3, 6, 16])
def test_gpu_every_instantiated_triple_computes_the_same_bits(n):
    r0, w0, cls, G, per_class = _forest_step(n, None)
    print(f"n = {n}: G {G}, rule {_rule(n, G)}, scenarios per env class {np.bincount(cls, minlength=4).tolist()}, "
          f"agent QPs per class {per_class}, counters {w0}")
    assert G == 64 // n and B_FOREST % G and B_FOREST > BLOCKS * G  # refill, and a partly filled last wavefront
    assert set(cls.tolist()) == {0, 1, 2, 3} and all(q > 0 for q in per_class)
    assert np.all(np.isfinite(r0.f_des)) and w0["qp_solves"] > 0
    p0 = _plain_steps(n, None)
    assert np.all(np.isfinite(p0[0].f_des)) and p0[1]["qp_solves"] >= 2 * n * B_PLAIN
    for modes in TRIPLES:
        r, w, cls_m, G_m, _ = _forest_step(n, modes)
        assert G_m == G and np.array_equal(cls_m, cls)
        _same(f"n = {n}, forest step, forced {modes}", (r, w), (r0, w0))
        _same(f"n = {n}, fused steps, forced {modes}", _plain_steps(n, modes), p0)


def test_gpu_unsupported_triple_is_refused():
    from distributed_aerial_transportation_amd import BatchedController
    from distributed_aerial_transportation_amd._lib import DatError

    n = 6
    x, accs = _plain_inputs(n, 2)
    eng = BatchedController("cadmm", n, B_PLAIN, es.params(n))
    try:
        eng.set_persistent_blocks(BLOCKS)
        eng.set_state(x)
        for bad in ((0, 0, 0), (2, 1, 2), (1, 2, 2), (2, 2, 0), (3, 2, 2), (2, 2, -1)):
            with pytest.raises(DatError):
                eng.debug_row_modes(bad)
        got = eng.control_steps(accs), {k: eng.work()[k] for k in LANE_COUNTERS}  # still the rule's
    finally:
        eng.close()
    _same("after refused triples", got, _plain_steps(n, None))


def test_gpu_single_build_site_fused_equals_separate():
    from distributed_aerial_transportation_amd import BatchedController

    n, K = 6, 3
    x, accs = _plain_inputs(n, K)
    sep = BatchedController("cadmm", n, B_PLAIN, es.params(n))
    try:
        sep.set_persistent_blocks(BLOCKS)
        sep.set_state(x)
        for k in range(K):
            rs = sep.control(None, accs[k])
        ws = {k: sep.work()[k] for k in LANE_COUNTERS}
    finally:
        sep.close()
    assert np.all(np.isfinite(rs.f_des))
    _same("fused K = 3 against three steps", _plain_steps(n, None, K), (rs, ws))
