"""The trajectory-tracking law (csrc/dat_track.hpp) on the host, no GPU: the host build of the functions the kernels
call (tests/track_host) and the numpy statement (tracking.py) against the reference's own recording of the law
(ref_rp.npz: the 20 s loop of test/control/test_rpcentralized.py:main, acc[k] computed from the state after step
k - 1 at t = k dt), and against each other on random records."""

import numpy as np
import pytest

from tests import track_host as th
from tests._golden import load


def _blocks(d, n=3):
    """the state the reference's law saw at step k = 1 .. K - 1 (the one recorded after step k - 1), as dat blocks"""
    from distributed_aerial_transportation_amd import layout

    x = d["states"][:-1]
    st = np.zeros((x.shape[0], layout.state_size(n)))
    st[:, layout.s_off("XL", n):] = x
    return st


def test_host_build_reproduces_the_reference_recording():
    from distributed_aerial_transportation_amd import tracking

    d = load("ref_rp.npz")
    K = d["acc"].shape[0]
    acc = th.desired(_blocks(d), 3, tracking.circle_record(), np.arange(1, K), float(d["dt"]))
    worst = float(np.max(np.abs(acc - d["acc"][1:])))
    print(f"host build vs the reference's acc, k = 1 .. {K - 1}: {worst:.2e}")
    assert worst <= 1e-12
    # step 0: the reference's start state (rest at the origin)
    a0 = th.desired(np.zeros((1, _blocks(d).shape[1])), 3, tracking.circle_record(), 0, float(d["dt"]))
    assert np.max(np.abs(a0[0] - d["acc"][0])) <= 1e-12


def test_numpy_statement_reproduces_the_reference_recording_exactly():
    from distributed_aerial_transportation_amd import tracking

    d = load("ref_rp.npz")
    K, dt = d["acc"].shape[0], float(d["dt"])
    x = d["states"][:-1]
    t = np.arange(1, K) * dt
    acc = tracking.desired_acceleration(x[:, :3], x[:, 3:6], tracking.circle_record(), t)
    assert np.array_equal(acc, d["acc"][1:]), float(np.max(np.abs(acc - d["acc"][1:])))
    # the clock's time is the reference's t_seq to the bit
    assert np.array_equal(np.arange(K) * dt, np.arange(0, 20, dt))


def _random_records(rng, K):
    from distributed_aerial_transportation_amd import tracking

    T = tracking.T
    rec = np.zeros((K, tracking.TRACK_SIZE))
    rec[:, T["CX"]], rec[:, T["CY"]] = rng.uniform(-3, 3, K), rng.uniform(-3, 3, K)
    rec[:, T["RADIUS"]], rec[:, T["HEIGHT"]] = rng.uniform(0, 3, K), rng.uniform(0.5, 3, K)
    rec[:, T["FREQ"]], rec[:, T["T0"]] = rng.uniform(0, 2, K), rng.uniform(-5, 50, K)
    rec[:, T["KP"]], rec[:, T["KV"]] = rng.uniform(0, 4, K), rng.uniform(0, 4, K)
    rec[:, T["AMAX"]] = np.where(rng.random(K) < 0.6, rng.uniform(0.2, 3, K), rng.choice([0.0, -1.0], K))
    rec[:, T["WAMP"]], rec[:, T["WZ"]] = rng.uniform(-2, 2, K), rng.uniform(-1, 1, K)
    rec[::7, T["T0"]] = 0.0
    rec[::3, T["AMAX"]] *= 100.0  # a clamp that is set and does not bind
    return rec


def test_numpy_statement_and_host_build_agree_on_random_records():
    from distributed_aerial_transportation_amd import layout, tracking

    rng = np.random.default_rng(11)
    K, n, dt = 200, 3, 1e-3
    T = tracking.T
    rec = _random_records(rng, K)
    tick = rng.integers(0, 200000, K)
    st = np.zeros((K, layout.state_size(n)))
    o = layout.s_off("XL", n)
    st[:, o:o + 3], st[:, o + 3:o + 6] = rng.uniform(-4, 4, (K, 3)), rng.uniform(-2, 2, (K, 3))
    acc_h = th.desired(st, n, rec, tick, dt)
    acc_n = tracking.desired_acceleration(st[:, o:o + 3], st[:, o + 3:o + 6], rec, tick * dt)
    nrm = np.linalg.norm(acc_n[:, :3], axis=1)
    on = rec[:, T["AMAX"]] > 0
    clamped = on & (nrm >= rec[:, T["AMAX"]] * (1 - 1e-12))
    # the cases the issue names are all among the records
    assert clamped.sum() >= 20 and (on & ~clamped).sum() >= 5 and (~on).sum() >= 20
    assert np.any(rec[:, T["T0"]] != 0) and np.any(rec[:, T["CX"]] != 0)
    assert np.max(np.abs(acc_h - acc_n)) <= 1e-14, float(np.max(np.abs(acc_h - acc_n)))
    assert np.all(nrm[on] <= rec[on, T["AMAX"]] * (1 + 1e-15))
    xr, vr, ar = th.references(rec, tick, dt)
    for a, b in zip((xr, vr, ar), tracking.references(rec, tick * dt)):
        assert np.max(np.abs(a - b)) <= 1e-14


def test_clamp_has_the_forest_laws_form():
    """With KP = KV = 1, no feed-forward (FREQ = 0: a_ref = 0, v_ref = 0), WAMP = WZ = 0 and AMAX = 1 the tracking
    law is d = -(vl - 0) - (xl - x_ref) clamped to 1: the forest law's expression with v_ref = 0.  Compared with the
    forest law on states shifted so that both see the same error vector, the clamp included."""
    from distributed_aerial_transportation_amd import layout, tracking

    rng = np.random.default_rng(5)
    K, n = 64, 3
    o = layout.s_off("XL", n)
    st = np.zeros((K, layout.state_size(n)))
    st[:, o:o + 3] = rng.uniform(-2, 2, (K, 3)) * rng.choice([0.1, 1.0], (K, 1))
    st[:, o + 3:o + 6] = rng.uniform(-1, 1, (K, 3)) * rng.choice([0.1, 1.0], (K, 1))
    # (x_ref leads by 1.5 m: the law is unclamped only near vl = (2, 0, 0), y = 0, z = 1.5 -- every other state there)
    st[::2, o:o + 3] = np.array([0.0, 0.0, 1.5]) + rng.uniform(-0.2, 0.2, (K // 2, 3))
    st[::2, o + 3:o + 6] = np.array([2.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, (K // 2, 3))
    # forest law on flat ground: x_ref = (xl0 + 1.5, 0, 1.5), v_ref = (0.5, 0, 0)
    acc_f = th.desired_forest(st, n, np.array([30.0, 0.0, 25.0, 1e300, 0.0]))
    ex = np.stack([np.full(K, -1.5), st[:, o + 1], st[:, o + 2] - 1.5], axis=1)  # xl - x_ref of the forest law
    ev = st[:, o + 3:o + 6] - np.array([0.5, 0.0, 0.0])
    st2 = np.zeros_like(st)
    st2[:, o:o + 3], st2[:, o + 3:o + 6] = ex, ev
    rec = tracking.circle_record(center=(0.0, 0.0), radius=0.0, height=0.0, freq=0.0, amax=1.0, wamp=0.0, wz=0.0)
    acc_t = th.desired(st2, n, rec, 0, 1e-3)
    nrm = np.linalg.norm(acc_f[:, :3], axis=1)
    assert (nrm > 1 - 1e-12).sum() >= 10 and (nrm < 0.99).sum() >= 10  # both sides of the clamp
    assert np.max(np.abs(acc_t - acc_f)) <= 1e-15, float(np.max(np.abs(acc_t - acc_f)))
    # no clamp: the raw law
    raw = th.desired(st2, n, tracking.circle_record(radius=0.0, height=0.0, freq=0.0, amax=0.0, wamp=0.0, wz=0.0), 0,
                     1e-3)
    assert np.max(np.abs(raw[:, :3] - (-ev - ex))) <= 1e-15


@pytest.mark.parametrize("field,value", [("RADIUS", -1.0), ("FREQ", -0.5), ("KP", -1.0), ("KV", -1e-9),
                                         ("HEIGHT", np.nan), ("T0", np.inf), ("AMAX", -np.inf), ("RESERVED", np.nan)])
def test_bad_records_are_named(field, value):
    from distributed_aerial_transportation_amd import tracking

    rec = tracking.circle_record()
    assert th.bad_field(rec) == -1
    rec[tracking.T[field]] = value
    assert th.bad_field(rec) == tracking.T[field]
