"""ref_track.npz against the oracle that wrote it (tests/golden/make_track.py): the first HL steps of each case's
tracked closed loop are replayed (tests/_track.py) and compared with the file, and the fixture's own figures -- pass
counts, the 1e-10-vs-1e-11 sensitivities -- are what test_gpu_tracking.py's bounds assume."""

import numpy as np
import pytest

from tests import _track
from tests._golden import load


@pytest.fixture(scope="module")
def fixture():
    return load("ref_track.npz")


@pytest.mark.parametrize("name", list(_track.CASES))
def test_fixture_replays_in_the_oracle(fixture, name):
    c = _track.Case(fixture, name)
    r = _track.run(name, 1e-11, steps=_track.REPLAY)
    K = _track.REPLAY
    assert np.array_equal(r["iters"], c.iters[:K])
    assert np.array_equal(r["start"], c.start)
    for key in ("acc", "f_des", "state"):
        assert np.max(np.abs(r[key] - getattr(c, key)[:K])) <= 1e-12, key
    np.testing.assert_allclose(r["err"], c.err[:K], rtol=1e-9, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", list(_track.CASES))
def test_fixture_shapes_and_sensitivities(fixture, name):
    c = _track.Case(fixture, name)
    kind, n, K = _track.CASES[name]
    assert c.acc.shape == (K, 6) and c.f_des.shape == (K, 3, n) and c.state.shape == (K, 12 * n + 18)
    assert K == (40 if n == 3 else 20)
    # the oracle's pass count moves nowhere between the two tolerances, so no step is excused on that account
    assert not c.count_moves.any() and np.all(np.isfinite(c.sens_f))
    # ... and its own state spread stays below a fifth of the GPU test's 1e-6 (test_gpu_tracking.py)
    assert 5 * float(c.state_spread) < 1e-6, float(c.state_spread)
    if kind == "centralized":
        assert np.all(c.iters == -1)
    else:
        assert np.all(c.iters >= 1) and np.all(c.iters <= _track.MAX_ITER)


def test_the_law_in_the_fixture_is_the_packages(fixture):
    """the fixture's acc_des (the law written out on the oracle's state) from the package's numpy statement"""
    from distributed_aerial_transportation_amd import tracking

    for name in _track.CASES:
        c = _track.Case(fixture, name)
        n = c.n
        x = np.concatenate([c.start[None], c.state[:-1]])
        t = np.arange(c.K) * _track.HL_EVERY * _track.DT
        acc = tracking.desired_acceleration(x[:, 12 * n:12 * n + 3], x[:, 12 * n + 3:12 * n + 6],
                                            tracking.circle_record(), t)
        assert np.array_equal(acc, c.acc), name
