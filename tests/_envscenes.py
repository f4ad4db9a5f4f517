"""The scenes the env-row tests run (test_env_rows_reference.py on the host build, test_gpu_env_rows_reference.py on
the device): per team size n in NS a list of at most 24 cases, each one payload state against its own forest of at
most 60 trees.  Deterministic: fixed seeds, no files.  Everything stated about a scene is asserted on the long-double
reference (tests/_envref.py) alone, never on the code under test.

Random scenes (RANDOM per n): 8 - 60 trees at radius 0.3 + rc / 2 ... 6.5 m around the payload, their centres up to
3.5 m above or below it; speed 0.05 - 3 m/s with the vertical component of the direction scaled by 0.05, 1 or 5; the
payload turned by up to 0.2 rad, so the agents' cameras look along different directions in every scene.

Named scenes (every n):
  cap_end1      descending, the capsule ends over a tree top more than 2 m + rc below the payload: t = 1, nearest
                point on the flat cap.
  cap_end0      ascending from over such a tree top: t = 0, nearest point on the flat cap.  The tree stands within
                0.3 m of the payload's vertical, behind every camera: only the centralized query sees it.
                (A cap contact with an interior minimiser does not exist as a unique minimum: over the cap the
                squared distance is (hz - 2)^2, strictly monotone in t unless the flight is level, and then every t
                over the cap is a minimiser and the row's min-time is not defined.  Both cap scenes are end points.)
  rim           ascending towards a tree whose top is just above the start: nearest point on the top rim, interior
                minimiser.
  graze         level flight past a tree at mid height, 5 mm clear: side contact, interior minimiser.
  vertical      |v_z| / |v| > 0.99 beside a tree.
  at_rest       vl = 0 with a tree inside the touch distance: collision, no row, min_env_dist = vision radius.
  inside        the payload body inside one tree and the capsule axis through another: negative min_env_dist,
                collision, rows from the other trees.
  crowd         30 trees on a spiral: some agent sees at least 14, and the 10 nearest are a strict subset.
  out_of_range  every tree outside the range test, some inside and some beyond the x-window ctr.x +- reach: no row.
  window_n      exactly n trees in the x-window (and trees beyond it on both sides);
  window_odd    2 n + 1 of them (no multiple of n).
  empty         a forest without trees.
  one           a single tree, in range.

Margins: the two sides of a comparison must not be able to disagree on a discontinuity through rounding alone, so on
the reference every tree in range has |d - 1e-4| > 1e-7, every tree |distance to the capsule centre - reach| > 1e-9,
every tree in range |cos - cos 100 deg| > 1e-9 for every agent, and every solve that sees more than 10 trees a gap
above 1e-6 between the 10th and the 11th nearest.  A random scene redraws the offending tree until they hold (no scene
is ever skipped); a named scene asserts them.

Coverage of the battery as a whole, asserted once (coverage()), counted over the (scene, tree in range) pairs and
over the solves (n agents and the centralized query per scene): at least 50 interior minimisers, 20 rim contacts,
2 cap contacts, 20 penetrations (d < 0) and 10 solves with more than 10 trees in view.  The battery holds
199 interior minimisers, 832 rim contacts, 10 cap contacts, 210 penetrations and 473 such solves."""

import functools
from dataclasses import dataclass

import numpy as np

from tests import _envref as er

NS = (3, 4, 6, 11, 16)
RANDOM = 11
MAX_CASES, MAX_TREES = 24, 60
ALPHA_D, ALPHA_C = 1.5, 2.0  # control/rqp_cadmm.py:221, control/rqp_centralized.py:210

TOUCH_MARGIN, RANGE_MARGIN, CONE_MARGIN, GAP_MARGIN = 1e-7, 1e-9, 1e-9, 1e-6
NEED = {"interior": 50, "rim": 20, "cap": 2, "penetration": 20, "crowded_solves": 10}


@dataclass
class Case:
    name: str
    n: int
    state: np.ndarray  # packed state (dat_layout.h DAT_S_*)
    trees: np.ndarray  # (T, 3), not sorted


@dataclass
class Ref:
    scene: er.Scene
    agents: list       # er.Rows of every agent, alpha 1.5
    central: er.Rows   # the centralized query, alpha 2.0


@functools.lru_cache(maxsize=None)
def params(n):
    from distributed_aerial_transportation_amd import scenarios

    return scenarios.params_block(n)


def _exp3(v):
    v = np.asarray(v, float)
    t = np.linalg.norm(v)
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    if t < 1e-8:
        return np.eye(3) + K
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t**2 * K @ K


def _state(n, xl, vl, rot):
    from distributed_aerial_transportation_amd.system import RQPState, pack_state

    return pack_state(RQPState(np.stack([np.eye(3)] * n, axis=2), np.zeros((3, n)), np.asarray(xl, float),
                               np.asarray(vl, float), _exp3(rot), np.zeros(3)))


def reference_of(case: Case) -> Ref:
    sc = er.scene(params(case.n), case.n, case.state, case.trees)
    return Ref(sc, [er.rows(sc, i, ALPHA_D) for i in range(case.n)], er.rows(sc, -1, ALPHA_C))


def offenders(ref: Ref):
    """trees (forest order) that stand within a margin of a discontinuity"""
    sc = ref.scene
    bad = set(np.nonzero(np.abs(sc.range_gap) <= RANGE_MARGIN)[0].tolist())
    inr = sc.range_gap <= 0
    bad |= set(np.nonzero(inr & (np.abs(sc.dist.d - er.TOUCH) <= TOUCH_MARGIN))[0].tolist())
    if sc.trees.shape[0]:
        for i in range(sc.fr.n):
            _, cg = er.cone_gap(sc, i)
            bad |= set(np.nonzero(inr & (np.abs(cg) <= CONE_MARGIN))[0].tolist())
    for r in ref.agents + [ref.central]:
        if not r.gap10 > GAP_MARGIN:
            order = r.seen[np.argsort(sc.dist.d[r.seen], kind="stable")]
            bad.add(int(order[er.NENV]))
    return sorted(bad)


# ---- random scenes ----------------------------------------------------------------------------------------------
def _random_case(n, k):
    rng = np.random.default_rng(1000 * n + k)
    rc = params(n)[er.layout.P["COLR"]]
    xl = np.array([12.0, -3.0, 2.5]) + rng.uniform(-1, 1, 3)
    u = rng.normal(size=3)
    u[2] *= (0.05, 1.0, 5.0)[k % 3]
    vl = rng.uniform(0.05, 3.0) * u / np.linalg.norm(u)
    ax = rng.normal(size=3)
    rot = rng.uniform(0, 0.2) * ax / np.linalg.norm(ax)

    def tree():
        rad, ang = rng.uniform(0.3 + rc / 2, 6.5), rng.uniform(0, 2 * np.pi)
        return [xl[0] + rad * np.cos(ang), xl[1] + rad * np.sin(ang), xl[2] + rng.uniform(-3.5, 3.5)]

    trees = np.array([tree() for _ in range(int(rng.integers(8, MAX_TREES + 1)))])
    case = Case(f"random{k}", n, _state(n, xl, vl, rot), trees)
    while True:
        ref = reference_of(case)
        bad = offenders(ref)
        if not bad:
            return case, ref
        for j in bad:
            case.trees[j] = tree()


# ---- named scenes -----------------------------------------------------------------------------------------------
X = np.array([12.0, -3.0, 2.5])
ROT = (0.02, -0.03, 0.15)


def _named(n):
    """[(case, check(ref): asserts on the reference that the scene hits its target)]"""
    prm = params(n)
    P = er.layout.P
    rc, visr, maxdec = prm[P["COLR"]], prm[P["VISR"]], prm[P["MAXDEC"]]
    reach = visr + 0.3
    out = []

    def add(name, vl, trees, check):
        out.append((Case(name, n, _state(n, X, vl, ROT), np.asarray(trees, float).reshape(-1, 3)), check))

    def h_of(speed):
        return 0.5 * speed * speed / maxdec

    def seen_by_agent(ref, j):
        return any(j in r.seen for r in ref.agents)

    # cap, end point t = 1
    ph = np.radians(35.0)
    d = np.array([np.cos(ph), 0.0, -np.sin(ph)])
    e = X + h_of(2.8) * d

    def chk(ref):
        D = ref.scene.dist
        assert D.region[0] == er.CAP and D.t[0] == 1 and D.d[0] > er.TOUCH
        assert ref.scene.trees[0, 2] < X[2] - (2 + rc) and 0 in ref.central.kept and seen_by_agent(ref, 0)
    add("cap_end1", 2.8 * d, [[e[0] + 0.1, e[1] + 0.05, e[2] - (rc + 0.4) - 2.0], [X[0] + 3.0, X[1] - 2.5, X[2]]], chk)

    # cap, end point t = 0
    d = np.array([np.cos(ph), 0.0, np.sin(ph)])

    def chk(ref):
        D = ref.scene.dist
        assert D.region[0] == er.CAP and D.t[0] == 0 and D.d[0] > er.TOUCH
        assert ref.scene.trees[0, 2] < X[2] - (2 + rc) and 0 in ref.central.kept
    add("cap_end0", 2.0 * d, [[X[0] - 0.1, X[1] + 0.08, X[2] - (rc + 0.4) - 2.0], [X[0] + 3.0, X[1] + 2.5, X[2]]], chk)

    # rim, interior minimiser
    ph = np.radians(50.0)
    d = np.array([np.cos(ph), 0.0, np.sin(ph)])

    def chk(ref):
        D = ref.scene.dist
        assert D.region[0] == er.RIM and D.interior[0] and D.d[0] > er.TOUCH
        assert D.p2[0, 2] == ref.scene.trees[0, 2] + 2 and seen_by_agent(ref, 0)
    add("rim", 2.8 * d, [[X[0] + 2.5, X[1], X[2] + 0.1 - 2.0]], chk)

    # graze
    def chk(ref):
        D = ref.scene.dist
        assert D.region[0] == er.SIDE and D.interior[0] and 1e-3 < D.d[0] < 1e-2 and seen_by_agent(ref, 0)
    add("graze", [2.0, 0.0, 0.0], [[X[0] + h_of(2.0) / 2, X[1] + 0.3 + rc + 5e-3, X[2]]], chk)

    # vertical flight
    d = np.array([0.06, 0.04, 1.0])
    d /= np.linalg.norm(d)

    def chk(ref):
        fr = ref.scene.fr
        assert abs(fr.vl[2]) / fr.speed > 0.99 and ref.scene.dist.d[0] > er.TOUCH and seen_by_agent(ref, 0)
    add("vertical", 2.5 * d, [[X[0] + 0.3 + rc + 0.4, X[1], X[2] + 0.5], [X[0] - 2.0, X[1] + 1.5, X[2] + 2.6]], chk)

    # at rest
    def chk(ref):
        assert ref.scene.dist.d[0] < er.TOUCH
        assert ref.central.collision and any(r.collision for r in ref.agents)
        for r in ref.agents + [ref.central]:
            assert r.rhs.size == 0 and r.min_env_dist == float(ref.scene.fr.visr)
    add("at_rest", [0.0, 0.0, 0.0], [[X[0] + 0.3 + rc / 2, X[1], X[2]], [X[0] + 3.0, X[1] + 1.0, X[2]]], chk)

    # inside
    def chk(ref):
        D = ref.scene.dist
        # (the bisection stops where the axis enters tree 1: distance 0 there, to rounding)
        assert D.region[0] == er.INSIDE and D.d[0] == -ref.scene.fr.rc and D.d[1] < 1e-15 - ref.scene.fr.rc
        assert ref.central.collision and ref.central.min_env_dist < 0 and ref.central.rhs.size >= 3
        hit = [r for r in ref.agents if 1 in r.seen]
        assert hit and all(r.collision and r.min_env_dist < 0 for r in hit) and any(r.rhs.size for r in hit)
    add("inside", [2.5, 0.0, 0.0],
        [[X[0] - 0.1, X[1] + 0.05, X[2] + 0.5], [X[0] + 1.2, X[1] + 0.2, X[2] - 0.4], [X[0] + 2.5, X[1] + 2.0, X[2]],
         [X[0] - 1.0, X[1] - 3.0, X[2] + 1.0], [X[0] + 3.0, X[1] - 2.2, X[2] - 1.0], [X[0] - 3.0, X[1] + 1.0, X[2]]],
        chk)

    # crowd
    k = np.arange(30)
    rad, ang = 0.3 + rc + 0.4 + 0.13 * k, 2.399963 * k

    def chk(ref):
        assert max(r.seen.size for r in ref.agents) >= 14 and ref.central.seen.size == 30
        assert all(r.gap10 > GAP_MARGIN for r in ref.agents + [ref.central])
    add("crowd", [1.0, 0.2, 0.0],
        np.column_stack([X[0] + rad * np.cos(ang), X[1] + rad * np.sin(ang), X[2] + 0.3 * (k % 5 - 2)]), chk)

    # out of range
    def chk(ref):
        fr = ref.scene.fr
        dx = np.abs(ref.scene.trees[:, 0] - fr.ctr[0])
        assert np.all(ref.scene.range_gap > 0) and np.sum(dx <= fr.reach) >= 3 and np.sum(dx > fr.reach) >= 2
        for r in ref.agents + [ref.central]:
            assert r.rhs.size == 0 and not r.collision and r.min_env_dist == float(fr.visr)
    add("out_of_range", [1.0, 0.0, 0.0],
        [[X[0] + 1.0, X[1] + reach + 0.5, X[2]], [X[0] - 2.0, X[1], X[2] + reach + 1.0],
         [X[0] + 3.0, X[1] - reach - 0.4, X[2]], [X[0] + reach + 2.0, X[1], X[2]], [X[0] - reach - 2.0, X[1], X[2]],
         [X[0] + reach + 5.0, X[1] + 1.0, X[2]]], chk)

    # x-window of exactly n trees, and of 2 n + 1
    for name, m in (("window_n", n), ("window_odd", 2 * n + 1)):
        ctr_x = X[0] + h_of(1.2) / 2
        x = np.linspace(ctr_x - reach + 0.2, ctr_x + reach - 0.2, m)
        j = np.arange(m)
        y = X[1] + np.where(j % 2, -1.0, 1.0) * (1.7 + 0.37 * (j % 7))
        inw = np.column_stack([x, y, X[2] + 0.4 * (j % 3 - 1)])
        beyond = [[ctr_x - reach - 0.3, X[1], X[2]], [ctr_x - reach - 4.0, X[1] + 1.0, X[2]],
                  [ctr_x + reach + 0.3, X[1], X[2]], [ctr_x + reach + 6.0, X[1] - 1.0, X[2]]]

        def chk(ref, m=m):
            fr = ref.scene.fr
            assert int(np.sum(np.abs(ref.scene.trees[:, 0] - fr.ctr[0]) <= fr.reach)) == m
            assert 0 < ref.central.seen.size < m
        add(name, [1.2, 0.0, 0.0], np.vstack([inw, beyond]), chk)

    def chk(ref):
        assert ref.central.rhs.size == 0 and not ref.central.collision
    add("empty", [1.0, 0.5, 0.1], np.zeros((0, 3)), chk)

    def chk(ref):
        assert ref.central.rhs.size == 1 and sum(r.rhs.size for r in ref.agents) >= 1
    add("one", [1.0, 0.5, 0.1], [[X[0] + 2.0, X[1] + 1.5, X[2] + 0.3]], chk)
    return out


@functools.lru_cache(maxsize=None)
def battery(n):
    """(cases, their references), named scenes first.  The library sorts every forest by x: the larger scenes built
    in x order are shuffled, the random ones are unsorted as drawn (the others name their trees by index)."""
    cases, refs = [], []
    for case, check in _named(n):
        if case.name in ("crowd", "window_n", "window_odd"):
            case.trees = case.trees[np.random.default_rng(7 * n + len(cases)).permutation(case.trees.shape[0])]
        ref = reference_of(case)
        check(ref)
        assert not offenders(ref), (n, case.name, offenders(ref))
        cases.append(case)
        refs.append(ref)
    for k in range(RANDOM):
        case, ref = _random_case(n, k)
        cases.append(case)
        refs.append(ref)
    assert len(cases) <= MAX_CASES and all(c.trees.shape[0] <= MAX_TREES for c in cases)
    for c in cases:
        c.state.setflags(write=False)
        c.trees.setflags(write=False)
    return tuple(cases), tuple(refs)


@functools.lru_cache(maxsize=None)
def coverage():
    """what the battery as a whole reaches, asserted against NEED"""
    got = dict.fromkeys(NEED, 0)
    for n in NS:
        for ref in battery(n)[1]:
            D, inr = ref.scene.dist, ref.scene.range_gap <= 0
            got["interior"] += int(np.sum(inr & D.interior))
            got["rim"] += int(np.sum(inr & (D.region == er.RIM)))
            got["cap"] += int(np.sum(inr & (D.region == er.CAP)))
            got["penetration"] += int(np.sum(inr & (D.d < 0)))
            got["crowded_solves"] += sum(r.seen.size > er.NENV for r in ref.agents + [ref.central])
    for k, need in NEED.items():
        assert got[k] >= need, (k, got[k], need)
    return got
