"""The visits of the contact sweep's walk (link-per-lane physics kernel): the k-th stops of the two envs of a wave are solved in the same
visit, and everything about a visit but "has this env applied an impulse yet" and "has it reached its fixed point" is fixed for the
substep - the kernels without joint limits read it from a table built once per substep (physics_ll.hip, VTAB).  What that table assumes,
pinned here by pairs of envs that the fixtures of tests/test_gpu_walk_up.py do not pin by themselves - against the float64 C oracle
(oracle/phys), one control step (4 substeps x 4 sweeps), PGS, both builds, 3 envs (a full pair and a half-empty wave) and 34 envs:
  one_seven  an env with ONE stop (it stands on its head) beside one with seven or more (lying on its back): the surplus visits of the
             first rest, and it never moves;  seven_one: the same pair in the other order
  air        an airborne env (no stop at all) beside a lying, a standing and a hand-standing one
  wrap       envs with two stops each whose LAST stops differ (L_Toe, R_Hand, L_Hand): in every later sweep the move into stop 0 comes
             from the env's own last stop
  hover      an env whose feet are within the contact offset of the ground but 12 mm above it: four stops, every point separated - its
             first sweep changes nothing, it is at its fixed point and drops out while its partner goes on
  late       an env whose left foot (its first two stops) hovers while its right foot (its last two) is in the ground: it applies its first
             impulse at its third stop, and only from there on does its walk move (the CPU test asserts from a one-substep step of the
             oracle that the left foot's links carry no force there and the right foot's do)
(An env that WAS live and then reaches its fixed point before the last sweep is not built on purpose: the box-friction sweep reaches a fixed
point in float32 only by chance, and the oracle does not report sweeps.  `hover` pins the drop-out itself; the closing move of a live env
from its last stop is what every other fixture runs.)
The poses, their builder and the oracle set-up are those of tests/phys_poses.py; `hover` and `late` are its `feet` states lifted
and rolled.  Bound: rows_all of tests/gpu_util.py with its cap on the conditioning term; test_visit_fixtures_are_what_they_claim
checks on the CPU that the float64 oracle, perturbed at the level of float32 rounding, stays inside that cap on its own (the seeds were
chosen there).  Env 0 holds the same state in the 3-env and in the 34-env batch beside different partners: same bits.
The table has no capacity limit to step over: a humanoid has 24 links, an env's stops are filed in the 32 lanes of its half of the wave."""
import functools

import numpy as np
import pytest

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import FEET, FLAT_MIN_TOUCHED, HOVER, POSES, STATE_IDS, _names, lowest_point

SIZES = (3, 34)
CASES = [(n, build) for n in SIZES for build in (1, 2)]
# pose of every env.  Env 0 is state 0 of its pose in both batches; its partner (env 1) is another pose in the two batches
_FILL = {
    "one_seven": [("head", "flat"), ("flat", "head")],
    "seven_one": [("flat", "head"), ("head", "flat")],
    "air": [("air", "flat"), ("feet", "air"), ("air", "hands"), ("flat", "air")],
    "wrap": [("ankle_toe", "hands"), ("hands", "ankle_toe"), ("head_hand", "ankle_toe"), ("ankle_toe", "toe_hand"), ("hands", "head_hand")],
    "hover": [("hover", "feet"), ("feet", "hover"), ("hover", "flat"), ("hands", "hover")],
    "late": [("late", "feet"), ("flat", "late"), ("late", "head"), ("hands", "late"), ("late", "late")],
}
_HEAD = {  # (the 3-env batch, the first pair of the 34-env batch)
    "one_seven": (["head", "flat", "flat"], ["head", "feet"]),
    "seven_one": (["flat", "head", "head"], ["flat", "air"]),
    "air": (["air", "flat", "feet"], ["air", "hands"]),
    "wrap": (["ankle_toe", "hands", "head_hand"], ["ankle_toe", "head_hand"]),
    "hover": (["hover", "feet", "hover"], ["hover", "flat"]),
    "late": (["late", "feet", "late"], ["late", "hands"]),
}
FIXTURES = tuple(_FILL)
SEEDS = {"one_seven": 0, "seven_one": 0, "air": 0, "wrap": 0, "hover": 0, "late": 0}  # (chosen on the CPU)


def env_poses(fixture, n):
    if n == 3:
        return _HEAD[fixture][0]
    fill = _FILL[fixture]
    return _HEAD[fixture][1] + [p for i in range(16) for p in fill[i % len(fill)]]


def states(fixture, n):
    return P.stack(P.state(pose, SEEDS[fixture], k) for pose, k in zip(env_poses(fixture, n), STATE_IDS[n]))


def oracle_for(fixture, n):
    return P.oracle_for(states(fixture, n), solver_type=0)


def assert_touched(own, fixture, n):
    """own [n, nsub, NB, 4]: the oracle's contact selection.  In the first substep every env touches the ground with exactly the links its
    pose was built for (flat: seven or more; hover, late: the four links of the feet - every one of them a stop of the walk), and the
    geometry of hover / late is what their names say."""
    names = _names()
    touched = (own[:, 0] >= 0).any(axis=-1)
    root, dpos, _, _ = states(fixture, n)
    stops = []
    for e, pose in enumerate(env_poses(fixture, n)):
        got = {names[b] for b in np.nonzero(touched[e])[0]}
        stops.append(len(got))
        if pose in ("hover", "late"):
            assert got == set(FEET), (fixture, e, pose, sorted(got))
            gap = lowest_point(root[e, 3:7], dpos[e])[[names.index(c) for c in FEET]] + root[e, 2]
            if pose == "hover":
                assert (gap > 0.5 * HOVER).all() and (gap < 0.02).all(), (fixture, e, gap)
            else:  # (the stops come in ascending link order: the left foot's first)
                assert names.index("L_Toe") < names.index("R_Ankle")
                assert (gap[:2] > 0.002).all() and (gap[:2] < 0.02).all() and gap[2:].min() < -0.001, (fixture, e, gap)
        elif POSES[pose][2] is None:
            assert len(got) >= FLAT_MIN_TOUCHED, (fixture, e, sorted(got))
        else:
            assert got == set(POSES[pose][2]), (fixture, e, pose, sorted(got))
    return stops


def _last_stop(pose):
    names = _names()
    return max(names.index(c) for c in POSES[pose][2])


def test_wrap_pairs_have_equal_counts_and_different_last_stops():
    """CPU: what the `wrap` fixture is for - in both batches env 0's pair has two stops each, and the last stops differ."""
    for n in SIZES:
        a, b = env_poses("wrap", n)[:2]
        assert len(POSES[a][2]) == len(POSES[b][2]) == 2 and _last_stop(a) != _last_stop(b), (n, a, b)


@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("n", SIZES)
def test_visit_fixtures_are_what_they_claim(fixture, n):
    """CPU: the envs touch the ground with the links they were built for (one stop beside seven, no stop beside some, ...), and the float64
    oracle moved by float32 rounding of its inputs (the largest change over 32 perturbed runs, on every element) against itself needs the
    conditioning term in no more envs than rows_close allows - it asserts that cap itself."""
    inputs = P.oracle_inputs(states(fixture, n))
    out = oracle_for(fixture, n).step(*inputs, nsub=P.NSUB, hold=2, want_selection=True)
    own = out["own"]
    stops = assert_touched(own, fixture, n)
    poses = env_poses(fixture, n)
    pairs = [(stops[e], stops[e + 1]) for e in range(0, n - 1, 2)]
    if fixture == "one_seven":
        assert pairs[0][0] == 1 and any(a == 1 and b >= 7 for a, b in pairs)
    if fixture == "seven_one":
        assert pairs[0][0] >= 7 and any(a >= 7 and b == 1 for a, b in pairs)
    if fixture == "air":
        assert pairs[0][0] == 0 and pairs[0][1] > 0 and any(a > 0 and b == 0 for a, b in pairs) == (n > 3)
    # a hovering env carries no load at the end of the step (it never applied an impulse), a late one does
    cf = np.abs(out["cf"]).reshape(n, -1).max(axis=1)
    for e, pose in enumerate(poses):
        assert (cf[e] == 0.0) == (pose in ("hover", "air")), (fixture, e, pose, cf[e])
    # ... and in the FIRST substep (a step of one substep from the same state) the left foot of a late env - its first two stops -
    # applies no impulse at all while its right foot does: the env turns live at its third stop
    if "late" in poses:
        cf1 = np.abs(oracle_for(fixture, n).step(*inputs, nsub=1, hold=2)["cf"]).max(axis=-1)  # [n, NB]
        names = _names()
        left, right = [names.index(c) for c in FEET[:2]], [names.index(c) for c in FEET[2:]]
        for e, pose in enumerate(poses):
            if pose == "late":
                assert (cf1[e, left] == 0.0).all() and cf1[e, right].max() > 1.0, (fixture, e, cf1[e, left], cf1[e, right])
    S.assert_oracle_holds_its_own_bound(oracle_for(fixture, n), inputs, own, "%s n=%d" % (fixture, n))


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(fixture, n, build):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    st = states(fixture, n)
    got = S.kernel_step(*st[:3], P.actions(st), build=build)
    return got, S.reference(oracle_for(fixture, n), got)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("n,build", CASES)
def test_sweep_visits_match_oracle(fixture, n, build):
    """Every env touches the ground with the links its pose was built for (the kernel's selection agrees on which links touch), the envs
    that stand on something carry load, the hovering and the airborne ones none, and the step is the oracle's within the bounds of
    rows_all."""
    from tests.gpu_util import _compare

    got, ref = run_case(fixture, n, build)
    assert_touched(ref["own"], fixture, n)
    assert np.array_equal((got["ids_sub"][:, 0] >= 0).any(axis=-1), (ref["own"][:, 0] >= 0).any(axis=-1))
    loaded = np.array([p not in ("air", "hover") for p in env_poses(fixture, n)])
    assert (np.abs(got["cf"]).reshape(n, -1).max(axis=1)[loaded] > 1.0).all(), "the contacts must carry load"
    assert np.abs(got["cf"][~loaded]).max(initial=0.0) == 0.0
    _compare(got, ref, "sweep visits, %s n=%d build %d" % (fixture, n, build))


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("build", [1, 2])
def test_env_bits_do_not_depend_on_the_partner(fixture, build):
    """Env 0 holds the same state in the 3-env and in the 34-env batch; the env it shares its wave with is another pose."""
    assert env_poses(fixture, 3)[1] != env_poses(fixture, 34)[1]
    S.assert_env0_ignores_its_partner(run_case(fixture, 3, build)[0], run_case(fixture, 34, build)[0])
