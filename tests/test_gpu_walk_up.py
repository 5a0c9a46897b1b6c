"""The way up of the contact sweep's walk (walk_to of the link-per-lane physics kernel: every link on the path from the link the walk
stands on to the lowest common ancestor of the move hands what its subtree has collected to its parent, and the ancestor answers what
arrives with its Lambda) - against the float64 C oracle (oracle/phys), one control step (4 substeps x 4 sweeps), PGS and TGS, both
builds of the kernel, 3 envs (one full pair and a half-empty wave) and 34 envs.

Every fixture is a pose built in tests/phys_poses.py with forward kinematics in numpy so that a chosen set of links, and only that set, is within reach
of the ground: joint angles put the chosen links lowest, a few free angles (a tilt of the root, one joint) are solved so that their lowest
hull vertices are level, and the root height sinks them 2 .. 4 mm into the ground; every other link stays more than the contact offset
(20 mm) above it.  Each test asserts from the oracle's own contact selection in the first substep that exactly this set touched.  Named
by what they make the level loop of the way up do (links are lanes in depth-first order; a link that is its parent's first child sits in
the lane after it and hands over through a lane shift, any other child through a pull - a "side entry"):
  ankle_toe  L_Ankle + L_Toe: one level, handed over by a first child; the walk turns at a touched link that holds impulse of its own
  feet       both feet: the walk turns at the root; L_Hip hands over as first child, R_Hip through a side entry
  hands      both hands: four chain levels, a side entry on both thoraxes, the turn at Chest (depth 3); nothing above the chest moves
             during the sweep
  head_hand  Head + L_Hand: a first-child arrival (Neck) and a side entry (L_Thorax) at the same turning link
  toe_hand   L_Toe + R_Hand: the turn at the root, Torso is not a first child, the longest way up (8 levels)
  mixed      the two envs of a wave differ: feet beside hands (they turn at different levels in the same move), feet beside an airborne
             env (one walk rests), beside an env that stands on its head (a single touched link: no move at all), and those among
             themselves
  flat       lying on the back: seven or more touched links
Bound: rows_all of tests/gpu_util.py (conditioning-aware; at most 2 % of the envs / 4 envs, and never more than half of them, may
need the conditioning term).  test_fixtures_touch_what_they_were_built_for checks on the CPU that the float64 oracle, perturbed at the
level of float32 rounding, stays inside that cap on its own (the seeds were chosen there).
(The kernels run without joint limits: the PGS cases go through the masked form of the way up, the TGS cases through the earlier form that
the TGS and joint-limit kernels keep - both forms stay covered.)
Env 0 holds the same state in the 3-env and in the 34-env batch beside different partners: its bits must not depend on the partner."""
import functools

import numpy as np
import pytest

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import FLAT_MIN_TOUCHED, POSES, STATE_IDS, _names

SIZES = (3, 34)
SOLVERS = ("pgs", "tgs")
CASES = [(n, build) for n in SIZES for build in (1, 2)]
FIXTURES = ("ankle_toe", "feet", "hands", "head_hand", "toe_hand", "mixed", "flat")
SEEDS = {"ankle_toe": 0, "feet": 0, "hands": 0, "head_hand": 0, "toe_hand": 0, "mixed": 0, "flat": 0}  # (chosen on the CPU)
# "mixed": the pose of every env.  Env 0 (feet, state 0) sits beside hands in the small batch and beside an airborne env in the large one
_MIXED_PAIRS = [("feet", "hands"), ("feet", "head"), ("hands", "feet"), ("head", "feet"), ("air", "feet"), ("hands", "head"), ("head", "hands"),
                ("hands", "air")]
MIXED = {3: ["feet", "hands", "air"], 34: ["feet", "air"] + [p for i in range(16) for p in _MIXED_PAIRS[i % len(_MIXED_PAIRS)]]}


def env_poses(fixture, n):
    return MIXED[n] if fixture == "mixed" else [fixture] * n


def states(fixture, n):
    return P.stack(P.state(pose, SEEDS[fixture], k) for pose, k in zip(env_poses(fixture, n), STATE_IDS[n]))


def oracle_for(fixture, n, solver):
    return P.oracle_for(states(fixture, n), solver_type={"pgs": 0, "tgs": 1}[solver])


def assert_touched(own, fixture, n):
    """own [n, nsub, NB, 4]: the oracle's contact selection.  In the first substep every env touches the ground with exactly the links
    its pose was built for (flat: with seven or more) - a fixture that does not exercise its level form fails here."""
    names = _names()
    touched = (own[:, 0] >= 0).any(axis=-1)  # [n, NB]
    for e, pose in enumerate(env_poses(fixture, n)):
        got = {names[b] for b in np.nonzero(touched[e])[0]}
        if POSES[pose][2] is None:
            assert len(got) >= FLAT_MIN_TOUCHED, (fixture, e, sorted(got))
        else:
            assert got == set(POSES[pose][2]), (fixture, e, pose, sorted(got))


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("n", SIZES)
def test_fixtures_touch_what_they_were_built_for(fixture, n, solver):
    """CPU: the fixtures touch the ground with the links they were built for, and the float64 oracle moved by float32 rounding of its
    inputs (the largest change over 32 perturbed runs, on every element) against itself needs the conditioning term in no more envs
    than rows_close allows - it asserts that cap itself."""
    inputs = P.oracle_inputs(states(fixture, n))
    own = oracle_for(fixture, n, solver).step(*inputs, nsub=P.NSUB, hold=2, want_selection=True)["own"]
    assert_touched(own, fixture, n)
    S.assert_oracle_holds_its_own_bound(oracle_for(fixture, n, solver), inputs, own, "%s %s n=%d" % (fixture, solver, n))


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(fixture, n, build, solver):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    st = states(fixture, n)
    got = S.kernel_step(*st[:3], P.actions(st), build=build, solver=solver)
    return got, S.reference(oracle_for(fixture, n, solver), got)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("n,build", CASES)
def test_way_up_matches_oracle(fixture, n, build, solver):
    """Every env of the fixture touches the ground with the links its pose was built for (the oracle's own selection in the first
    substep; the kernel's selection agrees on which links touch), the contacts carry load, and the step is the oracle's within the bounds of rows_all."""
    from tests.gpu_util import _compare

    got, ref = run_case(fixture, n, build, solver)
    assert_touched(ref["own"], fixture, n)
    assert np.array_equal((got["ids_sub"][:, 0] >= 0).any(axis=-1), (ref["own"][:, 0] >= 0).any(axis=-1))
    grounded = np.array([p != "air" for p in env_poses(fixture, n)])
    assert (np.abs(got["cf"]).reshape(n, -1).max(axis=1)[grounded] > 1.0).all(), "the contacts must carry load"
    assert np.abs(got["cf"][~grounded]).max(initial=0.0) == 0.0
    _compare(got, ref, "way up, %s %s n=%d build %d" % (fixture, solver, n, build))


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("build", [1, 2])
def test_env_bits_do_not_depend_on_the_partner(fixture, build, solver):
    """Env 0 holds the same state in the 3-env and in the 34-env batch; the env it shares its wave with differs."""
    S.assert_env0_ignores_its_partner(run_case(fixture, 3, build, solver)[0], run_case(fixture, 34, build, solver)[0])
