"""The tree passes of the link-per-lane physics kernel outside the contact sweep - pass 2 (articulated inertia, leaves -> root), the root
solve with pass 3 (root -> leaves) and the Lambda recursion - against the float64 C oracle (oracle/phys), one control step, both builds
of the kernel, 3 envs (one full pair and a half-empty wave) and 34 envs.

Three fixtures, built here from the baked body (forward kinematics in numpy decides the root height):
  air       every joint bent by 0.15 .. 0.45 rad, joint rates of ~1 rad/s, root tilted, tumbling and high above the ground: with
            enable_contact=False passes 1 - 3 and the integrator alone decide the result, every level of the tree, the links with two
            extra children (pelvis, chest) and the leaves all carry nonzero contributions.  Bound: the FLAT per-element bound of
            tests/gpu_util.py, no conditioning term.
  standing  upright on both feet (deepest touched links: the toes, depth 4), drives holding the pose.
  fallen    on the ground with the arms spread, rolled about the body's long axis onto one hand (left in the even states, right in the
            odd ones): the deepest touched link is a hand, depth 8.
            Bound of both: rows_all of tests/gpu_util.py (conditioning-aware, at most 2 % of the envs / 4 envs may need the
            conditioning term); test_contact_fixtures_are_well_conditioned checks on the CPU that the float64 oracle, perturbed at the
            level of float32 rounding, stays inside that cap on its own.
Env 0 holds the same state in the 3-env and in the 34-env batch beside different partners: its bits must not depend on the partner."""
import functools

import numpy as np
import pytest

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import STATE_IDS, _depths, lowest_point

SIZES = (3, 34)
CASES = [(n, build) for n in SIZES for build in (1, 2)]
KINDS = ("air", "standing", "fallen")
REST_VEL = {"standing": 0.05, "fallen": 0.05}       # joint rates of the resting fixtures, rad/s
SINK = {"standing": (0.002, 0.004), "fallen": (0.002, 0.004)}  # how far the lowest vertex is inside the ground, m
ROLL = (0.05, 0.25)  # rad
SEEDS = {"air": 0, "standing": 2, "fallen": 0}  # (chosen on the CPU: test_contact_fixtures_are_well_conditioned)


@functools.lru_cache(maxsize=None)
def state(kind, k):
    """State number k of a fixture: root [13] (xyzw quaternion), dof positions [69], dof velocities [69], residual wrench action [6]."""
    rng = np.random.default_rng([KINDS.index(kind), SEEDS[kind], k])
    root = np.zeros(13)
    if kind == "air":
        q = np.array([np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)]) + rng.normal(0, 0.3, size=4)
        dpos = rng.uniform(0.15, 0.45, size=69) * rng.choice([-1.0, 1.0], size=69) / np.sqrt(3.0)
        dvel = rng.normal(0, 1.0, size=69)
        root[7:10] = rng.normal(0, 0.5, size=3)
        root[10:13] = rng.normal(0, 1.0, size=3)
        height = 3.0
    else:
        # the baked body lies flat with the identity rotation; a quarter turn about x stands it up
        # (the fallen body is rolled about its long axis onto one hand, left or right: lying flat it rests on seven links at once, and
        # the float64 oracle itself then needs the conditioning term in a third of the envs)
        roll = 0.5 * rng.uniform(*ROLL) * (1.0 if k % 2 else -1.0)
        q = np.array([np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)]) if kind == "standing" else np.array([0.0, np.sin(roll), 0.0, np.cos(roll)])
        q = q + rng.normal(0, 0.0005, size=4)
        dpos = rng.normal(0, 0.004, size=69)
        dvel = rng.normal(0, REST_VEL[kind], size=69)
        root[7:10] = rng.normal(0, 0.4 * REST_VEL[kind], size=3)
        root[10:13] = rng.normal(0, 0.4 * REST_VEL[kind], size=3)
        height = None
    q /= np.linalg.norm(q)
    root[3:7] = q
    dpos, dvel = dpos.astype(np.float32), dvel.astype(np.float32)
    root = root.astype(np.float32)
    if height is None:  # the lowest vertex 2 .. 4 mm inside the ground
        height = -lowest_point(root[3:7], dpos).min() - rng.uniform(*SINK[kind])
    root[2] = height
    wrench = rng.normal(0, 0.17 if kind == "air" else 0.02, size=6).astype(np.float32)
    return root, dpos, dvel, wrench


def states(kind, n):
    return P.stack(state(kind, k) for k in STATE_IDS[n])


def oracle_for(kind, n):
    return P.oracle_for(states(kind, n), enable_contact=kind != "air")


@pytest.mark.parametrize("kind", ["standing", "fallen"])
@pytest.mark.parametrize("n", SIZES)
def test_contact_fixtures_are_well_conditioned(kind, n):
    """CPU: the fixtures touch the ground with the links they were built for (the deepest touched link sets how far the Lambda recursion
    runs), and the float64 oracle moved by float32 rounding of its inputs (the largest change over 32 perturbed runs, on every element)
    against itself needs the conditioning term in no more envs than rows_close allows - it asserts that cap itself."""
    dep = _depths()
    inputs = P.oracle_inputs(states(kind, n))
    own = oracle_for(kind, n).step(*inputs, nsub=P.NSUB, hold=2, want_selection=True)["own"]
    touched = (own >= 0).any(axis=-1)  # [n, nsub, NB]
    deepest = np.where(touched, dep[None, None, :], -1).max(axis=2)
    assert (deepest[:, 0] == {"standing": 4, "fallen": 8}[kind]).all(), deepest[:, 0].tolist()
    assert (touched[:, 0].sum(axis=1) >= {"standing": 2, "fallen": 1}[kind]).all()
    S.assert_oracle_holds_its_own_bound(oracle_for(kind, n), inputs, own, "%s n=%d" % (kind, n))


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(kind, n, build):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    st = states(kind, n)
    got = S.kernel_step(*st[:3], P.actions(st), build=build, contact=kind != "air")
    return got, S.reference(oracle_for(kind, n), got, contact=kind != "air")


@pytest.mark.gpu
@pytest.mark.parametrize("n,build", CASES)
def test_pd_only_step_matches_oracle_at_the_flat_bound(n, build):
    """Passes 1 - 3 and the integrator alone: every element of every env within the flat bounds of tests/gpu_util.py, no
    conditioning term (docs/NOTES.md A: PD-only runs never needed one; largest velocity error measured there 8e-6 rad/s)."""
    from tests.gpu_util import FORCE_ATOL, FORCE_RTOL, POS_ATOL, VEL_ATOL, VEL_RTOL, assert_none_over, rows_close

    got, ref = run_case("air", n, build)
    what = "tree passes, PD only n=%d build %d" % (n, build)
    assert np.abs(got["cf"]).max() == 0.0
    # every joint works: no drive force and no joint rate of the result is zero
    assert (np.abs(ref["df"]) > 1e-3).mean() > 0.95 and (np.abs(ref["dvel"]) > 1e-3).mean() > 0.95
    qs = np.sign(np.sum(got["rb"][..., 3:7] * ref["rb"][..., 3:7], axis=-1, keepdims=True))  # quaternion sign is arbitrary
    bad = rows_close(got["root"][:, :3], ref["root"][:, :3], POS_ATOL, 0.0, what + " root pos")
    bad |= rows_close(got["dpos"], ref["dpos"], 5e-5, 0.0, what + " dof_pos")
    bad |= rows_close(got["rb"][..., :3], ref["rb"][..., :3], POS_ATOL, 0.0, what + " rb pos")
    bad |= rows_close(got["rb"][..., 3:7] * qs, ref["rb"][..., 3:7], POS_ATOL, 0.0, what + " rb rot")
    bad |= rows_close(got["root"][:, 7:], ref["root"][:, 7:], VEL_ATOL, VEL_RTOL, what + " root vel")
    bad |= rows_close(got["dvel"], ref["dvel"], VEL_ATOL, VEL_RTOL, what + " dof_vel")
    bad |= rows_close(got["rb"][..., 7:], ref["rb"][..., 7:], VEL_ATOL, VEL_RTOL, what + " rb vel")
    bad |= rows_close(got["df"], ref["df"], FORCE_ATOL, FORCE_RTOL, what + " dof force")
    assert_none_over(bad, what)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["standing", "fallen"])
@pytest.mark.parametrize("n,build", CASES)
def test_contact_step_matches_oracle(kind, n, build):
    """With contacts: the Lambda recursion runs to depth 4 (standing, toes) and to depth 8 (fallen, hands); bounds of rows_all."""
    from tests.gpu_util import _compare

    got, ref = run_case(kind, n, build)
    dep = _depths()
    touched = (got["ids_sub"] >= 0).any(axis=-1)
    deepest = np.where(touched, dep[None, None, :], -1).max(axis=2)
    assert (deepest[:, 0] == {"standing": 4, "fallen": 8}[kind]).all(), deepest[:, 0].tolist()
    assert np.abs(got["cf"]).max() > 1.0, "the contacts must carry load"
    _compare(got, ref, "tree passes, %s n=%d build %d" % (kind, n, build))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("build", [1, 2])
def test_env_bits_do_not_depend_on_the_partner(kind, build):
    """Env 0 holds the same state in the 3-env and in the 34-env batch; the env it shares its wave with differs."""
    S.assert_env0_ignores_its_partner(run_case(kind, 3, build)[0], run_case(kind, 34, build)[0])
