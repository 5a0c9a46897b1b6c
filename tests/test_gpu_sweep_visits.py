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
The poses, their builder and the oracle set-up are those of tests/test_gpu_walk_up.py; `hover` and `late` are its `feet` states lifted
and rolled.  Bound: rows_all of tests/test_gpu_physics.py with its cap on the conditioning term; test_visit_fixtures_are_what_they_claim
checks on the CPU that the float64 oracle, perturbed at the level of float32 rounding, stays inside that cap on its own (the seeds were
chosen there).  Env 0 holds the same state in the 3-env and in the 34-env batch beside different partners: same bits.
The table has no capacity limit to step over: a humanoid has 24 links, an env's stops are filed in the 32 lanes of its half of the wave."""
import functools

import numpy as np
import pytest

from oracle import task_oracle as O
from oracle.phys_oracle import BatchOracle, default_params
from tests import test_gpu_walk_up as W
from tests.test_gpu_tree_passes import NB, NSUB, _mlib, _model, _rot_expmap, _rot_quat, lowest_point

SIZES = (3, 34)
CASES = [(n, build) for n in SIZES for build in (1, 2)]
HOVER = 0.012           # hover: the lowest vertex is this far above the ground, m (contact offset: 0.02; free fall over the step: 5.4 mm)
ROLL = 0.05             # late: roll of the standing body about its forward axis, rad (feet 0.2 m apart: ~1 cm between their soles)
FEET = ("L_Ankle", "L_Toe", "R_Ankle", "R_Toe")
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


@functools.lru_cache(maxsize=None)
def state(pose, seed, k):
    """As state() of tests/test_gpu_walk_up.py; hover / late: its `feet` state, lifted / rolled so that the left foot is the higher one."""
    if pose not in ("hover", "late"):
        return W.state(pose, seed, k)
    root, dpos, dvel, wrench = [a.copy() for a in W.state("feet", seed, k)]
    names = W._names()
    feet = [names.index(c) for c in FEET]
    if pose == "hover":
        root[2] = -lowest_point(root[3:7], dpos).min() + HOVER
        return root, dpos, dvel, wrench
    rng = np.random.default_rng([97, seed, k])
    for sign in (1.0, -1.0):  # (the forward axis of the standing body is a world axis up to its small random tilt)
        q = W._quat_of(_rot_expmap(W.Y * sign * ROLL) @ _rot_quat(root[3:7])).astype(np.float32)
        low = lowest_point(q, dpos)
        if low[feet[:2]].min() > low[feet[2:]].min():
            break
    root[3:7] = q
    root[2] = -low.min() - rng.uniform(*W.SINK)
    return root, dpos, dvel, wrench


def states(fixture, n):
    parts = [state(pose, SEEDS[fixture], k) for pose, k in zip(env_poses(fixture, n), W.STATE_IDS[n])]
    return [np.stack([p[i] for p in parts]) for i in range(4)]


def actions(fixture, n):
    _, dpos, _, wrench = states(fixture, n)
    return np.concatenate([dpos, wrench], axis=1).astype(np.float32)


def oracle_for(fixture, n):
    root, dpos, dvel, _ = states(fixture, n)
    oracle = BatchOracle(_model(), n, default_params(solver_type=0))
    oracle.set_state(root, dpos, dvel)
    return oracle


def assert_touched(own, fixture, n):
    """own [n, nsub, NB, 4]: the oracle's contact selection.  In the first substep every env touches the ground with exactly the links its
    pose was built for (flat: seven or more; hover, late: the four links of the feet - every one of them a stop of the walk), and the
    geometry of hover / late is what their names say."""
    names = W._names()
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
        elif W.POSES[pose][2] is None:
            assert len(got) >= W.FLAT_MIN_TOUCHED, (fixture, e, sorted(got))
        else:
            assert got == set(W.POSES[pose][2]), (fixture, e, pose, sorted(got))
    return stops


def _last_stop(pose):
    names = W._names()
    return max(names.index(c) for c in W.POSES[pose][2])


def test_wrap_pairs_have_equal_counts_and_different_last_stops():
    """CPU: what the `wrap` fixture is for - in both batches env 0's pair has two stops each, and the last stops differ."""
    for n in SIZES:
        a, b = env_poses("wrap", n)[:2]
        assert len(W.POSES[a][2]) == len(W.POSES[b][2]) == 2 and _last_stop(a) != _last_stop(b), (n, a, b)


@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("n", SIZES)
def test_visit_fixtures_are_what_they_claim(fixture, n):
    """CPU: the envs touch the ground with the links they were built for (one stop beside seven, no stop beside some, ...), and the float64
    oracle moved by float32 rounding of its inputs (the largest change over 32 perturbed runs, on every element) against itself needs the
    conditioning term in no more envs than rows_close allows - it asserts that cap itself."""
    from tests.gpu_util import N  # noqa: F401  (the helpers import torch; no GPU is touched here)
    from tests.test_gpu_physics import rows_all

    root, dpos, _, _ = states(fixture, n)
    act = actions(fixture, n)
    _, pd, _, force, torque = O.pre_physics(act, np.zeros(n, dtype=np.int64), dpos, root[:, 3:7], _model().kp.astype(np.float32))
    out = oracle_for(fixture, n).step(pd, force, torque, nsub=NSUB, hold=2, want_selection=True)
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
        cf1 = np.abs(oracle_for(fixture, n).step(pd, force, torque, nsub=1, hold=2)["cf"]).max(axis=-1)  # [n, NB]
        names = W._names()
        left, right = [names.index(c) for c in FEET[:2]], [names.index(c) for c in FEET[2:]]
        for e, pose in enumerate(poses):
            if pose == "late":
                assert (cf1[e, left] == 0.0).all() and cf1[e, right].max() > 1.0, (fixture, e, cf1[e, left], cf1[e, right])
    oracle = oracle_for(fixture, n)
    sens = oracle.sensitivity(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own, seed=n)
    ref = oracle.step(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own)
    ref["sens"] = sens
    moved = {k: ref[k] + sens[k] for k in ("root", "dpos", "dvel", "rb", "cf", "df")}
    bad = rows_all(moved, ref, "oracle at float32 rounding, %s n=%d" % (fixture, n))
    assert not bad.any()


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(fixture, n, build):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    import torch

    from tests.gpu_util import N, T, close, make_task

    task = make_task(n, _mlib(), enable_contact=True, residual_force_hold="first_sim", debug_contacts=2, pair_envs_by_load=False,
                     kernel_build=build, contact_solver="pgs", joint_limits=False)
    task.reset_with_times(None, T(np.full(n, 0.3)))
    root, dpos, dvel, _ = states(fixture, n)
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    oracle = oracle_for(fixture, n)
    act = actions(fixture, n)
    rb0 = N(task._rigid_body_state).reshape(n, NB, 13).copy()
    dpos_before = N(task._dof_pos).copy()
    task.pre_physics_step(T(act))
    task._physics_step()
    torch.cuda.synchronize()
    pd_tar = N(task._pd_target)
    _, pd_ref, _, force, torque = O.pre_physics(act, N(task.reset_buf), dpos_before, rb0[:, 0, 3:7], task.body_model.kp.astype(np.float32))
    close(pd_tar, pd_ref, 1e-6, "pd target")
    got = {"root": N(task._humanoid_root_states), "dpos": N(task._dof_pos), "dvel": N(task._dof_vel), "rb": N(task._rigid_body_state).reshape(n, NB, 13),
           "cf": N(task._contact_forces), "df": N(task.dof_force_tensor), "ids": N(task.debug_contacts()), "ids_sub": N(task.debug_contacts_substeps())}
    name = task.kernel_build()
    task.close()
    assert name.startswith({1: "lds-parked", 2: "registers"}[build])
    sens = oracle.sensitivity(pd_tar, force, torque, nsub=NSUB, hold=2, forced_ids=got["ids_sub"], seed=n)
    ref = oracle.step(pd_tar, force, torque, nsub=NSUB, hold=2, forced_ids=got["ids_sub"], want_selection=True)
    ref["sens"] = sens
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("n,build", CASES)
def test_sweep_visits_match_oracle(fixture, n, build):
    """Every env touches the ground with the links its pose was built for (the kernel's selection agrees on which links touch), the envs
    that stand on something carry load, the hovering and the airborne ones none, and the step is the oracle's within the bounds of
    rows_all."""
    from tests.test_gpu_physics import _compare

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
    a, _ = run_case(fixture, 3, build)
    b, _ = run_case(fixture, 34, build)
    assert env_poses(fixture, 3)[1] != env_poses(fixture, 34)[1]
    assert not np.array_equal(a["dvel"][1], b["dvel"][1]), "the partners must differ"
    for key in ("root", "dpos", "dvel", "rb", "cf", "df", "ids_sub"):
        assert np.array_equal(a[key][0], b[key][0]), key
