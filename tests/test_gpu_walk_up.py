"""The way up of the contact sweep's walk (walk_to of the link-per-lane physics kernel: every link on the path from the link the walk
stands on to the lowest common ancestor of the move hands what its subtree has collected to its parent, and the ancestor answers what
arrives with its Lambda) - against the float64 C oracle (oracle/phys), one control step (4 substeps x 4 sweeps), PGS and TGS, both
builds of the kernel, 3 envs (one full pair and a half-empty wave) and 34 envs.

Every fixture is a pose built here with forward kinematics in numpy so that a chosen set of links, and only that set, is within reach
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
Bound: rows_all of tests/test_gpu_physics.py (conditioning-aware; at most 2 % of the envs / 4 envs, and never more than half of them, may
need the conditioning term).  test_fixtures_touch_what_they_were_built_for checks on the CPU that the float64 oracle, perturbed at the
level of float32 rounding, stays inside that cap on its own (the seeds were chosen there).
(The kernels run without joint limits: the PGS cases go through the masked form of the way up, the TGS cases through the earlier form that
the TGS and joint-limit kernels keep - both forms stay covered.)
Env 0 holds the same state in the 3-env and in the 34-env batch beside different partners: its bits must not depend on the partner."""
import functools

import numpy as np
import pytest

from oracle import task_oracle as O
from oracle.phys_oracle import BatchOracle, default_params
from tests.test_gpu_tree_passes import NB, NSUB, _mlib, _model, _rot_expmap, lowest_point

SIZES = (3, 34)
SOLVERS = ("pgs", "tgs")
CASES = [(n, build) for n in SIZES for build in (1, 2)]
REST_VEL = 0.05          # joint rates, rad/s
SINK = (0.002, 0.004)    # how far the lowest vertex is inside the ground, m
LEVEL = 5e-4            # the lowest vertices of the chosen links are level within this, m
CLEAR = 0.03             # every link outside the chosen set is at least this far above the lowest vertex, m (contact offset: 0.02)
X, Y, Z = np.eye(3)
# pose: rotations of the root (expmaps about world axes, applied in turn; the baked body lies on its back with the identity rotation),
# joint rotations (expmaps, parent axes: x to the body's left, y up the spine, z forward), the links that touch, and the free angles
# that level them ("root": a tilt about a world axis)
POSES = {
    "ankle_toe": ([X * np.pi / 2], {"R_Hip": X * -0.8, "R_Knee": X * 1.2}, ("L_Ankle", "L_Toe"), [("root", X)]),
    "feet": ([X * np.pi / 2], {}, ("L_Ankle", "L_Toe", "R_Ankle", "R_Toe"), [("root", X), ("root", Y), ("R_Ankle", X)]),
    "hands": ([Y * np.pi], {"L_Shoulder": Y * -np.pi / 2, "R_Shoulder": Y * np.pi / 2}, ("L_Hand", "R_Hand"), [("root", Y)]),
    "head_hand": ([X * -np.pi / 2], {"L_Shoulder": Z * 0.6, "R_Shoulder": Z * np.pi / 2}, ("Head", "L_Hand"), [("L_Shoulder", Z)]),
    "toe_hand": ([Y * np.pi], {"R_Shoulder": Y * np.pi / 2, "R_Hip": X * 0.6}, ("L_Toe", "R_Hand"), [("root", X)]),
    "head": ([X * -np.pi / 2], {}, ("Head",), []),
    "air": ([X * np.pi / 2], {}, (), []),
    # (no chosen set: whatever lies within reach, seven links or more)
    "flat": ([], {}, None, [("root", X), ("root", Y), ("L_Shoulder", Y), ("R_Shoulder", Y), ("Neck", X)]),
}
FLAT_LEVEL = ("L_Hand", "R_Hand", "Pelvis", "Chest", "Head")  # flat: the links the free angles bring level
FLAT_MIN_TOUCHED = 7
FIXTURES = ("ankle_toe", "feet", "hands", "head_hand", "toe_hand", "mixed", "flat")
SEEDS = {"ankle_toe": 0, "feet": 0, "hands": 0, "head_hand": 0, "toe_hand": 0, "mixed": 0, "flat": 0}  # (chosen on the CPU)
# state number of every env: env 0 is state 0 in both batches, its partner (env 1) is state 1 in one and state 3 in the other
STATE_IDS = {3: [0, 1, 2], 34: [0] + list(range(3, 36))}
# "mixed": the pose of every env.  Env 0 (feet, state 0) sits beside hands in the small batch and beside an airborne env in the large one
_MIXED_PAIRS = [("feet", "hands"), ("feet", "head"), ("hands", "feet"), ("head", "feet"), ("air", "feet"), ("hands", "head"), ("head", "hands"),
                ("hands", "air")]
MIXED = {3: ["feet", "hands", "air"], 34: ["feet", "air"] + [p for i in range(16) for p in _MIXED_PAIRS[i % len(_MIXED_PAIRS)]]}


def _names():
    return list(_model().body_names)


def _quat_of(R):  # xyzw
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    q = np.array([x, y, z, w])
    return q / np.linalg.norm(q)


def _expmap_of(R):
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if ang < 1e-12:
        return np.zeros(3)
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (ang / (2 * np.sin(ang)))


def posed(pose, rng):
    """Root quaternion (xyzw) and joint angles [69] of a pose, with small random joint angles and a small random tilt under it, the
    free angles solved (Gauss-Newton on the forward kinematics) so that the lowest vertices of the chosen links are level."""
    idx = {nm: i for i, nm in enumerate(_names())}
    rots, joints, chosen, free = POSES[pose]
    R0 = np.eye(3)
    for v in rots:
        R0 = _rot_expmap(v) @ R0
    R0 = _rot_expmap(rng.normal(0, 0.002, size=3)) @ R0
    noise = rng.normal(0, 0.004, size=69)
    fixed = {idx[j]: _rot_expmap(v) for j, v in joints.items()}

    def at(p):
        R, dp = R0, dict(fixed)
        for (what, ax), a in zip(free, p):
            if what == "root":
                R = _rot_expmap(ax * a) @ R
            else:
                dp[idx[what]] = dp.get(idx[what], np.eye(3)) @ _rot_expmap(ax * a)
        dpos = np.concatenate([_expmap_of(dp.get(b, np.eye(3)) @ _rot_expmap(noise[3 * (b - 1):3 * b])) for b in range(1, NB)])
        return _quat_of(R), dpos

    p = np.zeros(len(free))
    if free:
        ids = [idx[c] for c in (FLAT_LEVEL if chosen is None else chosen)]

        def resid(p):
            low = lowest_point(*at(p))[ids]
            return low - low.mean()

        for _ in range(40):  # (damped: the lowest vertex of a hull is a piecewise linear function of the angles)
            r = resid(p)
            if np.abs(r).max() < 1e-7:
                break
            J = np.stack([(resid(p + 1e-5 * e) - r) / 1e-5 for e in np.eye(len(p))], axis=1)
            step, t = np.clip(np.linalg.lstsq(J, r, rcond=None)[0], -0.05, 0.05), 1.0
            while t > 1e-3 and np.abs(resid(p - t * step)).max() >= np.abs(r).max():
                t *= 0.5
            p = p - t * step
    return at(p)


@functools.lru_cache(maxsize=None)
def state(pose, seed, k):
    """State number k of a pose: root [13] (xyzw quaternion), dof positions [69], dof velocities [69], residual wrench action [6]."""
    rng = np.random.default_rng([sorted(POSES).index(pose), seed, k])
    q, dpos = posed(pose, rng)
    root = np.zeros(13)
    root[3:7] = q
    dvel = rng.normal(0, REST_VEL, size=69)
    root[7:10] = rng.normal(0, 0.4 * REST_VEL, size=3)
    root[10:13] = rng.normal(0, 0.4 * REST_VEL, size=3)
    root, dpos, dvel = root.astype(np.float32), dpos.astype(np.float32), dvel.astype(np.float32)
    low = lowest_point(root[3:7], dpos)
    chosen = POSES[pose][2]
    if chosen is not None and len(chosen):
        ids = [_names().index(c) for c in chosen]
        others = np.delete(low, ids)
        assert np.ptp(low[ids]) < LEVEL and others.min() > low[ids].max() + CLEAR, (pose, k, np.round(np.sort(low) - low.min(), 4)[:6])
    root[2] = 3.0 if pose == "air" else -low.min() - rng.uniform(*SINK)
    wrench = rng.normal(0, 0.02, size=6).astype(np.float32)
    return root, dpos, dvel, wrench


def env_poses(fixture, n):
    return MIXED[n] if fixture == "mixed" else [fixture] * n


def states(fixture, n):
    parts = [state(pose, SEEDS[fixture], k) for pose, k in zip(env_poses(fixture, n), STATE_IDS[n])]
    return [np.stack([p[i] for p in parts]) for i in range(4)]


def actions(fixture, n):
    """PD targets = the pose the fixture is in (the drives hold it), plus the fixture's residual wrench."""
    _, dpos, _, wrench = states(fixture, n)
    return np.concatenate([dpos, wrench], axis=1).astype(np.float32)


def oracle_for(fixture, n, solver):
    root, dpos, dvel, _ = states(fixture, n)
    oracle = BatchOracle(_model(), n, default_params(solver_type={"pgs": 0, "tgs": 1}[solver]))
    oracle.set_state(root, dpos, dvel)
    return oracle


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
    from tests.gpu_util import N  # noqa: F401  (the helpers import torch; no GPU is touched here)
    from tests.test_gpu_physics import rows_all

    root, dpos, _, _ = states(fixture, n)
    act = actions(fixture, n)
    _, pd, _, force, torque = O.pre_physics(act, np.zeros(n, dtype=np.int64), dpos, root[:, 3:7], _model().kp.astype(np.float32))
    own = oracle_for(fixture, n, solver).step(pd, force, torque, nsub=NSUB, hold=2, want_selection=True)["own"]
    assert_touched(own, fixture, n)
    oracle = oracle_for(fixture, n, solver)
    sens = oracle.sensitivity(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own, seed=n)
    ref = oracle.step(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own)
    ref["sens"] = sens
    moved = {k: ref[k] + sens[k] for k in ("root", "dpos", "dvel", "rb", "cf", "df")}
    bad = rows_all(moved, ref, "oracle at float32 rounding, %s %s n=%d" % (fixture, solver, n))
    assert not bad.any()


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(fixture, n, build, solver):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    import torch

    from tests.gpu_util import N, T, close, make_task

    task = make_task(n, _mlib(), enable_contact=True, residual_force_hold="first_sim", debug_contacts=2, pair_envs_by_load=False,
                     kernel_build=build, contact_solver=solver, joint_limits=False)
    task.reset_with_times(None, T(np.full(n, 0.3)))
    root, dpos, dvel, _ = states(fixture, n)
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    oracle = oracle_for(fixture, n, solver)
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
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("n,build", CASES)
def test_way_up_matches_oracle(fixture, n, build, solver):
    """Every env of the fixture touches the ground with the links its pose was built for (the oracle's own selection in the first
    substep; the kernel's selection agrees on which links touch), the contacts carry load, and the step is the oracle's within the bounds of rows_all."""
    from tests.test_gpu_physics import _compare

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
    a, _ = run_case(fixture, 3, build, solver)
    b, _ = run_case(fixture, 34, build, solver)
    assert not np.array_equal(a["dvel"][1], b["dvel"][1]), "the partners must differ"
    for key in ("root", "dpos", "dvel", "rb", "cf", "df", "ids_sub"):
        assert np.array_equal(a[key][0], b[key][0]), key
