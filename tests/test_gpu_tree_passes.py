"""The tree passes of the link-per-lane physics kernel outside the contact sweep - pass 2 (articulated inertia, leaves -> root), the root
solve with pass 3 (root -> leaves) and the Lambda recursion - against the float64 C oracle (oracle/phys), one control step, both builds
of the kernel, 3 envs (one full pair and a half-empty wave) and 34 envs.

Three fixtures, built here from the baked body (forward kinematics in numpy decides the root height):
  air       every joint bent by 0.15 .. 0.45 rad, joint rates of ~1 rad/s, root tilted, tumbling and high above the ground: with
            enable_contact=False passes 1 - 3 and the integrator alone decide the result, every level of the tree, the links with two
            extra children (pelvis, chest) and the leaves all carry nonzero contributions.  Bound: the FLAT per-element bound of
            tests/test_gpu_physics.py, no conditioning term.
  standing  upright on both feet (deepest touched links: the toes, depth 4), drives holding the pose.
  fallen    on the ground with the arms spread, rolled about the body's long axis onto one hand (left in the even states, right in the
            odd ones): the deepest touched link is a hand, depth 8.
            Bound of both: rows_all of tests/test_gpu_physics.py (conditioning-aware, at most 2 % of the envs / 4 envs may need the
            conditioning term); test_contact_fixtures_are_well_conditioned checks on the CPU that the float64 oracle, perturbed at the
            level of float32 rounding, stays inside that cap on its own.
Env 0 holds the same state in the 3-env and in the 34-env batch beside different partners: its bits must not depend on the partner."""
import functools

import numpy as np
import pytest

from oracle import task_oracle as O
from oracle.phys_oracle import BatchOracle, default_params

NSUB = 4
NB = 24
SIZES = (3, 34)
CASES = [(n, build) for n in SIZES for build in (1, 2)]
KINDS = ("air", "standing", "fallen")
REST_VEL = {"standing": 0.05, "fallen": 0.05}       # joint rates of the resting fixtures, rad/s
SINK = {"standing": (0.002, 0.004), "fallen": (0.002, 0.004)}  # how far the lowest vertex is inside the ground, m
ROLL = (0.05, 0.25)  # rad
SEEDS = {"air": 0, "standing": 2, "fallen": 0}  # (chosen on the CPU: test_contact_fixtures_are_well_conditioned)
# state number of every env: env 0 is state 0 in both batches, its partner (env 1) is state 1 in one and state 3 in the other
STATE_IDS = {3: [0, 1, 2], 34: [0] + list(range(3, 36))}


def _model():
    from vid2player3d_amd.model import load_baked_model

    return load_baked_model()


def _depths():
    par = np.asarray(_model().parents)
    dep = np.zeros(NB, dtype=int)
    for b in range(1, NB):
        dep[b] = dep[par[b]] + 1
    return dep


def _rot_expmap(v):
    a = float(np.linalg.norm(v))
    if a < 1e-12:
        return np.eye(3)
    k = np.asarray(v, dtype=np.float64) / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _rot_quat(q):  # xyzw
    x, y, z, w = [float(c) for c in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def lowest_point(quat, dpos):
    """Height of the lowest hull vertex of every link above the root's origin (forward kinematics, float64)."""
    m = _model()
    par, lp = np.asarray(m.parents), np.asarray(m.local_pos, dtype=np.float64)
    hv, ho = np.asarray(m.hull_verts, dtype=np.float64), np.asarray(m.hull_offsets)
    R, x = [None] * NB, np.zeros((NB, 3))
    R[0] = _rot_quat(quat)
    low = np.zeros(NB)
    for b in range(NB):
        if b:
            p = int(par[b])
            x[b] = x[p] + R[p] @ lp[b]
            R[b] = R[p] @ _rot_expmap(dpos[3 * (b - 1):3 * b])
        low[b] = (hv[ho[b]:ho[b + 1]] @ R[b].T)[:, 2].min() + x[b, 2]
    return low


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
    parts = [state(kind, k) for k in STATE_IDS[n]]
    return [np.stack([p[i] for p in parts]) for i in range(4)]


def actions(kind, n):
    """PD targets = the pose the fixture is in (the drives hold it), plus the fixture's residual wrench."""
    _, dpos, _, wrench = states(kind, n)
    return np.concatenate([dpos, wrench], axis=1).astype(np.float32)


def oracle_for(kind, n):
    root, dpos, dvel, _ = states(kind, n)
    oracle = BatchOracle(_model(), n, default_params(enable_contact=kind != "air"))
    oracle.set_state(root, dpos, dvel)
    return oracle


@pytest.mark.parametrize("kind", ["standing", "fallen"])
@pytest.mark.parametrize("n", SIZES)
def test_contact_fixtures_are_well_conditioned(kind, n):
    """CPU: the fixtures touch the ground with the links they were built for (the deepest touched link sets how far the Lambda recursion
    runs), and the float64 oracle moved by float32 rounding of its inputs (the largest change over 32 perturbed runs, on every element)
    against itself needs the conditioning term in no more envs than rows_close allows - it asserts that cap itself."""
    from tests.gpu_util import N  # noqa: F401  (the helpers import torch; no GPU is touched here)
    from tests.test_gpu_physics import rows_all

    dep = _depths()
    root, dpos, _, _ = states(kind, n)
    act = actions(kind, n)
    reset = np.zeros(n, dtype=np.int64)
    _, pd, _, force, torque = O.pre_physics(act, reset, dpos, root[:, 3:7], _model().kp.astype(np.float32))
    own = oracle_for(kind, n).step(pd, force, torque, nsub=NSUB, hold=2, want_selection=True)["own"]
    touched = (own >= 0).any(axis=-1)  # [n, nsub, NB]
    deepest = np.where(touched, dep[None, None, :], -1).max(axis=2)
    assert (deepest[:, 0] == {"standing": 4, "fallen": 8}[kind]).all(), deepest[:, 0].tolist()
    assert (touched[:, 0].sum(axis=1) >= {"standing": 2, "fallen": 1}[kind]).all()
    oracle = oracle_for(kind, n)
    sens = oracle.sensitivity(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own, seed=n)
    ref = oracle.step(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own)
    ref["sens"] = sens
    moved = {k: ref[k] + sens[k] for k in ("root", "dpos", "dvel", "rb", "cf", "df")}
    bad = rows_all(moved, ref, "oracle at float32 rounding, %s n=%d" % (kind, n))
    assert not bad.any()


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _mlib():
    from tests.gpu_util import DEV, synth_tables
    from vid2player3d_amd.motion_lib import MotionLib

    return MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV)


@functools.lru_cache(maxsize=None)
def run_case(kind, n, build):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    import torch

    from tests.gpu_util import N, T, close, make_task

    contact = kind != "air"
    task = make_task(n, _mlib(), enable_contact=contact, residual_force_hold="first_sim", debug_contacts=2, pair_envs_by_load=False,
                     kernel_build=build, contact_solver="pgs", joint_limits=False)
    task.reset_with_times(None, T(np.full(n, 0.3)))
    root, dpos, dvel, _ = states(kind, n)
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    oracle = oracle_for(kind, n)
    act = actions(kind, n)
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
    forced = got["ids_sub"] if contact else None
    sens = oracle.sensitivity(pd_tar, force, torque, nsub=NSUB, hold=2, forced_ids=forced, seed=n) if contact else None
    ref = oracle.step(pd_tar, force, torque, nsub=NSUB, hold=2, forced_ids=forced, want_selection=True)
    ref["sens"] = sens
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("n,build", CASES)
def test_pd_only_step_matches_oracle_at_the_flat_bound(n, build):
    """Passes 1 - 3 and the integrator alone: every element of every env within the flat bounds of tests/test_gpu_physics.py, no
    conditioning term (docs/NOTES.md A: PD-only runs never needed one; largest velocity error measured there 8e-6 rad/s)."""
    from tests.gpu_util import rows_close
    from tests.test_gpu_physics import POS_ATOL, VEL_ATOL, VEL_RTOL, FORCE_ATOL, FORCE_RTOL, assert_none_over

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
    from tests.test_gpu_physics import _compare

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
    a, _ = run_case(kind, 3, build)
    b, _ = run_case(kind, 34, build)
    assert not np.array_equal(a["dvel"][1], b["dvel"][1]), "the partners must differ"
    for key in ("root", "dpos", "dvel", "rb", "cf", "df", "ids_sub"):
        assert np.array_equal(a[key][0], b[key][0]), key
