"""Parity of the HIP physics step (float32, O(n) recursions) with the C oracle (dense float64 restatement of the same model,
oracle/phys) through the C ABI, plus size-independent properties at the BASELINE sizes.  PhysX itself is closed: parity with
Isaac Gym is unpinned.

EVERY env is compared.  Contact SELECTION and contact SOLVE are judged separately: the kernel reports the hull vertices it
selected in every substep (v2p_env_debug_contacts_substeps); the oracle is stepped with exactly those vertices, so that the
dynamics (articulated-body recursion + Gauss-Seidel) is compared on 100 % of the envs, and it also reports what its own selection
rule picks in the same state and how narrowly (decision margin in metres).  The selections must agree except where the rule is
within float32 rounding of deciding otherwise (a vertex at the contact offset, two candidates equally deep / far / wide)."""
import numpy as np
import pytest
import torch

from oracle import task_oracle as O
from oracle.phys_oracle import BatchOracle, default_params
from tests.gpu_util import (DEV, FORCE_ATOL, FORCE_RTOL, K_SENS, POS_ATOL, VEL_ATOL, VEL_RTOL, N, T, _compare, assert_none_over, close, make_task,
                            rows_all, rows_close, synth_tables)  # noqa: F401  (rows_all: tools/parity_sweep.py reads it from this module)

pytestmark = pytest.mark.gpu

# a selection decision closer than this (metres) is a tie between float32 and float64 evaluation of the same state
TIE_TOL = 5e-5
NSUB = 4


@pytest.fixture(scope="module")
def mlib():
    from vid2player3d_amd.motion_lib import MotionLib

    return MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV)


def selection_report(hip_ids, own_ids, margin, what, min_rate=0.99):
    """hip_ids / own_ids [n, nsub, 24, 4], margin [n, nsub, 24]: agreement of the two selections per (env, substep, body), over the
    bodies either of them puts in contact; every disagreement must be a tie of the selection rule."""
    active = (hip_ids >= 0).any(-1) | (own_ids >= 0).any(-1)
    same = np.all(hip_ids == own_ids, axis=-1)
    n_act, n_bad = int(active.sum()), int((active & ~same).sum())
    rate = 1.0 - n_bad / max(n_act, 1)
    env_rate = float(np.all(same, axis=(1, 2)).mean())
    worst = float(margin[active & ~same].max()) if n_bad else 0.0
    print("[selection] %s: %d touching (env, substep, body) triples, %d differ (agreement %.4f; envs with all substeps identical %.3f); "
          "largest decision margin among the differences %.2e m" % (what, n_act, n_bad, rate, env_rate, worst))
    assert n_act == 0 or rate >= min_rate, "%s: contact selection agrees on %.4f of the touching bodies only" % (what, rate)
    assert worst < TIE_TOL, "%s: a selection difference is not a tie (margin %.2e m)" % (what, worst)
    return rate, env_rate


def _perturbed_task(mlib, n, contact, rng, lift, vel_sigma, hold, shapes, **env):
    extra = {} if shapes is None else {"body_model": shapes}
    task = make_task(n, mlib, enable_contact=contact, residual_force_hold=hold, debug_contacts=2, **extra, **env)
    times = T(rng.uniform(0.1, 1.0, size=n))
    task.reset_with_times(None, times)
    # perturb the reference state so that the drives, Coriolis terms and contacts all have work to do
    root = N(task._humanoid_root_states).copy()
    root[:, 2] += lift
    root[:, 7:13] += rng.normal(0, vel_sigma, size=(n, 6)).astype(np.float32)
    dpos = N(task._dof_pos).copy() + rng.normal(0, 0.05, size=(n, 69)).astype(np.float32)
    dvel = N(task._dof_vel).copy() + rng.normal(0, vel_sigma, size=(n, 69)).astype(np.float32)
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    return task, root, dpos, dvel


def _run_pair(mlib, n, contact, seed, lift=0.0, vel_sigma=0.5, steps=1, hold="first_sim", shapes=None, subset=None, solver="pgs", what="", limits=False,
              act_sigma=0.17, oracle_solver=None, **env):
    """subset: env indices that get an oracle (all by default); the returned arrays are restricted to them.  Returns one
    (got, ref) per control step; ref carries the oracle's own selection ("own") and its margins next to the forced one."""
    rng = np.random.default_rng(seed)
    # (solver=None: env.contact_solver is not given - the sim block decides - and the oracle runs `oracle_solver`)
    if solver is not None:
        env = dict(env, contact_solver=solver)
    task, root, dpos, dvel = _perturbed_task(mlib, n, contact, rng, lift, vel_sigma, hold, shapes, joint_limits=limits, **env)
    ids_o = np.arange(n) if subset is None else np.asarray([int(i) for i in subset])
    par = default_params(enable_contact=contact)
    par.solver_type = {"pgs": 0, "tgs": 1}[solver or oracle_solver]
    par.joint_limits = int(limits)
    if "limit_margin" in env:
        par.limit_margin = float(env["limit_margin"])
    par.friction_frame = {"world": 0, "velocity": 1}[env.get("friction_frame", "world")]
    par.rest_offset = float(((env.get("sim_overrides") or {}).get("physx") or {}).get("rest_offset", 0.0))
    if shapes is None:
        oracle = BatchOracle(task.body_model, len(ids_o), par)
    else:  # the oracle of env e simulates the body shape of its clip (only the shapes of the compared envs are built)
        used, model_of = np.unique(np.asarray(task._env_shape_ids)[ids_o], return_inverse=True)
        oracle = BatchOracle([shapes[int(k)] for k in used], len(ids_o), par, model_of=model_of)
    oracle.set_state(root[ids_o], dpos[ids_o], dvel[ids_o])
    out = []
    for s in range(steps):
        act = np.concatenate([N(task._target_dof_pos) + rng.normal(0, act_sigma, size=(n, 69)), rng.normal(0, 0.17, size=(n, 6))], axis=1).astype(np.float32)
        rb0 = N(task._rigid_body_state).reshape(n, 24, 13).copy()
        dpos_before = N(task._dof_pos).copy()
        a = T(act)
        task.pre_physics_step(a)
        task._physics_step()
        torch.cuda.synchronize()
        pd_tar = N(task._pd_target)
        # wrench from the numpy oracle of pre_physics on the same inputs
        _, pd_ref, _, force, torque = O.pre_physics(act, N(task.reset_buf), dpos_before, rb0[:, 0, 3:7], task.body_model.kp.astype(np.float32))
        close(pd_tar, pd_ref, 1e-6, "pd target")
        got = {"root": N(task._humanoid_root_states), "dpos": N(task._dof_pos), "dvel": N(task._dof_vel),
               "rb": N(task._rigid_body_state).reshape(n, 24, 13), "cf": N(task._contact_forces), "df": N(task.dof_force_tensor),
               "ids": N(task.debug_contacts()), "ids_sub": N(task.debug_contacts_substeps()),
               # the inputs of the step (tools/parity_sweep.py --dump: outlier envs are re-examined offline with the CPU oracle)
               "in_root": root if s == 0 else None, "in_dpos": dpos if s == 0 else None, "in_dvel": dvel if s == 0 else None,
               "pd": pd_tar, "force": force, "torque": torque}
        got = {k: v for k, v in got.items() if v is not None}
        got = {k: v[ids_o] for k, v in got.items()}
        assert np.array_equal(got["ids_sub"][:, -1], got["ids"])
        hold_n = 2 if hold == "first_sim" else NSUB
        sens = oracle.sensitivity(pd_tar[ids_o], force[ids_o], torque[ids_o], nsub=NSUB, hold=hold_n, forced_ids=got["ids_sub"] if contact else None, seed=seed + s)
        ref = oracle.step(pd_tar[ids_o], force[ids_o], torque[ids_o], nsub=NSUB, hold=hold_n,
                          forced_ids=got["ids_sub"] if contact else None, want_selection=True)
        ref["sens"] = sens
        if contact:
            selection_report(got["ids_sub"], ref["own"], ref["margin"], "%s step %d" % (what or "seed %d" % seed, s))
        out.append((got, ref))
        task.post_physics_step()
    task.close()
    return out


def test_pd_only_step_matches_oracle(mlib):
    """BASELINE config 2 (small): flat ground absent, PD control + gravity + residual wrench only."""
    (got, ref), = _run_pair(mlib, 32, contact=False, seed=1, lift=0.5)
    _compare(got, ref, "no-contact", contact=False)
    assert np.abs(got["cf"]).max() == 0.0


def test_config2_1024_envs_pd_only(mlib):
    """BASELINE config 2 at its size: 1024 envs, PD control only; 96 of them (first, last, a spread) against their own oracles."""
    n = 1024
    subset = sorted(set([0, 1, n - 2, n - 1] + list(np.random.default_rng(2).integers(0, n, size=92))))
    for (got, ref) in _run_pair(mlib, n, contact=False, seed=12, lift=0.3, steps=2, subset=subset):
        _compare(got, ref, "config 2", contact=False)


def test_residual_wrench_held_for_all_simulate_calls(mlib):
    """residual_force_hold='all': the root wrench acts during all 4 substeps (the other reading of Isaac Gym's force lifetime)."""
    (got, ref), = _run_pair(mlib, 16, contact=False, seed=7, lift=0.5, hold="all")
    _compare(got, ref, "hold=all", contact=False)
    (got2, _), = _run_pair(mlib, 16, contact=False, seed=7, lift=0.5, hold="first_sim")
    assert np.abs(got["root"][:, 7:10] - got2["root"][:, 7:10]).max() > 1e-4  # and it does change the result


def test_contact_step_matches_oracle(mlib):
    """BASELINE config 3: hull-vs-plane contacts with the PGS solve; every env compared."""
    (got, ref), = _run_pair(mlib, 64, contact=True, seed=2, lift=0.0, what="standing")
    assert (got["ids"] >= 0).any(axis=(1, 2)).mean() > 0.8, "fixture must put most humanoids in contact"
    _compare(got, ref, "contact")


def test_fallen_humanoid_many_contacts_matches_oracle(mlib):
    """Low root height: most bodies touch the plane (worst case for the block Gauss-Seidel sweep); every env compared."""
    (got, ref), = _run_pair(mlib, 32, contact=True, seed=3, lift=-0.75, vel_sigma=0.2, what="fallen")
    assert ((got["ids"] >= 0).any(axis=2).sum(axis=1) >= 6).mean() > 0.5
    _compare(got, ref, "fallen")


def test_tgs_option_matches_oracle(mlib):
    """contact_solver='tgs' (v2p_sim_cfg.solver_type 1): temporal Gauss-Seidel with frozen Jacobians, kernel vs oracle; and it is a
    different solver (results differ from PGS on the same inputs)."""
    (got, ref), = _run_pair(mlib, 48, contact=True, seed=2, lift=-0.1, solver="tgs", what="tgs")
    _compare(got, ref, "tgs")
    (got_p, _), = _run_pair(mlib, 48, contact=True, seed=2, lift=-0.1, solver="pgs", what="pgs twin")
    assert np.abs(got["rb"][..., 7:] - got_p["rb"][..., 7:]).max() > 1e-3


@pytest.mark.parametrize("solver", ["pgs", "tgs"])
def test_velocity_aligned_friction_frame_matches_oracle(mlib, solver):
    """v2p_sim_cfg.friction_frame = velocity (ABI 14): the tangent rows of every hull x ground point along / across the tangential velocity
    the point has under v*; kernel (its own instantiation) against the oracle on every env, standing and fallen, either solver, with the
    racket arm's limit rows in the sweep as well; and the frame does change the result (sliding contacts)."""
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.racket import with_racket

    for seed, lift, sig, extra, what in ((2, 0.0, 0.5, {}, "standing"), (3, -0.75, 0.2, {}, "fallen"), (13, -0.5, 3.0, {}, "fast"),
                                         (62, -0.75, 0.2, dict(limits=True, body_model=with_racket(load_baked_model())[0], act_sigma=0.5), "fallen + limits")):
        what = "vfric %s %s" % (what, solver)
        pairs = _run_pair(mlib, 48, contact=True, seed=seed, lift=lift, vel_sigma=sig, steps=2, solver=solver, what=what, friction_frame="velocity", **extra)
        for got, ref in pairs:
            _compare(got, ref, what)
        (got_w, _), = _run_pair(mlib, 48, contact=True, seed=seed, lift=lift, vel_sigma=sig, solver=solver, what=what + " (world twin)", **extra)
        d = np.abs(pairs[0][0]["rb"][..., 7:] - got_w["rb"][..., 7:]).max(axis=(1, 2))
        print("[vfric] %s: body velocities differ from the world-frame run in %d of 48 envs (max %.3f m/s)" % (what, int((d > 1e-3).sum()), d.max()))
        if lift < 0:
            assert (d > 1e-3).mean() > 0.25


@pytest.mark.parametrize("build", [1, 2])
def test_both_builds_of_the_kernel_match_oracle(mlib, build):
    """The library holds two builds of the link-per-lane kernel (v2p_sim_cfg.kernel_build: 1 = contact records parked in LDS, three waves
    per SIMD; 2 = registers only, two waves) and picks by env count - the small fixtures of this file would otherwise only ever see
    build 2.  Each build on its own against the oracle: PGS standing, TGS, joint limits on a fallen fixture, PD only; a wrong value is refused."""
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.racket import with_racket

    name = {1: "lds-parked, 3 waves per SIMD", 2: "registers, 2 waves per SIMD"}[build]
    task = make_task(8, mlib, kernel_build=build)
    assert task.kernel_build() == name
    task.close()
    for kw in (dict(contact=True, seed=2, lift=0.0), dict(contact=True, seed=2, lift=-0.1, solver="tgs"), dict(contact=False, seed=1),
               dict(contact=True, seed=62, lift=-0.75, vel_sigma=0.2, limits=True, body_model=with_racket(load_baked_model())[0], act_sigma=0.5),
               dict(contact=True, seed=62, lift=-0.75, vel_sigma=0.2, limits=True, solver="tgs", body_model=with_racket(load_baked_model())[0], act_sigma=0.5),
               dict(contact=True, seed=3, lift=-0.75, vel_sigma=0.2, friction_frame="velocity")):
        what = "build %d %s" % (build, " ".join("%s=%s" % (k, v) for k, v in kw.items() if k in ("contact", "solver", "limits", "lift")))
        (got, ref), = _run_pair(mlib, 48, what=what, kernel_build=build, **kw)
        _compare(got, ref, what, contact=kw["contact"])
    with pytest.raises(RuntimeError, match="kernel_build"):
        make_task(8, mlib, kernel_build=3)


def test_engine_picks_the_build_by_envs_resident_on_the_device(mlib):
    """kernel_build = 0: by the envs of ALL live batches of the process on the device (rollout groups share the GPU's wave slots), launch
    by launch - a small batch runs the register build while it is alone and the three-wave build while a large one lives beside it."""
    small = make_task(64, mlib)
    assert small.kernel_build().startswith("registers")
    large = make_task(8192, mlib)
    assert large.kernel_build().startswith("lds-parked") and small.kernel_build().startswith("lds-parked")
    halves = [make_task(4096, mlib) for _ in range(2)]  # 2 x 4096 = what bench.py --groups 2 and PPOAgent's rollout groups create
    assert all(h.kernel_build().startswith("lds-parked") for h in halves)
    for t in halves + [large]:
        t.close()
    assert small.kernel_build().startswith("registers")
    fixed = make_task(64, mlib, kernel_build=1)
    assert fixed.kernel_build().startswith("lds-parked") and small.kernel_build().startswith("registers")
    a = torch.cat([small._target_dof_pos.clone(), torch.zeros((64, 6), device=DEV)], dim=1).contiguous()
    small.reset_with_times(None, torch.full((64,), 0.3, device=DEV))
    small.step(a)
    small.check()
    # the choice is LATCHED at the first launch of an epoch (advisor r5): a batch that comes or goes next to a stepping one does not switch
    # it to the other build mid-epoch (the builds agree to rounding only); the next whole-batch reset chooses anew
    other = make_task(8192, mlib)
    assert small.kernel_build().startswith("registers") and other.kernel_build().startswith("lds-parked")
    small.step(a)
    assert small.kernel_build().startswith("registers")
    small.reset_with_times(None, torch.full((64,), 0.3, device=DEV))
    assert small.kernel_build().startswith("lds-parked")
    small.step(a)
    other.close()
    assert small.kernel_build().startswith("lds-parked")  # ... and holds again until the next reset
    small.check()
    small.close()
    fixed.close()


PHYSX_AMASS_IM = {"num_threads": 4, "solver_type": 1, "num_position_iterations": 4, "num_velocity_iterations": 0, "contact_offset": 0.02, "rest_offset": 0.0,
                  "bounce_threshold_velocity": 0.2, "max_depenetration_velocity": 10.0, "default_buffer_size_multiplier": 10.0}  # cfg/amass_im.yaml:39-48


def test_the_references_sim_block_runs_tgs_and_other_values_reach_the_engine(mlib):
    """The sim.physx block of the reference's yaml at the boundary: solver_type 1 makes the engine run TGS (same numbers as
    env.contact_solver='tgs', different from PGS); rest_offset moves the rest height of the hull vertices in kernel and oracle alike;
    num_velocity_iterations != 0 is refused by the library."""
    task = make_task(8, mlib, sim_overrides={"physx": dict(PHYSX_AMASS_IM)})
    assert task.contact_solver == "tgs" and task.contact_solver_source == "sim.physx.solver_type"
    task.close()
    (got_y, _), = _run_pair(mlib, 24, contact=True, seed=2, lift=-0.1, what="yaml tgs", sim_overrides={"physx": dict(PHYSX_AMASS_IM)}, solver=None, oracle_solver="tgs")
    (got_e, _), = _run_pair(mlib, 24, contact=True, seed=2, lift=-0.1, what="env tgs", solver="tgs")
    assert np.array_equal(got_y["rb"], got_e["rb"]) and np.array_equal(got_y["cf"], got_e["cf"])
    (got, ref), = _run_pair(mlib, 32, contact=True, seed=2, lift=0.0, what="rest offset", sim_overrides={"physx": dict(PHYSX_AMASS_IM, solver_type=0, rest_offset=0.005)})
    _compare(got, ref, "rest_offset 5 mm")
    (got0, _), = _run_pair(mlib, 32, contact=True, seed=2, lift=0.0, what="rest offset 0", sim_overrides={"physx": dict(PHYSX_AMASS_IM, solver_type=0)})
    assert np.abs(got["rb"][..., 7:] - got0["rb"][..., 7:]).max() > 1e-3, "rest_offset must change the result"
    with pytest.raises(RuntimeError, match="num_velocity_iterations"):
        make_task(8, mlib, sim_overrides={"physx": dict(PHYSX_AMASS_IM, num_velocity_iterations=1)})


@pytest.mark.parametrize("solver", ["pgs", "tgs"])
def test_joint_limits_match_oracle(mlib, solver):
    """v2p_sim_cfg.joint_limits with the player MJCF's racket-arm ranges (R_Wrist +-10 / +-45 / +-90 deg, R_Elbow_x <= 90 deg): the
    reference poses put the wrist beyond +-10 deg in most envs, so the rows work against violated limits (erp) and against approached
    ones (speculative); standing and fallen fixtures, every env against its oracle; and the rows do change the result."""
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.racket import with_racket

    bm, _ = with_racket(load_baked_model())
    jw = 3 * (bm.body_index("R_Wrist") - 1)
    for seed, lift, sig, what in ((61, 0.0, 0.5, "limits standing"), (62, -0.75, 0.2, "limits fallen")):
        what = what + " " + solver
        pairs = _run_pair(mlib, 48, contact=True, seed=seed, lift=lift, vel_sigma=sig, steps=2, limits=True, body_model=bm, act_sigma=0.5, what=what, solver=solver)
        for got, ref in pairs:
            _compare(got, ref, what)
        (got0, _), = _run_pair(mlib, 48, contact=True, seed=seed, lift=lift, vel_sigma=sig, limits=False, body_model=bm, act_sigma=0.5, what=what + " off", solver=solver)
        moved = np.abs(pairs[0][0]["dvel"][:, jw:jw + 3] - got0["dvel"][:, jw:jw + 3]).max(axis=1)
        print("[limits] %s: wrist rates differ from the run without limits in %d of 48 envs (max %.2f rad/s)" % (what, (moved > 1e-2).sum(), moved.max()))
        assert (moved > 1e-2).mean() > 0.5


def test_multi_step_drift_is_bounded(mlib):
    """8 control steps (32 substeps) from a perturbed state: float32 vs float64 trajectories of every env stay close when both
    use the contact vertices the kernel selected."""
    pairs = _run_pair(mlib, 32, contact=True, seed=4, steps=8, what="8 steps")
    got, ref = pairs[-1]
    close(got["rb"][..., :3], ref["rb"][..., :3], 2e-3, "rb pos after 8 steps")
    qs = np.sign(np.sum(got["rb"][..., 3:7] * ref["rb"][..., 3:7], axis=-1, keepdims=True))
    close(got["rb"][..., 3:7] * qs, ref["rb"][..., 3:7], 2e-3, "rb rot after 8 steps")


def test_config4_settings_match_oracle():
    """BASELINE config 4 without racket and ball (djokovic_im.yaml = the same task class with head termination height
    -0.5 and tennis-speed clips): physics vs the C oracle and reward / reset flags vs the task oracle over 4 control steps."""
    from vid2player3d_amd import motion_tables, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    bm = load_baked_model()
    clips = synth.make_clips(9, 8, 60, 120, 2.0)  # speed 2: faster random walks
    tabs = motion_tables.build_tables(clips, bm.parents, bm.local_pos)
    lib = MotionLib(tabs, DEV)
    n = 64
    _epoch_against_oracles(lib, tabs, n, steps=4, seed=21, sigma=0.17, terminationHeadHeight=-0.5)


def test_config1_four_envs_one_clip_whole_epoch():
    """BASELINE config 1 (embodied_pose amass_im cfg, num_envs=4, ONE clip; the reference runs it on the CPU PhysX path - this engine has
    no CPU path, so the same configuration runs on the GPU): 4 envs bound to one 300-frame clip, contacts on, a whole
    32-step epoch against TaskOracle + the C oracle: physics per element on every env, rewards, reset / terminate / progress flags."""
    from vid2player3d_amd import motion_tables, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    bm = load_baked_model()
    tabs = motion_tables.build_tables(synth.make_clips(7, 1, 300, 300), bm.parents, bm.local_pos)
    assert len(tabs["motion_num_frames"]) == 1 and int(tabs["motion_num_frames"][0]) == 300
    _epoch_against_oracles(MotionLib(tabs, DEV), tabs, 4, steps=32, seed=7, sigma=0.17)


def test_epoch_under_the_references_solver_choice():
    """The reference's yaml names TGS (cfg/amass_im.yaml:41, solver_type 1): the same epoch comparison - physics per element on every
    env, rewards, flags - with the engine's TGS selected the way the reference selects it, through the sim block."""
    from vid2player3d_amd import motion_tables, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    bm = load_baked_model()
    tabs = motion_tables.build_tables(synth.make_clips(11, 8, 90, 160), bm.parents, bm.local_pos)
    _epoch_against_oracles(MotionLib(tabs, DEV), tabs, 32, steps=12, seed=41, sigma=0.4, oracle_solver=1, sim_overrides={"physx": dict(PHYSX_AMASS_IM)})


def _epoch_against_oracles(lib, tabs, n, steps, seed, sigma, oracle_solver=0, **env):
    """`steps` control steps after one reset, teacher-forced per control step: before every step the C oracle is set to
    the engine's state, both take the step (the oracle with the kernel's contact vertices), the physics results are compared at
    the one-step tolerances on EVERY env, and the task oracle continues from the ORACLE's result with its own sticky buffers:
    rewards to 1e-3, reset / terminate / progress flags flag for flag at every step."""
    rng = np.random.default_rng(seed)
    task = make_task(n, lib, debug_contacts=2, **env)
    bm = task.body_model
    times = rng.uniform(0.05, 0.6, size=n).astype(np.float32)
    task.reset_with_times(None, T(times))
    th = N(task._termination_heights).copy()
    ref = O.TaskOracle(tabs, N(task._reset_ref_motion_ids), bm.kp.astype(np.float32), term_heights=th)
    ref.reset_all(times)
    close(N(task.obs_buf), ref.obs_buf, 5e-6, "reset obs")
    oracle = BatchOracle(bm, n, default_params(solver_type=oracle_solver))
    assert task.contact_solver == ("tgs" if oracle_solver else "pgs")
    died = 0
    for k in range(steps):
        oracle.set_state(N(task._humanoid_root_states), N(task._dof_pos), N(task._dof_vel))
        act = np.concatenate([ref.target[2] + rng.normal(0, sigma, size=(n, 69)), rng.normal(0, sigma, size=(n, 6))], axis=1).astype(np.float32)
        a = T(act)
        task.step(a)
        torch.cuda.synchronize()
        _, pd, _, force, torque = ref.pre_physics_step(act)
        assert np.array_equal(N(a), ref.actions), "in-place action masking of dead envs"
        ids_sub = N(task.debug_contacts_substeps())
        sens = oracle.sensitivity(pd, force, torque, nsub=NSUB, hold=2, forced_ids=ids_sub, seed=seed + k)
        res = oracle.step(pd, force, torque, nsub=NSUB, hold=2, forced_ids=ids_sub, want_selection=True)
        selection_report(ids_sub, res["own"], res["margin"], "epoch step %d" % k, min_rate=0.985)
        ref.set_sim_state(res["dpos"].astype(np.float32), res["dvel"].astype(np.float32), res["rb"].astype(np.float32))
        ref.post_physics_step()
        rb = N(task._rigid_body_state).reshape(n, 24, 13)
        # the per-element, conditioning-aware bounds of the one-step tests on EVERY env at every step (flailing ragdolls included)
        bad = rows_close(rb[..., :3], res["rb"][..., :3], POS_ATOL, 0.0, "epoch step %d rb pos" % k, sens["rb"][..., :3], K_SENS)
        bad |= rows_close(rb[..., 7:], res["rb"][..., 7:], VEL_ATOL, VEL_RTOL, "epoch step %d rb vel" % k, sens["rb"][..., 7:], K_SENS)
        bad |= rows_close(N(task._dof_vel), res["dvel"], VEL_ATOL, VEL_RTOL, "epoch step %d dof vel" % k, sens["dvel"], K_SENS)
        bad |= rows_close(N(task._contact_forces), res["cf"], FORCE_ATOL, FORCE_RTOL, "epoch step %d contact force" % k, sens["cf"], K_SENS)
        assert_none_over(bad, "epoch step %d" % k)
        assert np.array_equal(N(task.progress_buf), ref.progress_buf), "progress, step %d" % k
        assert np.array_equal(N(task.reset_buf), ref.reset_buf), "reset flags, step %d: %d differ" % (k, (N(task.reset_buf) != ref.reset_buf).sum())
        assert np.array_equal(N(task._terminate_buf), ref.terminate_buf), "terminate flags, step %d" % k
        close(N(task.rew_buf), ref.rew_buf, 1e-3, "reward, step %d" % k)
        died = int(ref.reset_buf.sum())
    task.close()
    return died


def test_epoch_32_steps_sticky_resets_flag_for_flag():
    """One whole epoch (32 control steps, horizon_length of amass_im.yaml:137) with action noise large enough that humanoids fall:
    sticky reset / terminate flags (humanoid_smpl_im.py:724-739), zeroed rewards and masked actions of dead envs, compared flag for
    flag at every step against TaskOracle + the C physics oracle (terminated envs keep being simulated as ragdolls by both)."""
    from vid2player3d_amd import motion_tables, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    bm = load_baked_model()
    tabs = motion_tables.build_tables(synth.make_clips(5, 8, 90, 160), bm.parents, bm.local_pos)
    died = _epoch_against_oracles(MotionLib(tabs, DEV), tabs, 48, steps=32, seed=33, sigma=0.6)
    assert 4 <= died, "the fixture must make some humanoids terminate (got %d)" % died


@pytest.mark.parametrize("n", [1024, 8192])
def test_full_size_properties(mlib, n):
    """Size-independent invariants at the BASELINE env counts: finite state, unit quaternions, nothing
    tunnels the plane, contact forces push up, FK consistency of the exposed tensors, determinism."""
    def run():
        task = make_task(n, mlib)
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        for _ in range(6):
            a = torch.cat([task._target_dof_pos + 0.17 * torch.randn((n, 69), device=DEV, generator=g), 0.17 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            task.step(a)
        torch.cuda.synchronize()
        out = {k: getattr(task, k).clone() for k in ("obs_buf", "rew_buf", "reset_buf", "_rigid_body_state", "_contact_forces", "_dof_state")}
        task.close()
        return out
    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k], b[k]), "%s is not deterministic" % k
    rb = a["_rigid_body_state"].view(n, 24, 13)
    assert torch.isfinite(rb).all() and torch.isfinite(a["obs_buf"]).all() and torch.isfinite(a["rew_buf"]).all()
    assert (rb[..., 3:7].norm(dim=-1) - 1).abs().max() < 1e-4
    assert rb[..., 2].min() > -0.25
    assert a["_contact_forces"][..., 2].min() >= 0.0
    assert (a["rew_buf"] >= 0).all() and (a["rew_buf"] <= 1.0 + 1e-6).all()
    # root state == rigid body 0 ; obs is the concat of the exposed tensors
    assert torch.equal(a["obs_buf"][:, :72], rb[..., 0:3].reshape(n, 72))
    assert torch.equal(a["obs_buf"][:, 168:237], a["_dof_state"].view(n, 69, 2)[..., 0])


def test_both_schedules_agree(mlib):
    """link-per-lane (registers, level-synchronous) and env-per-lane (LDS) kernels evaluate the same model.  Each of them against the
    oracle on every env (one step from the same perturbed state, n not a multiple of 2, 32 or 64: tail handling of both kernels);
    then directly against each other on the envs where the two float32 kernels selected the same vertices in all four substeps
    (the others are ties of the selection rule, as the oracle comparison of each kernel has just shown)."""
    n = 130
    outs = []
    for sched in ("link_per_lane", "env_per_lane"):
        (got, ref), = _run_pair(mlib, n, contact=True, seed=5, lift=-0.05, what=sched, kernel_schedule=sched)
        _compare(got, ref, sched)
        outs.append(got)
    a, b = outs
    same = np.all(a["ids_sub"] == b["ids_sub"], axis=(1, 2, 3))
    print("[schedules] identical contact vertices in all substeps: %d of %d envs" % (same.sum(), n))
    assert same.mean() > 0.9
    close(a["rb"][same][..., :7], b["rb"][same][..., :7], 2e-5, "rb pose")
    close(a["rb"][same][..., 7:], b["rb"][same][..., 7:], 5e-4, "rb vel")
    close(a["dvel"][same], b["dvel"][same], 5e-4, "dof vel")
    close(a["cf"][same], b["cf"][same], 5e-3, "contact force")


@pytest.mark.parametrize("n", [1, 3, 65])
def test_small_and_ragged_env_counts(mlib, n):
    task = make_task(n, mlib)
    task.reset_with_times(None, torch.full((n,), 0.3, device=DEV))
    a = torch.cat([task._target_dof_pos.clone(), torch.zeros((n, 6), device=DEV)], dim=1).contiguous()
    for _ in range(2):
        task.step(a)
    torch.cuda.synchronize()
    rb = task._rigid_body_state.view(n, 24, 13)
    assert torch.isfinite(rb).all() and torch.isfinite(task.obs_buf).all()
    # every env was bound to the same clip position here, and clips repeat with period num_motions: env i and env i+8 match
    if n > 8:
        assert torch.allclose(rb[0], rb[8], atol=1e-6)
    task.close()


def test_env_pairing_is_invisible(mlib):
    """Envs are handed to waves in order of their contact load (v2p_sim_cfg.pair_envs_by_load); which env shares a wave with
    which must not change any env's numbers: paired and unpaired runs agree bit for bit over 6 control steps."""
    n = 257
    outs = []
    for pair in (False, True):
        task = make_task(n, mlib, pair_envs_by_load=pair, pair_mix_permille=300)
        g = torch.Generator(device=DEV)
        g.manual_seed(11)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        for _ in range(6):
            a = torch.cat([task._target_dof_pos + 0.3 * torch.randn((n, 69), device=DEV, generator=g), 0.3 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            task.step(a)
        torch.cuda.synchronize()
        outs.append([N(task._rigid_body_state), N(task._dof_state), N(task._contact_forces), N(task.dof_force_tensor), N(task.rew_buf), N(task.obs_buf),
                     N(task.debug_contacts())])
        if pair:
            perm, _ = task.debug_pairing()
            assert not np.array_equal(N(perm), np.arange(n)), "pairing must actually reorder the envs"
        task.close()
    assert (outs[0][6] >= 0).any()  # contacts were active
    for k, (x, y) in enumerate(zip(*outs)):
        assert np.array_equal(x, y), (k, float(np.abs(x.astype(np.float64) - y).max()), int((x != y).sum()), x.size)


@pytest.mark.parametrize("n", [3, 257, 8192])
def test_substep_jobs_are_invisible(mlib, n):
    """v2p_sim_cfg.substep_jobs: the physics launch cut into (substep, env pair) jobs that hand the state over through memory
    (system-scope stores / loads + a progress word per pair) must give bit-identical results to one workgroup per pair, step
    after step, under load (8192 envs = 16384 jobs on ~2048 wave slots: most hand-offs cross workgroups, CUs and XCDs)."""
    outs = []
    for jobs in (False, True):
        task = make_task(n, mlib, substep_jobs=2 * int(jobs))
        g = torch.Generator(device=DEV)
        g.manual_seed(17)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        snaps = []
        for k in range(12):
            a = torch.cat([task._target_dof_pos + 0.4 * torch.randn((n, 69), device=DEV, generator=g), 0.3 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            if k % 3 == 2:
                task.pre_physics_step(a); task._physics_step(); task.post_physics_step()  # the staged API takes the same path
            else:
                task.step(a)
            snaps.append([N(task._rigid_body_state).copy(), N(task._dof_state).copy(), N(task._contact_forces).copy(), N(task.dof_force_tensor).copy(),
                          N(task.rew_buf).copy(), N(task.reset_buf).copy(), N(task.debug_contacts()).copy()])
        task.check()
        outs.append(snaps)
        task.close()
    assert (outs[0][-1][6] >= 0).any()
    for k, (sa, sb) in enumerate(zip(*outs)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            assert np.array_equal(x, y), "step %d, tensor %d: %d of %d values differ (max %.3e)" % (k, j, int((x != y).sum()), x.size, float(np.abs(x.astype(np.float64) - y).max()))


@pytest.mark.parametrize("build", [1, 2])
@pytest.mark.parametrize("what,env", [("tgs", dict(contact_solver="tgs")), ("pd only", dict(enable_contact=False)), ("limits", dict(joint_limits=True)),
                                      ("limits tgs", dict(joint_limits=True, contact_solver="tgs")), ("vfric", dict(friction_frame="velocity"))])
def test_substep_jobs_are_invisible_in_every_instantiation(mlib, what, env, build):
    """TGS, the contact-free kernel and the joint-limit kernel cut into substep jobs (forced: at this size the engine would keep whole
    control steps per workgroup) == one workgroup per env pair, bit for bit, over several steps incl. the fused post-physics; in either
    build of the kernel (v2p_sim_cfg.kernel_build)."""
    n = 1500
    env = dict(env, kernel_build=build)
    if what.startswith("limits"):
        from vid2player3d_amd.model import load_baked_model
        from vid2player3d_amd.racket import with_racket

        env = dict(env, body_model=with_racket(load_baked_model())[0])
    outs = []
    for jobs in (0, 2):
        task = make_task(n, mlib, substep_jobs=jobs, **env)
        g = torch.Generator(device=DEV)
        g.manual_seed(31)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        snaps = []
        for k in range(6):
            a = torch.cat([task._target_dof_pos + 0.4 * torch.randn((n, 69), device=DEV, generator=g), 0.3 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            task.step(a)
            snaps.append([N(task._rigid_body_state).copy(), N(task._dof_state).copy(), N(task._contact_forces).copy(), N(task.dof_force_tensor).copy(),
                          N(task.rew_buf).copy(), N(task.reset_buf).copy(), N(task.obs_buf).copy()])
        task.check()
        outs.append(snaps)
        task.close()
    for k, (sa, sb) in enumerate(zip(*outs)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            assert np.array_equal(x, y), "%s step %d, tensor %d: %d of %d values differ" % (what, k, j, int((x != y).sum()), x.size)


def test_a_job_that_gives_up_waiting_recomputes_and_changes_nothing(mlib):
    """Forward progress of the substep jobs must not rest on the dispatch order.  With the time-out set to zero polls every job whose
    predecessor has not finished at its first look gives up at once and recomputes the pair's earlier substeps itself, while the
    predecessor still runs (and later rewrites the same values): results stay bit-identical to whole control steps per workgroup, with
    and without the ball (whose per-call flags and accumulators must not be touched by a replay)."""
    import warnings

    n = 4096
    outs = []
    for jobs, spins in ((False, 0), (True, -1)):  # v2p_sim_cfg.job_timeout_spins < 0: give up at the first look
        task = make_task(n, mlib, substep_jobs=2 * int(jobs), job_timeout_spins=spins)
        g = torch.Generator(device=DEV)
        g.manual_seed(29)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        snaps = []
        for k in range(8):
            a = torch.cat([task._target_dof_pos + 0.4 * torch.randn((n, 69), device=DEV, generator=g), 0.3 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            task.step(a)
            snaps.append([N(task._rigid_body_state).copy(), N(task._dof_state).copy(), N(task._contact_forces).copy(), N(task.rew_buf).copy(), N(task.reset_buf).copy(),
                          N(task.obs_buf).copy()])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            task.check()
        if jobs:
            assert task.job_recoveries() > 100, "the fixture must exercise the recovery path (%d)" % task.job_recoveries()
        else:
            assert task.job_recoveries() == 0
        outs.append(snaps)
        task.close()
    for k, (sa, sb) in enumerate(zip(*outs)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            assert np.array_equal(x, y), "step %d, tensor %d: %d of %d values differ (max %.3e)" % (k, j, int((x != y).sum()), x.size, float(np.abs(x.astype(np.float64) - y).max()))


@pytest.mark.parametrize("job_len", [None, 2, 5])
def test_substep_jobs_with_twelve_substeps_per_control_step(mlib, job_len):
    """sim.substeps 6 x controlFrequencyInv 2 = 12 substeps per control step (vid2player's controller configs,
    vid2player/cfg/*.yaml `substeps: 6`): the progress word of a pair counts launch x (nsub + 1) + substep, so the hand-overs of one
    launch can never satisfy the waits of the next (with the stride fixed at 8 they did from nsub = 9 on).  Jobs on == jobs off, bit
    for bit, over several launches."""
    # job_len: substeps per job (the engine takes 2 for launches with plenty of jobs; 5: an uneven split of the 12, 5 + 5 + 2)
    n = 4096
    outs = []
    for jobs in (False, True):
        task = make_task(n, mlib, sim_overrides={"substeps": 6}, substep_jobs=2 * int(jobs), job_len=(job_len or 0) if jobs else 0)
        assert task.sim_params.substeps * task.control_freq_inv == 12
        g = torch.Generator(device=DEV)
        g.manual_seed(23)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        snaps = []
        for k in range(6):
            a = torch.cat([task._target_dof_pos + 0.4 * torch.randn((n, 69), device=DEV, generator=g), 0.3 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            task.step(a)
            snaps.append([N(task._rigid_body_state).copy(), N(task._dof_state).copy(), N(task._contact_forces).copy(), N(task.rew_buf).copy(), N(task.reset_buf).copy()])
        task.check()
        outs.append(snaps)
        task.close()
    for k, (sa, sb) in enumerate(zip(*outs)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            assert np.array_equal(x, y), "step %d, tensor %d: %d of %d values differ (max %.3e)" % (k, j, int((x != y).sum()), x.size, float(np.abs(x.astype(np.float64) - y).max()))


@pytest.mark.parametrize("n,mix", [(2, 0), (3, 250), (1000, 0), (1000, 250), (8195, 250), (8195, 500)])
def test_pairing_order_is_a_descending_permutation(mlib, n, mix):
    """The wave order for the next launch is a permutation of the envs; read by RANK it has non-increasing contact-load keys (counting
    sort spread over the physics and pre-physics kernels), and rank r sits in slot 2r (r < m), 2 (n-1-r) + 1 (r >= n - m), r + m
    (otherwise), m = n x pair_mix_permille / 1000: the m heaviest envs share their waves with the m lightest, the rest pair by rank.
    Also when pre-physics is not called between physics launches."""
    task = make_task(n, mlib, pair_mix_permille=mix)
    m = min(n * mix // 1000, n // 2)
    slots = np.arange(n)
    rank_of_slot = np.where(slots < 2 * m, np.where(slots % 2 == 0, slots // 2, n - 1 - (slots - 1) // 2), slots - m)
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
    a = torch.cat([task._target_dof_pos + 0.5 * torch.randn((n, 69), device=DEV, generator=g), torch.zeros((n, 6), device=DEV)], dim=1).contiguous()

    def check():
        perm, key = task.debug_pairing()
        torch.cuda.synchronize()
        if n <= 2:  # a single wave: no pairing
            return
        pm, kp = N(perm).astype(np.int64), N(key).astype(np.int64)
        assert np.array_equal(np.sort(pm), np.arange(n)) and np.array_equal(np.sort(rank_of_slot), np.arange(n))
        by_rank = np.empty(n, np.int64)
        by_rank[rank_of_slot] = kp[pm]
        assert np.all(np.diff(by_rank) <= 0)
        assert n < 1000 or len(np.unique(kp)) > 3

    for _ in range(3):
        task.step(a.clone())
    check()
    task.step_fused(a.clone())
    task.step_fused(a.clone())
    check()
    for _ in range(3):  # physics only: the scatter falls back to its own small kernel
        task._physics_step()
    check()
    task.step(a.clone())
    check()
    task.close()


def test_per_env_body_shapes_match_oracle():
    """One body shape per clip (the reference builds one asset per clip from its betas / scale, humanoid_smpl_im.py:255-296):
    eight uniformly scaled variants of the body, env i simulates the shape of its clip; every env against its own oracle."""
    from vid2player3d_amd import synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    base = load_baked_model()
    shapes = [base.scaled(s) for s in (0.85, 0.9, 0.95, 1.0, 1.05, 1.1, 1.15, 1.2)]
    assert abs(shapes[0].total_mass / base.total_mass - 0.85 ** 3) < 1e-9
    clips = synth.make_clips(5, 8, 60, 120)
    lib = MotionLib.from_clips(clips, shapes, DEV)
    for contact, lift, seed in ((False, 0.0, 41), (True, -0.05, 42)):
        (got, ref), = _run_pair(lib, 48, contact, seed, lift=lift, shapes=shapes, what="scaled shapes")
        if contact:
            assert (got["ids"] >= 0).any(axis=(1, 2)).mean() > 0.8
        _compare(got, ref, "shapes contact=%s" % contact, contact=contact)
    # the shapes really differ: pelvis height of the rest pose scales with the body
    t = make_task(16, lib, body_model=shapes)
    h = N(t.smpl_rest_joints)[:, :, :].copy()
    assert not np.allclose(h[0], h[7])
    with pytest.raises(RuntimeError):
        t.set_schedule("env_per_lane")  # the cross-check kernel is single-shape
    t.close()


def test_non_uniform_body_shapes_match_oracle():
    """Per-clip assets from vertex clouds (body_shapes.py: own hulls, reduced to <= 64 vertices, hull-integrated mass properties):
    eight NON-uniform shapes - limb proportions, girth, shoulder width differ, so hull topology and mass ratios do - one per clip;
    every env against the oracle of its own shape, with and without contacts."""
    from vid2player3d_amd import body_shapes, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    base = load_baked_model()
    shapes = body_shapes.synthetic_shape_family(base, 8, seed=1)
    assert len({tuple(np.diff(m.hull_offsets)) for m in shapes}) > 1  # different vertex counts per body: different hull topology
    lib = MotionLib.from_clips(synth.make_clips(6, 8, 60, 120), shapes, DEV)
    for contact, lift, seed in ((False, 0.0, 51), (True, -0.05, 52), (True, -0.7, 53)):
        (got, ref), = _run_pair(lib, 48, contact, seed, lift=lift, shapes=shapes, what="non-uniform shapes")
        _compare(got, ref, "non-uniform shapes contact=%s lift=%.2f" % (contact, lift), contact=contact)


def test_fused_step_equals_staged_step(mlib):
    """v2p_env_step (pre-physics inside the physics kernel's prologue, post-physics in its epilogue, both compiled with precise
    semantics there) against pre_physics + physics + post_physics as separate kernels: bit-identical state, observations, rewards,
    masks, times and targets over 3 steps; dead envs get their action rows zeroed in place by both."""
    n = 96
    outs = []
    for fused in (False, True):
        task = make_task(n, mlib)
        g = torch.Generator(device=DEV)
        g.manual_seed(23)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        task.reset_buf[::5] = 1  # some dead envs
        acts = []
        for _ in range(3):
            a = torch.cat([task._target_dof_pos + 0.2 * torch.randn((n, 69), device=DEV, generator=g), 0.5 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            if fused:
                task.step_fused(a)
            else:
                task.pre_physics_step(a)
                task._physics_step()
                task.post_physics_step()
            acts.append(N(a))
        torch.cuda.synchronize()
        outs.append({"acts": np.stack(acts), "pd": N(task._pd_target), "rb": N(task._rigid_body_state), "dof": N(task._dof_state), "obs": N(task.obs_buf),
                     "rew": N(task.rew_buf), "reset": N(task.reset_buf), "ids": N(task.debug_contacts()),
                     # post-physics runs in the epilogue of the physics kernel in the fused step, as its own kernel in the staged one
                     "sub_rewards": N(task._sub_rewards), "terminate": N(task._terminate_buf), "progress": N(task.progress_buf),
                     "cur_time": N(task._cur_ref_motion_times), "target0": N(task._target_bufs[0]), "target1": N(task._target_bufs[1]),
                     "target_dof_pos": N(task._target_dof_pos)})
        task.close()
    a, b = outs
    assert (a["acts"][:, ::5] == 0).all() and (a["acts"][:, 1] != 0).any()
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s differs between the fused and the staged step (max %.3e)" % (k, np.abs(a[k].astype(np.float64) - b[k]).max())


def test_full_size_sample_matches_oracle(mlib):
    """8192 envs on the GPU (4096 waves, paired by contact load), 64 of them - first, last, and a spread in between - against
    their own float64 oracles, all compared: indexing, pairing and the tail of the launch at the BASELINE size."""
    n = 8192
    subset = sorted(set([0, 1, 2, n - 1, n - 2] + list(np.random.default_rng(8).integers(0, n, size=59))))
    (got, ref), = _run_pair(mlib, n, contact=True, seed=6, lift=0.0, subset=subset, what="8192-env sample")
    _compare(got, ref, "8192-env sample")


def test_full_size_sample_with_one_body_shape_per_clip_at_amass_scale():
    """The reference's real body configuration at its scale (humanoid_smpl_im.py:247-296: every env simulates the SMPL body of its clip;
    AMASS = thousands of clips): 2048 non-uniform shapes compiled on the device (v2p_shapes_compile), 2048 clips - each built on its
    own skeleton -, 8192 envs, env i -> clip i % 2048 -> its shape; 64 sampled envs, each against the float64 oracle of ITS shape."""
    from vid2player3d_amd import body_shapes, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    n, S = 8192, 2048
    base = load_baked_model()
    shapes = body_shapes.synthetic_shape_family(base, S, seed=21, device=DEV)
    lib = MotionLib.from_clips(synth.make_clips(9, S, 40, 80), shapes, DEV)
    subset = sorted(set([0, 1, S - 1, S, n - 1, n - 2] + list(np.random.default_rng(9).integers(0, n, size=58))))
    for contact, lift, seed in ((True, -0.05, 71), (True, -0.7, 72)):
        (got, ref), = _run_pair(lib, n, contact, seed, lift=lift, vel_sigma=0.5 if lift > -0.5 else 0.2, shapes=shapes, subset=subset, what="2048 shapes lift %.2f" % lift)
        assert (got["ids"] >= 0).any(axis=(1, 2)).mean() > 0.8
        _compare(got, ref, "2048 shapes lift %.2f" % lift)
    t = make_task(n, lib, body_model=shapes)
    ids = np.asarray(t._env_shape_ids)
    assert np.array_equal(ids, np.arange(n) % S) and len(np.unique(np.round(t.humanoid_masses, 6))) > 2000
    t.close()


def test_freeze_terminated_envs_option(mlib):
    """cfg['env']['freeze_terminated_envs'] (opt-in, not the reference's behaviour): envs whose reset flag is set stop moving, every
    other env's numbers are bit-identical to the default engine's (and so are rewards / reset flags, which never read dead envs)."""
    n = 200
    STEPS = 40
    outs = []
    for freeze in (False, True):
        task = make_task(n, mlib, freeze_terminated_envs=freeze)
        g = torch.Generator(device=DEV)
        g.manual_seed(31)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.5)
        snaps = []
        for k in range(STEPS):
            a = torch.cat([task._target_dof_pos + 1.0 * torch.randn((n, 69), device=DEV, generator=g), 2.0 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            task.step(a)
            snaps.append((N(task.reset_buf).copy(), N(task._rigid_body_state).reshape(n, 24, 13).copy(), N(task.rew_buf).copy(), N(task._dof_state).copy()))
        torch.cuda.synchronize()
        outs.append(snaps)
        task.close()
    ref, frz = outs
    died = 0
    for k in range(STEPS):
        assert np.array_equal(ref[k][0], frz[k][0])  # same envs terminate at the same steps
        assert np.array_equal(ref[k][2], frz[k][2])  # same rewards
        alive_before = (ref[k - 1][0] == 0) if k else np.ones(n, bool)  # simulated in step k by both engines
        assert np.array_equal(ref[k][1][alive_before], frz[k][1][alive_before])
        assert np.array_equal(ref[k][3].reshape(n, -1)[alive_before], frz[k][3].reshape(n, -1)[alive_before])
        if k:
            dead = ref[k - 1][0] == 1
            died = max(died, int(dead.sum()))
            assert np.array_equal(frz[k][1][dead], frz[k - 1][1][dead])  # frozen
            if dead.any():
                assert not np.array_equal(ref[k][1][dead], ref[k - 1][1][dead])  # the default keeps simulating them
    assert died > 10


def test_free_fall_at_full_size(mlib):
    """A size-independent property at BASELINE's env count: 8192 humanoids in free fall (contacts off, the PD targets at the current pose,
    no joint motion, no spin) - in every control step every link of every env gains g x dt of vertical velocity and falls by the
    semi-implicit distance sum_k h (v + k h g), whatever its env's initial velocity."""
    n = 8192
    task = make_task(n, mlib, enable_contact=False)
    torch.manual_seed(1)
    task.reset()
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    v = torch.randn((n, 3), device=DEV, generator=g)
    task._humanoid_root_states[:, 2] += 3.0
    task._humanoid_root_states[:, 7:10] = v
    task._humanoid_root_states[:, 10:13] = 0.0
    task._dof_vel.zero_()
    task._reset_env_tensors(None)
    actions = torch.cat([task._dof_pos, torch.zeros((n, 6), device=DEV)], dim=1).contiguous()  # PD target = the current pose: no drive torque
    nsub, gz = 4, -9.81
    h = task.dt / nsub
    x_before = None
    for step in range(2):
        task.step(actions.clone())
        torch.cuda.synchronize()
        v_after = v + torch.tensor([0.0, 0.0, gz * task.dt], device=DEV)
        assert (task._rigid_body_vel - v_after[:, None, :]).abs().max() < 2e-4
        assert task._rigid_body_ang_vel.abs().max() < 2e-4 and task._dof_vel.abs().max() < 2e-4
        if x_before is not None:  # (the rigid-body tensor of before the first step still shows the clip's pose, not the engine's)
            fall = sum(h * (v + torch.tensor([0.0, 0.0, gz * h * (k + 1)], device=DEV)) for k in range(nsub))
            assert (task._rigid_body_pos - x_before - fall[:, None, :]).abs().max() < 2e-5
        x_before, v = task._rigid_body_pos.clone(), v_after
    task.close()


def test_rest_contact_supports_the_weight_at_full_size(mlib):
    """Another property that needs no reference: 8192 humanoids dropped flat from the default pose (root 0.89 m up, joints at zero) come
    to rest on the plane - no sinking, no creeping, and the exposed net contact forces (those of the step's last substep) carry the
    weight: within 15 % in every step, within 5 % averaged over 15 steps."""
    from vid2player3d_amd.model import load_baked_model

    n = 8192
    task = make_task(n, mlib, stateInit="Default")
    task.reset()
    weight = load_baked_model().total_mass * 9.81
    act = torch.zeros((n, 75), device=DEV)
    ratios, heights = [], []
    for k in range(30):
        task.step(act.clone())
        if k >= 15:
            ratios.append(task._contact_forces[..., 2].sum(dim=1) / weight)
            heights.append(task._rigid_body_pos[:, 0, 2].clone())
    r, z = torch.stack(ratios), torch.stack(heights)
    assert torch.isfinite(r).all() and float(r.min()) > 0.85 and float(r.max()) < 1.15, (float(r.min()), float(r.max()))
    assert abs(float(r.mean()) - 1.0) < 0.05, float(r.mean())
    assert float((z - z[0]).abs().max()) < 2e-3 and float(z.min()) > 0.05  # lying on the plane, not in it
    assert float(task._rigid_body_vel.abs().max()) < 0.2
    task.close()


@pytest.mark.parametrize("frame", ["world", "velocity"])
def test_engine_obeys_the_closed_form_friction_law(mlib, frame):
    """(frame = velocity, v2p_sim_cfg.friction_frame 1: t1 along the tangential velocity of the point under v* - the limit is mu in every
    direction: the diagonal push lets go at 1.3 with (alpha - mu) g, where the world-aligned box still holds.)
    Closed-form facts of the contact model, on the HIP ENGINE itself (tests/test_phys_oracle.py checks the same on the float64 oracle):
    a rigid box on the plane (the root link of a 24-link model whose other links are 0.1 g points on stiff drives, far from the ground),
    pushed horizontally at its centre of mass with alpha x its weight through the residual-force actions (a slope of tan(theta) = alpha),
    mu = 1: along a tangent axis it sticks at alpha = 0.9 and slides with (alpha - mu) g at 1.1; along the DIAGONAL it still sticks at 1.3
    and slides with (alpha - sqrt(2) mu) g at 1.5 - the friction limit is a pyramid aligned with world x / y (box friction per tangent row)."""
    from scipy.spatial.transform import Rotation

    from tests.test_phys_oracle import box_model
    from vid2player3d_amd.model import load_baked_model

    BASEQ = np.array([0.5, 0.5, 0.5, 0.5])
    R = Rotation.from_quat(BASEQ).as_matrix()                      # body -> world at the root pose of the test (SMPL y-up body, z-up world)
    half_world = np.array([0.25, 0.25, 0.1])
    half_body = np.abs(R.T) @ half_world
    bm = box_model(load_baked_model(), half=tuple(half_body), mass=10.0)
    up_body = R.T @ np.array([0.0, 0.0, 1.0])                      # the 23 point links stack upwards in the WORLD
    lp = bm.blob["local_pos"].copy()
    lp[1:] = 0.05 * up_body
    blob = dict(bm.blob, local_pos=lp)
    from vid2player3d_amd.model import BodyModel
    bm = BodyModel(blob, default_humanoid_mass=float(bm.mass.sum()))
    cases = [(0.9, (1, 0)), (1.1, (1, 0)), (1.3, (1, 1)), (1.5, (1, 1)), (0.9, (0, 1)), (1.1, (0, -1)), (0.9, (1, 1)), (1.3, (0.3, -1.0))]
    n = len(cases)
    task = make_task(n, mlib, body_model=bm, residual_force_hold="all", terminationHeadHeight=-0.5, enableEarlyTermination=False, debug_contacts=1, friction_frame=frame)
    assert task.friction_frame == frame
    task.reset_with_times(None, torch.full((n,), 0.1, device=DEV))
    root = np.zeros((n, 13), np.float32)
    root[:, 2], root[:, 3:7] = 0.1, BASEQ
    task._humanoid_root_states[:] = T(root)
    task._dof_pos.zero_()
    task._dof_vel.zero_()
    task._reset_env_tensors(None)
    weight = bm.total_mass * 9.81
    act = np.zeros((n, 75), np.float32)
    for _ in range(10):  # settle
        task.step(T(act.copy()))
    dirs = np.array([np.array(d, np.float64) / np.linalg.norm(d) for _, d in cases])
    for e, (alpha, _) in enumerate(cases):
        act[e, 69:71] = alpha * weight * dirs[e] / 31.85
    v = []
    for _ in range(30):
        task.step(T(act.copy()))
        v.append(N(task._humanoid_root_states)[:, 7:9].copy())
    torch.cuda.synchronize()
    assert int(N(task.reset_buf).sum()) == 0                       # (no env was reset: the pushes acted for all 30 steps)
    ids = N(task.debug_contacts())
    assert np.all((ids[:, 0] >= 0).sum(axis=1) == 4) and np.all(ids[:, 1:] < 0)    # the boxes rest on their four bottom corners
    fz = N(task._contact_forces)[:, :, 2].sum(axis=1)
    assert np.all(np.abs(fz - weight) < 0.02 * weight)
    v = np.array(v)                                                # [steps, env, 2]
    t = 30 / 30.0
    mu = 1.0
    for e, (alpha, d) in enumerate(cases):
        along = v[:, e] @ dirs[e]
        dn = np.abs(dirs[e])
        # world frame: a box aligned with x / y - each component of the push is held up to mu on its own, what exceeds it accelerates that axis;
        # velocity frame: the limit is mu along the push
        acc = np.sign(dirs[e]) * np.maximum(alpha * dn - mu, 0.0) * 9.81 if frame == "world" else dirs[e] * max(alpha - mu, 0.0) * 9.81
        want = float(acc @ dirs[e]) * t
        if want == 0.0:
            assert np.abs(v[-10:, e]).max() < 1e-2 and abs(along[-1] - along[-11]) / (10 / 30.0) < 0.005 * 9.81, (e, alpha, np.abs(v[-10:, e]).max())
        else:
            assert abs(along[-1] - want) < 0.06 * want and np.all(np.diff(along) > 0), (e, alpha, along[-1], want)
            if frame == "velocity":  # ... and the box slides ALONG the push, not along a world axis
                assert np.linalg.norm(v[-1, e] - along[-1] * dirs[e]) < 0.03 * want, (e, v[-1, e], along[-1] * dirs[e])
    task.close()
