"""The imitation target from the motion generator's pose on the device: `v2p_mvae_target_step` / `_reset` / `_actions` on what the
reference itself computed (tests/golden/mvae_target.npz), `ImitationTarget.compute_observations`, and the control step of
`TennisControllerTask` with a motion generator and a target attached on a racket + ball batch."""
import types

import numpy as np
import pytest
import torch

from tests import mvae_target_fixture as FX
from vid2player3d_amd import mvae_target as mt

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def N(t):
    return t.detach().cpu().numpy()


def step_tensors(g, v, t, n, prev_target=None):
    """Device tensors of step t of variant v for n envs (fixture rows repeated), the outputs poisoned, one guard row behind the target."""
    s = FX.step_inputs(g, v, t)
    idx = np.arange(n) % len(s["root_pos"])
    ball, rb = np.full((n, 13), NAN, np.float32), np.full((n, 24, 13), NAN, np.float32)
    ball[:, 0:3], rb[:, 0, 0:3] = s["ball_pos"][idx], s["sim_root_pos"][idx]
    whole = torch.full((n + 1, mt.ROW), NAN, device=DEV)
    d = dict(root_pos=T(s["root_pos"][idx]), joint_rotmat=T(s["joint_rotmat"][idx]), residual_root=None if s["residual_root"] is None else T(s["residual_root"][idx]),
             ball_state=T(ball), joint_pos_bind=T(s["joint_pos_bind"]), env_shape_id=T(s["env_shape_id"][idx], torch.int32), target=whole[:n],
             prev_target=T(s["prev_target"][idx]) if prev_target is None else prev_target, rb_state=T(rb),
             hold_reset=torch.full((n,), 7, dtype=torch.int64, device=DEV), hold_progress=torch.full((n,), 5, dtype=torch.int64, device=DEV),
             hold_cur_time=torch.full((n,), 3.3, device=DEV))
    return d, whole, idx


@gpu
@pytest.mark.parametrize("n", [None, 1, 3, 33, 65])
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_step_kernel_matches_the_reference_step_by_step(v, n):
    """every step teacher-forced from the recorded state, outputs poisoned beforehand, every env compared; what the step only reads
    comes back bit-identical; n: the fixture's rows, or rows repeated to a lone half wave, an odd env, partial last waves and workgroups"""
    g = FX.golden()
    st = FX.settings(g, v)
    sc = FX.scatter_of(g, "step")
    rows = len(g[v + "/env_shape_id"]) if n is None else n
    for t in range(FX.steps(g, v)):
        d, whole, idx = step_tensors(g, v, t, rows)
        before = {k: N(x).copy() for k, x in d.items() if x is not None}
        mt.launch_step(st, d, rows, len(g[v + "/joint_pos_bind"]))
        torch.cuda.synchronize()
        what = "variant %s, %d envs, step %d" % (v, rows, t)
        FX.assert_row(N(d["target"]), g[v + "/target"][t + 1][idx], sc, what)
        assert np.isnan(N(whole)[rows]).all(), what + ": the row behind the last env was written"
        for k in ("root_pos", "residual_root", "ball_state", "joint_pos_bind", "env_shape_id", "prev_target", "rb_state"):
            if k in before:
                assert np.array_equal(before[k], N(d[k]), equal_nan=True), "%s: the kernel wrote %s" % (what, k)
        got = N(d["joint_rotmat"])
        FX.assert_close(got, FX.expected_rotmat(g, v, t, st)[idx], sc["joint_rotmat"], what + ": joint_rotmat")
        others = [j for j in range(24) if not st["fix_head_orientation"] or j not in (st["smpl_head"], st["smpl_neck"])]
        assert np.array_equal(got[:, others], before["joint_rotmat"][:, others]), what + ": a joint other than Head and Neck was written"
        assert not N(d["hold_reset"]).any() and not N(d["hold_progress"]).any() and not N(d["hold_cur_time"]).any(), what + ": the wrapped task's clocks are not held"


@gpu
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_free_run_follows_the_recorded_sequence(v):
    g = FX.golden()
    st = FX.settings(g, v)
    n, shapes = len(g[v + "/env_shape_id"]), len(g[v + "/joint_pos_bind"])
    bufs = [torch.full((n, mt.ROW), NAN, device=DEV) for _ in range(2)]
    r = FX.reset_inputs(g, v)
    reset = dict(root_pos=T(r["root_pos"]), joint_rotmat=T(r["joint_rotmat"]), joint_pos_bind=T(r["joint_pos_bind"]), env_shape_id=T(r["env_shape_id"], torch.int32), target=bufs[0])
    mt.launch_reset(st, reset, n, torch.arange(n, device=DEV), shapes)
    FX.assert_close(N(bufs[0]), g[v + "/target"][0], FX.scatter_of(g, "reset")["target"], "variant %s reset" % v)
    sc, cur = FX.scatter_of(g, "free"), 1
    for t in range(FX.steps(g, v)):
        d, _, _ = step_tensors(g, v, t, n, prev_target=bufs[1 - cur])
        d["target"] = bufs[cur]
        mt.launch_step(st, d, n, shapes)
        FX.assert_row(N(bufs[cur]), g[v + "/target"][t + 1], sc, "variant %s free run, step %d" % (v, t))
        cur = 1 - cur


@gpu
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_reset_of_an_id_list(v):
    """the named rows match the fixture, all other rows of all five buffers are bit-identical, velocities are exactly zero"""
    g = FX.golden()
    st = FX.settings(g, v)
    n, shapes = len(g[v + "/env_shape_id"]), len(g[v + "/joint_pos_bind"])
    rng = np.random.default_rng(3)
    r = FX.reset_inputs(g, v)
    d = dict(root_pos=T(r["root_pos"]), joint_rotmat=T(r["joint_rotmat"]), joint_pos_bind=T(r["joint_pos_bind"]), env_shape_id=T(r["env_shape_id"], torch.int32),
             target=T(rng.normal(size=(n, mt.ROW))), root_states=T(rng.normal(size=(n, 13))), dof_state=T(rng.normal(size=(n, 69, 2))), rb_state=T(rng.normal(size=(n, 24, 13))))
    before = {k: N(x).copy() for k, x in d.items()}
    mt.launch_reset(st, d, n, torch.as_tensor([3, n, 0, -1, n - 1, 6], device=DEV), shapes)
    torch.cuda.synchronize()
    got = {k: N(x) for k, x in d.items()}
    named = [3, 0, n - 1, 6]
    others = [e for e in range(n) if e not in named]
    for k in before:
        rows = others if k in ("target", "root_states", "dof_state", "rb_state") else slice(None)
        assert np.array_equal(before[k][rows], got[k][rows]), "variant %s: rows of other envs (or an input) written in %s" % (v, k)
    want = g[v + "/target"][0][named]
    FX.assert_close(got["target"][named], want, FX.scatter_of(g, "reset")["target"], "variant %s reset rows" % v)
    row = mt.unpack_row(got["target"][named])
    for k in ("root_vel", "root_ang_vel", "dof_vel"):
        assert not row[k].any(), k
    assert np.array_equal(row["key_pos"], row["rb_pos"].reshape(4, 24, 3)[:, st["key_bodies"]].reshape(4, 12))
    assert np.array_equal(got["root_states"][named, 0:3], row["root_pos"]) and np.array_equal(got["root_states"][named, 3:7], row["root_rot"])
    assert not got["root_states"][named, 7:].any() and not got["dof_state"][named][..., 1].any() and not got["rb_state"][named][..., 7:].any()
    assert np.array_equal(got["dof_state"][named][..., 0], row["dof_pos"])
    assert np.array_equal(got["rb_state"][named][..., 0:3].reshape(4, 72), row["rb_pos"]) and np.array_equal(got["rb_state"][named][..., 3:7].reshape(4, 96), row["rb_rot"])


@gpu
@pytest.mark.parametrize("no_scale", [False, True])
@pytest.mark.parametrize("base", sorted(mt.PD_TARGET_BASES))
def test_actions_kernel_gives_the_pd_targets_before_the_clamp(base, no_scale):
    g = FX.golden()
    st = FX.settings(g, "H", pd_target_base=base, no_scale_action=no_scale)
    a = T(g["actions/in"])
    n = len(a)
    out = torch.full((n + 1, 75), NAN, device=DEV)
    d = dict(target=T(g["actions/target"]), dof_state=T(np.stack([g["actions/dof_pos"], np.full_like(g["actions/dof_pos"], NAN)], -1)),
             pd_action_scale=T(g["actions/pd_action_scale"]), pd_action_offset=T(g["actions/pd_action_offset"]))
    mt.launch_actions(st, d, n, a, out[:n])
    torch.cuda.synchronize()
    name = "%s/%d" % (base, int(no_scale))
    FX.assert_close(N(out)[:n, :69], g["actions/out/" + name], FX.scatter_of(g, "actions")[name], "pd targets " + name)
    assert np.array_equal(N(out)[:n, 69:], g["actions/in"][:, 69:]) and np.isnan(N(out)[n]).all()
    assert np.array_equal(N(a), g["actions/in"])


def stand_in(g, v):
    """A task and a player that carry the fixture's tensors under the names ImitationTarget reads."""
    m = FX.model()
    n = len(g[v + "/env_shape_id"])
    shapes = g[v + "/env_shape_id"] if len(g[v + "/joint_pos_bind"]) > 1 else None
    task = types.SimpleNamespace(device=DEV, num_envs=n, pd_tar_lim=np.pi / 2, dt=FX.DT, body_names=list(m.body_names), body_model=m, racket_players=None,
                                 _key_body_ids=torch.as_tensor([list(m.body_names).index(b) for b in FX.KEY_BODIES]), _env_shape_ids=shapes,
                                 _target_bufs=[torch.full((n, mt.ROW), NAN, device=DEV) for _ in range(2)], _cur=0, _rigid_body_state=T(g[v + "/in/rb_state"]).view(n * 24, 13),
                                 _dof_state=T(g[v + "/in/dof_state"]).view(n * 69, 2), _ball_root_states=torch.zeros((n, 13), device=DEV),
                                 _humanoid_root_states=torch.zeros((n, 13), device=DEV), reset_buf=torch.ones(n, dtype=torch.long, device=DEV),
                                 progress_buf=torch.ones(n, dtype=torch.long, device=DEV), _cur_ref_motion_times=torch.ones(n, device=DEV), pushed=[])
    task._reset_env_tensors = lambda ids, with_rb_state=False: task.pushed.append((N(ids).tolist(), with_rb_state))
    player = types.SimpleNamespace(device=DEV, num_envs=n, _root_pos=torch.zeros((n, 3), device=DEV), _joint_rotmat=torch.zeros((n, 24, 3, 3), device=DEV))
    cfg = {"v2p": {"fix_head_orientation": bool(g[v + "/settings"][0]), "add_residual_root": bool(g[v + "/settings"][2]), "smpl_beta": np.linspace(-0.5, 0.5, 10)},
           "env": {"no_scale_action": True}}
    return task, player, mt.ImitationTarget(task, player, g[v + "/joint_pos_bind"], cfg)


@gpu
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_object_steps_resets_and_observes_like_the_reference(v):
    """`ImitationTarget` on stand-ins that carry the fixture: reset, then every step from the recorded previous target; the observation
    of the recorded target against the recorded obs_buf"""
    g = FX.golden()
    task, player, target = stand_in(g, v)
    n = task.num_envs
    player._root_pos.copy_(T(g[v + "/in/root_pos"][0]))
    player._joint_rotmat.copy_(T(g[v + "/in/joint_rotmat"][0]))
    keep = task._rigid_body_state.clone(), task._dof_state.clone()
    target.reset(torch.arange(n, device=DEV))
    assert task.pushed == [(list(range(n)), True)]
    FX.assert_close(N(task._target_bufs[1]), g[v + "/target"][0], FX.scatter_of(g, "reset")["target"], "variant %s: reset into the previous target" % v)
    assert np.isnan(N(task._target_bufs[0])).all()
    FX.assert_close(N(task._rigid_body_state).reshape(n, 24, 13)[..., 0:3].reshape(n, 72), g[v + "/target"][0][:, 163:235], FX.scatter_of(g, "reset")["target"], "reset rb_state")
    task._rigid_body_state.copy_(keep[0])
    task._dof_state.copy_(keep[1])
    sc = FX.scatter_of(g, "step")
    for t in range(FX.steps(g, v)):
        s = FX.step_inputs(g, v, t)
        task._target_bufs[1 - task._cur].copy_(T(s["prev_target"]))
        player._root_pos.copy_(T(s["root_pos"]))
        player._joint_rotmat.copy_(T(s["joint_rotmat"]))
        task._ball_root_states[:, 0:3] = T(s["ball_pos"])
        body0 = task._rigid_body_state.view(n, 24, 13)[:, 0, 0:3]
        sim_root = body0.clone()
        body0.copy_(T(s["sim_root_pos"]))  # (the simulated root of the head rule's miss test)
        task.reset_buf.fill_(1)
        target.step(None if s["residual_root"] is None else T(s["residual_root"]))
        body0.copy_(sim_root)
        what = "variant %s object step %d" % (v, t)
        FX.assert_row(N(task._target_bufs[task._cur]), g[v + "/target"][t + 1], sc, what)
        assert not N(task.reset_buf).any() and not N(task.progress_buf).any() and not N(task._cur_ref_motion_times).any()
        task._target_bufs[task._cur].copy_(T(g[v + "/target"][t + 1]))
        obs = target.compute_observations()
        FX.assert_close(N(obs), g[v + "/out/obs"][t], sc["obs"], what + ": obs_buf")
        task._cur = 1 - task._cur
    a = torch.as_tensor(np.random.default_rng(1).normal(size=(n, 75)).astype(np.float32), device=DEV)
    pd = target.actions(a)
    assert torch.equal(pd[:, :69], task._target_bufs[task._cur][:, 7:76] + a[:, :69]) and torch.equal(pd[:, 69:], a[:, 69:])


@gpu
def test_object_refuses_what_is_not_built():
    g = FX.golden()
    task, player, _ = stand_in(g, "P")
    task.pd_tar_lim = 0.5
    with pytest.raises(ValueError, match="pd_tar_lim"):
        mt.ImitationTarget(task, player, g["P/joint_pos_bind"], {"env": {"no_scale_action": True}})
    task.pd_tar_lim = np.pi / 2
    with pytest.raises(ValueError, match="pd_action_scale"):
        mt.ImitationTarget(task, player, g["P/joint_pos_bind"], {})
    with pytest.raises(NotImplementedError, match="dual_mode"):
        mt.ImitationTarget(task, player, g["P/joint_pos_bind"], {"v2p": {"dual_mode": "different"}, "env": {"no_scale_action": True}})
    with pytest.raises(NotImplementedError, match="obs_type"):
        mt.ImitationTarget(task, player, g["P/joint_pos_bind"], {"env": {"no_scale_action": True, "obs_type": "joint_pos"}})
    plain = mt.ImitationTarget(task, player, g["P/joint_pos_bind"], {"env": {"no_scale_action": True}})
    with pytest.raises(RuntimeError, match="add_residual_root"):
        plain.step(torch.zeros((task.num_envs, 3), device=DEV))


@gpu
def test_controller_runs_vid2players_control_step_on_a_racket_ball_batch():
    """64 envs, 6 substeps, synthetic clips shorter than the run, a seeded motion generator and the target attached, 16 control steps
    through pre_physics_step -> physics_step -> post_physics_step with the flagged envs reset.  After every step: the engine's PD target
    is the clamp of target_dof_pos + action, exactly; the previous target is the target written before the step, bit for bit; the new
    target is target_step_reference of the task's own tensors; the wrapped task's reset flag stays 0 past the clips' ends; freshly
    reset envs sit in the generator's pose with zero velocity; everything stays finite."""
    from tests import mvae_fixture as MF
    from tests import tennis_fixture as F
    from tests.gpu_util import synth_tables
    from vid2player3d_amd import ball_traj, mvae
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg
    from vid2player3d_amd.tasks import tennis_controller as tc

    n, steps = 64, 16
    torch.manual_seed(7)
    tg, g = F.golden(), FX.golden()
    gen = ball_traj.TennisBallGenerator({"num_samples": 500}, device=DEV, seed=3)
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=10, max_frames=14), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                  "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                  "reset_reaction_nframes": 6, "ball_traj_out_x_file": tg["traj_out_x"], "ball_traj_out_y_file": tg["traj_out_y"], "add_residual_dof": "euler",
                  "add_residual_root": True, "residual_root_scale": 0.02, "fix_head_orientation": True}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in tg["grids"]]

    ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": 300, "enableEarlyTermination": True}, "v2p": cfg["v2p"]}, params=SmallGrid)
    w, avg, std = MF.weights()
    # poses of the fixture (constructed, moderate) as the generator's start, as a feature: root, zero velocities, rot6d of the matrices
    rot = g["H/in/joint_rotmat"][0][np.arange(n) % 12]
    init = np.tile(avg, (n, 1)).astype(np.float32)
    init[:, 2] = 0.92
    init[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(n, 144)
    bind = g["H/joint_pos_bind"][0]
    player = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, n, w, avg, std, init, bind - bind[:1], True, DEV)
    with pytest.raises(NotImplementedError, match="add_residual_root"):
        ctl.attach_motion_generator(player)  # (as before: a residual root needs the target)
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)
    assert ctl.get_action_size() == 32 + 3 + 3
    st, seen, step_of_target = target.settings, {}, target.step

    def watched_step(residual_root=None):  # (the generator's matrices before the head rule writes Head and Neck back)
        seen.update(pose=N(player._joint_rotmat).copy(), residual=N(residual_root).copy())
        step_of_target(residual_root)

    target.step = watched_step
    task.reset()
    ctl.reset()
    torch.cuda.synchronize()

    def fresh_pose(ids):
        """freshly reset envs sit in the generator's pose (the previous target's) with zero velocity"""
        prev = mt.unpack_row(N(task._target_bufs[1 - task._cur])[ids])
        rb = N(task._rigid_body_state).reshape(n, 24, 13)[ids]
        assert np.array_equal(rb[..., 0:3].reshape(len(ids), 72), prev["rb_pos"]) and np.array_equal(rb[..., 3:7].reshape(len(ids), 96), prev["rb_rot"])
        assert not rb[..., 7:].any() and not N(task._dof_vel)[ids].any() and not N(task._humanoid_root_states)[ids, 7:].any()
        assert np.array_equal(N(task._dof_pos)[ids], prev["dof_pos"]) and np.array_equal(N(task._humanoid_root_states)[ids, 0:3], N(player._root_pos)[ids])

    fresh_pose(np.arange(n))
    rng = np.random.default_rng(2)
    sc = FX.scatter_of(g, "step")
    resets, seen_cur = 0, set()
    for k in range(steps):
        actions = torch.as_tensor(rng.normal(0, 0.5, (n, 38)).astype(np.float32), device=DEV)
        ll = torch.as_tensor(rng.normal(0, 0.3, (n, 75)).astype(np.float32), device=DEV)
        prev_row = N(task._target_bufs[1 - task._cur]).copy()
        ball, sim_root = N(task._ball_root_states)[:, 0:3].copy(), N(task._rigid_body_state).reshape(n, 24, 13)[:, 0, 0:3].copy()
        ctl.pre_physics_step(actions)
        torch.cuda.synchronize()
        # ---- the new target against the numpy statement of the task's own tensors (the generator's pose as the kernel found it)
        written = N(task._target_bufs[task._cur]).copy()
        res = N(actions)[:, 35:38] * np.float32(0.02)
        s = dict(root_pos=N(player._root_pos), joint_rotmat=seen["pose"], residual_root=res, ball_pos=ball, sim_root_pos=sim_root, joint_pos_bind=bind[None],
                 env_shape_id=None, prev_target=prev_row)
        assert np.array_equal(seen["residual"], res)
        want = mt.target_step_reference(st, s)
        FX.assert_row(written, want["target"], sc, "integration step %d" % k)
        FX.assert_close(N(player._joint_rotmat), want["joint_rotmat"], sc["joint_rotmat"], "integration step %d: joint_rotmat" % k)
        assert np.array_equal(N(task._target_bufs[1 - task._cur]), prev_row), "step %d: the previous target was written" % k
        assert not N(task.reset_buf).any() and np.isfinite(N(target.obs_buf)).all()
        dof_pos, tgt_dof = task._dof_pos.clone(), task._target_dof_pos.clone()
        ctl.physics_step(ll)
        ctl.post_physics_step()
        torch.cuda.synchronize()
        lim = np.float32(np.pi / 2)
        pd = torch.maximum(torch.minimum(tgt_dof + ll[:, :69], dof_pos + lim), dof_pos - lim)
        assert torch.equal(task._pd_target, pd), "step %d: the engine's PD target is not the clamp of target_dof_pos + action" % k
        assert np.array_equal(N(task._target_bufs[1 - task._cur]), written), "step %d: the previous target is not the target written before the step" % k
        assert not N(task.reset_buf).any(), "step %d: the wrapped task's own clocks ended an episode" % k
        for x in (task._rigid_body_state, task._dof_state, task._humanoid_root_states, task._pd_target, ctl.obs_buf, ctl.rew_buf, player._conditions, task._ball_root_states):
            assert torch.isfinite(x).all(), "step %d: a tensor is not finite" % k
        ids = ctl.reset_buf.nonzero(as_tuple=False).flatten()
        if k in (6, 9):  # (a partial id list in the middle of the run whatever the flags say, with `_cur` in either state)
            ids = torch.unique(torch.cat([ids, torch.as_tensor([1, 5, 40, n - 1], device=DEV)]))
            seen_cur.add(task._cur)
        ctl.reset(ids)
        torch.cuda.synchronize()
        if len(ids):
            fresh_pose(N(ids))
            resets += len(ids)
    assert resets >= 8 and seen_cur == {0, 1}, "the reset of a partial id list did not run with the target buffers in both states"
    assert float(task._cur_ref_motion_times.max()) <= 2 * task.dt and float(task._motion_lib._motion_lengths.max()) < steps * task.dt, "the clips are not shorter than the run"
