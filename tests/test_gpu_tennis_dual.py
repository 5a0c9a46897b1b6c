"""The two-player rally on the device: `v2p_tennis_dual_step` and `v2p_tennis_dual_handover` on what the reference itself computed
(tests/golden/tennis_dual.npz) and on their numpy statements, at one pair, a full workgroup, a half-filled last workgroup and many
workgroups with a partial one; the single-player step beside them; and `DualTennisControllerTask` on a racket + ball batch."""
import numpy as np
import pytest
import torch

from tests import tennis_dual_fixture as F
from vid2player3d_amd.tasks import tennis_controller as tc
from vid2player3d_amd.tasks import tennis_controller_dual as td

gpu = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (2, 4, 6, 66)
DTYPES = {"wrist_link": torch.int64, "swing_type": torch.int64, "swing_type_cycle": torch.int64, "tar_time_total": torch.int64, "tar_action": torch.int64,
          "tar_time": torch.int64, "progress": torch.int64, "traj_cursor": torch.int32, "vel_x_overflow": torch.int64, "reset": torch.int64, "terminate": torch.int64,
          "num_reset_reaction": torch.int64}
BYTES = ("has_bounce", "has_bounce_now", "has_racket_contact", "has_racket_contact_now", "bounce_in", "est_bounce_in", "reset_reaction", "reset_recovery")
STEP_WRITES = {"has_racket_contact", "has_racket_contact_now", "tar_time", "progress", "prev_ball_vy", "traj_cursor", "ball_obs", "bounce_in", "distance", "racket_pos",
               "racket_normal", "obs", "rew", "sub_rewards", "reset", "reset_reaction", "reset_recovery"}


def upload(s, **more):
    t = {}
    for k, v in dict(s, **more).items():
        if v is None:
            continue
        dt = torch.uint8 if k in BYTES else DTYPES.get(k, torch.float32)
        t[k] = torch.as_tensor(np.ascontiguousarray(v).astype(np.uint8 if k in BYTES else v.dtype)).to(device=DEV, dtype=dt).contiguous()
    return t


def download(t):
    return {k: v.detach().cpu().numpy() for k, v in t.items()}


def step_tensors(st, s):
    """The step's inputs plus poisoned outputs (NaN / 7: whatever survives was not written); `reset` keeps the fixture's value."""
    n = len(s["rb_state"])
    nan = lambda *shape: np.full(shape, np.nan, np.float32)
    return upload(s, racket_pos=nan(n, 3), racket_normal=nan(n, 3), obs=np.full((n, tc.obs_width(st)), np.inf, np.float32), rew=nan(n),
                  sub_rewards=nan(n, tc.num_sub_rewards(st)), reset_reaction=np.full(n, 7, np.uint8), reset_recovery=np.full(n, 7, np.uint8))


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", F.VARIANTS)
def test_dual_step_kernel_matches_the_reference(name, n):
    st, s = F.settings(name), F.inputs("step", name, n)
    dev = step_tensors(st, s)
    before = download(dev)
    names = td.launch_dual_step(st, dev, n)
    torch.cuda.synchronize()
    got = download(dev)
    F.compare(got, F.expected("step", name, n), F.scatter("step"), "step %s n=%d" % (name, n))
    want = td.dual_step_reference(st, s)
    assert names == want.pop("sub_rewards_names")
    F.compare(got, {k: np.asarray(v) for k, v in want.items()}, F.scatter("step"), "step %s n=%d against the statement" % (name, n))
    for k in before:  # what the dual step only reads - the out-estimator's values among it - keeps its bits
        if k not in STEP_WRITES or (k.startswith("has_racket_contact") and not st["contact_by_velocity"]) or (k == "traj_cursor" and st["use_history"]):
            assert np.array_equal(before[k], got[k], equal_nan=True), "step %s n=%d: the kernel wrote %s" % (name, n, k)


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", F.VARIANTS)
def test_handover_kernel_matches_the_reference(name, n):
    st, s = F.settings(name), F.inputs("hand", name, n)
    dev = upload(s)
    before = download(dev)
    td.launch_handover(st, dev, n)
    torch.cuda.synchronize()
    got = download(dev)
    want = F.expected("hand", name, n)
    F.compare(got, want, F.scatter("hand"), "hand-over %s n=%d" % (name, n))
    stated = td.handover_reference(st, s)
    stated.pop("table_rows")
    F.compare(got, {k: np.asarray(v) for k, v in stated.items()}, F.scatter("hand"), "hand-over %s n=%d against the statement" % (name, n))
    # rows of envs whose pair has no flag match bit for bit, in every tensor; so does every tensor the launch only reads
    rea, rec = s["reset_reaction"].reshape(-1, 2), s["reset_recovery"].reshape(-1, 2)
    untouched = np.repeat(~(rea.any(1) | rec.any(1)), 2)
    for k, v in before.items():
        if len(v) == n:
            assert np.array_equal(v[untouched], got[k][untouched], equal_nan=True), "hand-over %s n=%d: a pair without a flag changed its %s" % (name, n, k)
        if k not in want:
            assert np.array_equal(v, got[k], equal_nan=True), "hand-over %s n=%d: the kernel wrote %s" % (name, n, k)
    assert np.array_equal(got["reset_reaction"], before["reset_reaction"]) and np.array_equal(got["reset_recovery"], before["reset_recovery"])


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_single_player_step_on_the_same_buffers_is_what_it_was(n):
    """`v2p_tennis_task_step` on the dual fixture's buffers still is its numpy statement: flags and integers exact, floats within the
    step's scatter.  That it gives the same BITS as before the third instantiation stood beside it does not rest on this test but on
    tools/kernel_identity.py: instantiations <1,0> and <0,0> are the parent's machine code, instruction for instruction and descriptor
    for descriptor (profiles/r26a_kernel_identity_tennis.txt)."""
    from tests import tennis_fixture as SF

    st, s = F.settings("A"), F.inputs("step", "A", n)
    g = SF.golden()
    st = dict(st, grids=g["grids"], court_min=(-5.0, -16.0), court_max=(5.0, -1.0), early_termination=True, max_episode_length=300)
    s.update(traj_out_x=g["traj_out_x"], traj_out_y=g["traj_out_y"], tar_time_total=np.full(n, 20, np.int64), vel_x_overflow=np.zeros(1, np.int64))
    from vid2player3d_amd import _lib

    dev = {k: v for k, v in step_tensors(st, s).items() if k in _lib.TENNIS_BUFFER_NAMES}
    dev["terminate"] = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    tc.launch_step(st, dev, n)
    torch.cuda.synchronize()
    got = download(dev)
    want = tc.task_step_reference(st, s)
    want.pop("sub_rewards_names")
    want["vel_x_overflow"] = np.asarray(want["vel_x_overflow"]).reshape(1)
    sc = dict(F.scatter("step"), est_bounce_pos=1e-6, est_bounce_time=1e-6, est_max_height=1e-6)
    F.compare(got, {k: np.asarray(v) for k, v in want.items()}, sc, "single step n=%d" % n)


@gpu
def test_dual_controller_on_a_racket_ball_batch():
    """8 envs, 6 substeps, `dual_mode: True` with a seeded motion generator and the imitation target.  A forced hit (the velocity rule's
    inputs) makes the hitter recover and its opponent react; after `post_physics_step()` and `reset([])` the pair's `_ball_root_states`
    are the statement's; one more `task.step` moves the receiver's ball off the mirrored in-state along its new velocity - the engine
    reads the kernel's write.  A pair that terminates resets through `reset(ids)` into the generator's pose with the serve state at the
    server's racket head."""
    from tests import mvae_fixture as MF
    from tests import mvae_target_fixture as FX
    from tests.gpu_util import N, synth_tables
    from vid2player3d_amd import mvae
    from vid2player3d_amd import mvae_target as mt
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    n = 8
    torch.manual_seed(11)
    d, g = F.golden(), FX.golden()
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = {"dual_mode": True, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                  "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                  "use_random_ball_target": True, "reset_reaction_nframes": 6, "ball_traj_in_file": d["traj_in"], "add_residual_dof": "euler", "serve_from": "near"}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class InGrid:
        HEIGHT_RANGE, VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE = [tuple(r) for r in d["in_grids"]]

    ctl = td.DualTennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"]}, traj_in_params=InGrid)
    assert ctl.settings["contact_by_velocity"] and not N(ctl._reset_reaction_buf).any() and not N(ctl._reset_recovery_buf).any()
    w, avg, std = MF.weights()
    rot = g["H/in/joint_rotmat"][0][np.arange(2) % 12]
    frames = np.tile(avg, (2, 1)).astype(np.float32)
    frames[:, 2] = 0.92
    frames[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(2, 144)
    bind = g["H/joint_pos_bind"][0]
    player = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler", "dual_mode": True}, n, w, avg, std, frames[:1], bind - bind[:1],
                                  True, DEV, init_data_ready=frames[:1], init_data_serve=frames[1:])
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)
    task.reset()
    # ---- the first reset of all pairs: odd envs serve ('near': the even envs react)
    draws = np.random.default_rng(3).uniform(0, 1, (n // 2, 3)).astype(np.float32)
    ctl.reset(None, serve_vel_draws=draws)
    torch.cuda.synchronize()
    servers, receivers = np.arange(1, n, 2), np.arange(0, n, 2)
    ball = N(task._ball_root_states)
    head = N(player._racket_pos)
    assert np.array_equal(ball[servers, 0:2], head[servers, 0:2]), "the serve starts at the server's racket head"
    assert np.allclose(ball[servers, 2], np.clip(np.round((head[servers, 2] - 0.5) / 0.5), 0, 2) * 0.5 + 0.5, atol=1e-6), "... at the height of its grid cell"
    serve_vel = draws * np.array([4, 4, 3], np.float32) + np.array([-2, 28, 5], np.float32)
    assert np.allclose(np.hypot(ball[servers, 7], ball[servers, 8]), np.clip(np.round((np.hypot(serve_vel[:, 0], serve_vel[:, 1]) - 20) / 2), 0, 3) * 2 + 20, atol=1e-4)
    assert np.array_equal(ball[receivers, 0:2], -ball[servers, 0:2]) and np.array_equal(ball[receivers, 7:9], -ball[servers, 7:9])
    assert (N(ctl._tar_action)[receivers] == 1).all() and (N(ctl._tar_action)[servers] == 0).all() and (N(ctl._ball_traj_cursor)[receivers] == 0).all()
    assert np.array_equal(N(task._humanoid_root_states)[:, 0:3], N(player._root_pos)), "the pairs stand in the generator's pose"
    assert np.allclose(N(player._conditions)[receivers, 0, 3:], ((frames[0] - avg) / std)[None, 3:], atol=1e-5), "the receivers start from the ready frame"
    assert np.allclose(N(player._conditions)[servers, 0, 3:], ((frames[1] - avg) / std)[None, 3:], atol=1e-5), "the servers start from the serve frame"
    assert np.abs(frames[0] - frames[1]).max() > 0.1
    assert np.isfinite(N(ctl.obs_buf)[receivers]).all() and ctl.reset(None) is None

    # ---- a rally step: env 1 hits (velocity rule), env 0 is in recovery
    act = torch.zeros((n, 75), device=DEV)
    task.step(act.clone())
    hitter = torch.tensor([1.0, -11.0, 1.1, 0, 0, 0, 1, 1.5, 22.5, 5.8, 20.0, -25.0, 6.0], device=DEV)
    task._ball_root_states[1] = hitter
    ctl._prev_ball_vy[1] = -20.0
    ctl._tar_action[:] = torch.tensor([0, 1] * (n // 2), device=DEV)
    task._has_bounce[:] = False
    task._has_racket_ball_contact[:] = False
    rng = np.random.default_rng(5)
    phase, swing = torch.as_tensor(rng.uniform(2, 4, n).astype(np.float32), device=DEV), torch.as_tensor(rng.integers(-1, 4, n), device=DEV)
    ctl._phase_pred.copy_(phase); ctl._swing_type.copy_(swing); ctl._swing_type_cycle.copy_(swing)  # (what the step copies in: the statement reads it)
    before = ctl.state_arrays()
    ctl.post_physics_step(phase, swing, swing)
    torch.cuda.synchronize()
    got = ctl.state_arrays()
    want = td.dual_step_reference(ctl.settings, before)
    want.pop("sub_rewards_names")
    F.compare(got, {k: np.asarray(v) for k, v in want.items()}, F.scatter("step"), "integration step")
    assert got["has_racket_contact_now"][1] and got["reset_recovery"][1] and got["reset_reaction"][0] and not got["reset_reaction"][1] and not got["reset"][0:2].any()
    # ---- the hand-over
    before = ctl.state_arrays()
    ctl.reset([])
    torch.cuda.synchronize()
    got = ctl.state_arrays()
    before["target_draw"] = got["target_draw"]  # (drawn by `reset` before its launch)
    want = td.handover_reference(ctl.settings, before)
    want.pop("table_rows")
    F.compare(got, {k: np.asarray(v) for k, v in want.items()}, F.scatter("hand"), "integration hand-over")
    assert np.array_equal(got["ball_state"][0, 0:2], -N(hitter)[0:2]) and np.array_equal(got["ball_state"][1, 0:2], N(hitter)[0:2])
    assert got["tar_action"][0] == 1 and got["tar_action"][1] == 0 and got["traj_cursor"][0] == 0
    # ---- the engine flies the receiver's ball from the kernel's write
    start = got["ball_state"][0].copy()
    task.step(act.clone())
    torch.cuda.synchronize()
    moved = N(task._ball_root_states)[0, 0:3] - start[0:3]
    assert np.abs(moved - start[7:10] / 30.0).max() < 0.1 and np.dot(moved, start[7:10]) > 0.5 * np.dot(start[7:10], start[7:10]) / 30.0
    # ---- a miss ends the episode of the pair, and `reset(ids)` serves again
    ctl._tar_action[2:4] = torch.tensor([1, 0], device=DEV)
    task._ball_root_states[2, 1] = task._humanoid_root_states[2, 1] - 3.0
    ctl.post_physics_step(phase, swing, swing)
    torch.cuda.synchronize()
    assert N(ctl.reset_buf)[2:4].all() and not N(ctl._reset_reaction_buf)[2:4].any() and not N(ctl._reset_recovery_buf)[2:4].any()
    ids = ctl.reset_buf.nonzero(as_tuple=False).flatten()
    ctl.reset(ids)
    torch.cuda.synchronize()
    assert not N(ctl.reset_buf)[2:4].any() and (N(ctl.progress_buf)[2:4] == 0).all()
    ball = N(task._ball_root_states)
    assert np.array_equal(ball[3, 0:2], N(player._racket_pos)[3, 0:2]) and np.array_equal(ball[2, 0:2], -ball[3, 0:2])
    assert np.array_equal(N(task._humanoid_root_states)[2:4, 0:3], N(player._root_pos)[2:4]) and np.isfinite(N(ctl.obs_buf)).all()


@gpu
def test_dual_controller_over_a_two_player_task_with_a_grip_per_player():
    """`dual_mode: 'different'` as the shipped two-player configs have it - two players, `grip` a list of two names - over a two-player
    racket + ball task of 4 envs: the task object is built, one `post_physics_step` and one `reset([])` follow the statements, and
    the racket normal is the wrist's rotation times the grip of the env's parity."""
    from tests.gpu_util import N, synth_tables
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    n = 4
    torch.manual_seed(17)
    d = F.golden()
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = {"dual_mode": "different", "player": ["nadal", "federer"], "righthand": [False, True], "grip": ["semi_western", "eastern"], "restitution": 1.4,
                  "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate", "reward_weights": {"pos": 0.5, "ball_pos": 0.5},
                  "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10, "reset_reaction_nframes": 6, "ball_traj_in_file": d["traj_in"]}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
    assert task.racket_players == ["nadal", "federer"]

    class InGrid:
        HEIGHT_RANGE, VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE = [tuple(r) for r in d["in_grids"]]

    ctl = td.DualTennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"]}, traj_in_params=InGrid)
    assert ctl.settings["grip_normals"] == (tuple(tc.GRIP_NORMALS["semi_western"]), tuple(tc.GRIP_NORMALS["eastern"]))
    assert ctl.settings["grip_normal"] == tuple(tc.GRIP_NORMALS["semi_western"])
    wrist = N(ctl._wrist_link)
    assert wrist[0] != wrist[1] and np.array_equal(wrist[0::2], wrist[0:1].repeat(n // 2)), "a left-handed and a right-handed player: two wrist links"
    with pytest.raises(ValueError, match="list of two names"):
        td.DualTennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": dict(cfg["v2p"], grip="eastern")}, traj_in_params=InGrid)
    task.reset()
    task.step(torch.zeros((n, 75), device=DEV))
    # env 1 hits (the velocity rule's inputs), env 0 is in recovery
    task._ball_root_states[1] = torch.tensor([1.0, -11.0, 1.1, 0, 0, 0, 1, 1.5, 22.5, 5.8, 20.0, -25.0, 6.0], device=DEV)
    ctl._prev_ball_vy[1] = -20.0
    ctl._tar_action[:] = torch.tensor([0, 1] * (n // 2), device=DEV)
    task._has_bounce[:] = False
    task._has_racket_ball_contact[:] = False
    ctl.reset_buf[:] = 0
    rng = np.random.default_rng(7)
    phase, swing = torch.as_tensor(rng.uniform(2, 4, n).astype(np.float32), device=DEV), torch.as_tensor(rng.integers(-1, 4, n), device=DEV)
    ctl._phase_pred.copy_(phase); ctl._swing_type.copy_(swing); ctl._swing_type_cycle.copy_(swing)  # (what the step copies in: the statement reads it)
    before = ctl.state_arrays()
    ctl.post_physics_step(phase, swing, swing)
    torch.cuda.synchronize()
    got = ctl.state_arrays()
    want = td.dual_step_reference(ctl.settings, before)
    want.pop("sub_rewards_names")
    F.compare(got, {k: np.asarray(v) for k, v in want.items()}, F.scatter("step"), "two-player step")
    assert got["reset_recovery"][1] and got["reset_reaction"][0]
    # ---- the racket normal by parity: each side's own grip, and not the other's
    for side, (mine, other) in enumerate((("semi_western", "eastern"), ("eastern", "semi_western"))):
        rows = np.arange(side, n, 2)
        own = tc.observation_reference(dict(ctl.settings, grip_normal=tc.GRIP_NORMALS[mine]), before, rows)[3]
        wrong = tc.observation_reference(dict(ctl.settings, grip_normal=tc.GRIP_NORMALS[other]), before, rows)[3]
        assert np.abs(got["racket_normal"][rows] - own).max() <= 8 * F.scatter("step")["racket_normal"], "side %d has its own grip" % side
        assert np.abs(got["racket_normal"][rows] - wrong).max() > 0.1, "side %d does not have its opponent's grip" % side
        assert np.array_equal(got["obs"][rows, 222:225], got["racket_normal"][rows])
    # ---- the hand-over
    before = ctl.state_arrays()
    ctl.reset([])
    torch.cuda.synchronize()
    got = ctl.state_arrays()
    want = td.handover_reference(ctl.settings, before)
    want.pop("table_rows")
    F.compare(got, {k: np.asarray(v) for k, v in want.items()}, F.scatter("hand"), "two-player hand-over")
    assert got["tar_action"][0] == 1 and got["tar_action"][1] == 0 and np.array_equal(got["ball_state"][0, 0:2], -before["ball_state"][1, 0:2])
    assert np.array_equal(got["racket_normal"][0], before["racket_normal"][0]), "the receiver's observation keeps its side's grip"
