"""The tennis controller's task step on the device: `v2p_tennis_task_step` / `v2p_tennis_task_obs` on what the reference itself computed
(tests/golden/tennis_controller.npz), step by step, and `TennisControllerTask` on a racket + ball batch against `task_step_reference`."""
import numpy as np
import pytest
import torch

from tests import tennis_fixture as F
from vid2player3d_amd.tasks import tennis_controller as tc

gpu = pytest.mark.gpu
DEV = "cuda:0"
WRITTEN = {"has_racket_contact", "has_racket_contact_now", "tar_time", "progress", "prev_ball_vy", "traj_cursor", "ball_obs", "bounce_in", "est_bounce_pos", "est_bounce_time",
           "est_max_height", "est_bounce_in", "distance", "vel_x_overflow", "racket_pos", "racket_normal", "obs", "rew", "sub_rewards", "reset", "terminate", "reset_reaction",
           "reset_recovery"}
DTYPES = {"wrist_link": torch.int64, "swing_type": torch.int64, "swing_type_cycle": torch.int64, "tar_time_total": torch.int64, "tar_action": torch.int64,
          "tar_time": torch.int64, "progress": torch.int64, "traj_cursor": torch.int32, "vel_x_overflow": torch.int64, "reset": torch.int64, "terminate": torch.int64}
BYTES = ("has_bounce", "has_bounce_now", "has_racket_contact", "has_racket_contact_now", "bounce_in", "est_bounce_in", "reset_reaction", "reset_recovery")


def upload(st, s):
    """The arrays of a fixture step as device tensors, plus poisoned outputs (NaN / -7: whatever survives was not written)."""
    n = len(s["rb_state"])
    t = {}
    for k, v in s.items():
        if v is None:
            continue
        dt = torch.uint8 if k in BYTES else DTYPES.get(k, torch.float32)
        t[k] = torch.as_tensor(np.ascontiguousarray(v).astype(np.uint8 if k in BYTES else v.dtype)).to(device=DEV, dtype=dt).contiguous()
    f = dict(dtype=torch.float32, device=DEV)
    t.update(racket_pos=torch.full((n, 3), float("nan"), **f), racket_normal=torch.full((n, 3), float("nan"), **f), obs=torch.full((n, tc.obs_width(st)), float("inf"), **f),
             rew=torch.full((n,), float("nan"), **f), sub_rewards=torch.full((n, tc.num_sub_rewards(st)), float("nan"), **f))
    for k in ("reset", "terminate"):
        t[k] = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    for k in ("reset_reaction", "reset_recovery"):
        t[k] = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    return t


def download(t):
    return {k: v.detach().cpu().numpy() for k, v in t.items()}


@gpu
@pytest.mark.parametrize("name", F.VARIANTS)
def test_task_step_kernel_matches_the_reference_step_by_step(name):
    st, steps = F.settings(name)
    for t in range(steps):
        s = F.step_inputs(name, t)
        dev = upload(st, s)
        before = download(dev)
        names = tc.launch_step(st, dev, len(s["rb_state"]))
        torch.cuda.synchronize()
        got = download(dev)
        want = F.step_expected(name, t)
        F.compare(got, want, "%s step %d" % (name, t))
        assert names == F.golden()[name + "/sub_rewards_names"].tobytes().decode()
        assert int(got["vel_x_overflow"][0]) == int(want["vel_x_overflow"])
        for k in before:  # tensors the step only reads (without the velocity rule: the racket task's flags too) are unchanged
            if k not in WRITTEN or (k.startswith("has_racket_contact") and not st["contact_by_velocity"]):
                assert np.array_equal(before[k], got[k], equal_nan=True), "%s step %d: the kernel wrote %s" % (name, t, k)
        assert np.array_equal(got["est_bounce_pos"][:, 2], before["est_bounce_pos"][:, 2])


@gpu
@pytest.mark.parametrize("name", F.VARIANTS)
def test_obs_kernel_matches_the_reference_at_reset_time(name):
    st, steps = F.settings(name)
    cases = 0
    for t in range(steps - 1):
        s, ids, want = F.reset_obs_case(name, t)
        if len(ids) == 0:
            continue
        dev = upload(st, s)
        before = download(dev)
        # (an id outside the batch is skipped, not followed)
        tc.launch_obs(st, dev, len(s["rb_state"]), torch.as_tensor(np.concatenate([ids, [len(s["rb_state"]), -1]]), device=DEV))
        torch.cuda.synchronize()
        got = download(dev)
        rows = {k: got[k][ids] for k in want}
        F.compare(rows, want, "%s reset after step %d" % (name, t))
        others = np.setdiff1d(np.arange(len(s["rb_state"])), ids)
        for k in before:
            if k in ("obs", "racket_pos", "racket_normal", "ball_obs"):
                assert np.array_equal(before[k][others], got[k][others], equal_nan=True), "%s: rows of other envs written in %s" % (name, k)
            else:
                assert np.array_equal(before[k], got[k], equal_nan=True), "%s: the observation call wrote %s" % (name, k)
        cases += 1
    assert cases >= 2


@gpu
def test_controller_on_a_racket_ball_batch_follows_the_reference_step():
    """64 envs, 6 substeps (the racket hit comes from the velocity rule), balls from a generated pool, 12 steps with zero actions: after
    every step the task's outputs equal task_step_reference applied to its own tensors; every env gets a reaction reset, which puts the
    new launch position into frame 0 of its window; the observation is finite."""
    from tests.gpu_util import N, synth_tables
    from vid2player3d_amd import ball_traj
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    n, steps = 64, 12
    torch.manual_seed(5)
    gen = ball_traj.TennisBallGenerator({"num_samples": 1000}, device=DEV, seed=3)
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    rng = np.random.default_rng(9)
    g = F.golden()
    cfg["v2p"] = {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                  "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                  "use_random_ball_target": True, "reset_reaction_nframes": 6, "ball_traj_out_x_file": g["traj_out_x"], "ball_traj_out_y_file": g["traj_out_y"]}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in g["grids"]]

    ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": 300, "enableEarlyTermination": True}, "v2p": cfg["v2p"]}, params=SmallGrid)
    assert ctl.settings["contact_by_velocity"] and ctl.obs_buf.shape == (n, 225 + 30 + 2) == (n, ctl.get_actor_obs_size() + ctl.get_task_obs_size())
    task.reset()
    ctl.reset()
    assert np.array_equal(N(ctl.ball_traj_window())[:, 0], N(task._ball_root_states)[:, 0:3]) and np.isfinite(N(ctl.obs_buf)).all()
    reaction_resets = np.zeros(n, np.int64)
    act = torch.zeros((n, 75), device=DEV)
    for k in range(steps):
        task.step(act.clone())
        phase = torch.as_tensor(rng.uniform(2, 4, n).astype(np.float32), device=DEV)
        swing = torch.as_tensor(rng.integers(-1, 4, n), device=DEV)
        cycle = torch.as_tensor(rng.integers(-1, 4, n), device=DEV)
        ctl._phase_pred.copy_(phase); ctl._swing_type.copy_(swing); ctl._swing_type_cycle.copy_(cycle)
        before = ctl.state_arrays()
        ctl.post_physics_step(phase, swing, cycle)
        torch.cuda.synchronize()
        got = ctl.state_arrays()
        want = tc.task_step_reference(ctl.settings, before)
        names = want.pop("sub_rewards_names")
        F.compare(got, want, "integration step %d" % k)
        assert ctl.extras["sub_rewards_names"] == names and ctl.extras["terminate"] is ctl._terminate_buf
        assert np.isfinite(got["obs"]).all()
        due = N(ctl._reset_reaction_buf).astype(bool)
        reaction_resets += due
        ctl.reset(ctl.reset_buf.nonzero(as_tuple=False).flatten())
        ids = np.nonzero(due)[0]
        assert np.array_equal(N(ctl.ball_traj_window())[ids, 0], N(task._ball_root_states)[ids, 0:3]), "frame 0 of a fresh window is the launch position"
        assert (N(ctl._ball_traj_cursor)[ids] == 0).all() and (N(ctl._tar_time)[ids] == 0).all() and (N(ctl._tar_action)[ids] == 1).all()
        assert np.isfinite(N(ctl.obs_buf)).all()
    assert (reaction_resets >= 1).all(), "every env has had a reaction reset"
