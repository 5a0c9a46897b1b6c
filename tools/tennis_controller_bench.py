"""What one control step of the tennis controller's task costs on the GPU (vid2player3d_amd/tasks/tennis_controller.py):

    kernel      TennisControllerTask.post_physics_step: one launch of v2p_tennis_task_step
    torch       the same step written in torch on device tensors the way the reference has it (physics_mvae_controller.py:441-452 with
                its two host synchronisations, + the roll of :365-366) - the transcription below; it lives here, not in the product
    physics     the racket + ball step (HumanoidSMPLIMRacketBall.step) alone, and followed by the controller step

8192 envs, L = 10, return_w_estimate, 6 substeps.  Every timing is taken with device events around `--iters` repetitions after `--warmup`
repetitions, three rounds each, alternating the candidates; one JSON line per figure and a summary line at the end.
    python tools/tennis_controller_bench.py [--envs 8192] [--iters 200] [--warmup 30]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vid2player3d_amd import ball_traj  # noqa: E402
from vid2player3d_amd.motion_lib import MotionLib  # noqa: E402
from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg, tennis_controller as tc  # noqa: E402

DEV = "cuda:0"


class MidGrid:  # the reference's ranges at ten times its velocity steps: tables of 16500 rows (the reference's have 8.25 million)
    VEL_X_RANGE = (10, 65, 1.0)
    VEL_Y_RANGE = (-5, 10, 1.0)
    VSPIN_RANGE = (-10, 10, 1.0)
    TRAJ_X_RANGE = (0, 30, 0.5)
    TRAJ_Y_RANGE = (0, 3, 0.1)


def quat_to_rotmat_wxyz(q):
    """konia_transform.quaternion_to_rotation_matrix (default order), op by op"""
    q = torch.nn.functional.normalize(q, p=2.0, dim=-1, eps=1e-12)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = torch.tensor(1.0, device=q.device)
    m = torch.stack((one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)), dim=-1)
    return m.view(q.shape[:-1] + (3, 3))


class TorchController:
    """post_physics_step of the reference on device tensors (the yardstick: what the step costs without the kernel).  State is its own."""

    def __init__(self, ctl, est):
        self.c, self.t, self.est, self.st = ctl, ctl.task, est, ctl.settings
        n, dev = ctl.num_envs, ctl.device
        z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=dev)
        self.tar_time, self.progress = ctl._tar_time.clone(), ctl.progress_buf.clone()
        self.ball_vel = ctl.task._ball_root_states[:, 7:10].clone()
        self.hit, self.hit_now = z(n, dtype=torch.bool), z(n, dtype=torch.bool)
        self.bounce_in, self.est_pos, self.est_time, self.est_in, self.est_peak = z(n, dtype=torch.bool), z(n, 3), z(n), z(n, dtype=torch.bool), z(n)
        self.obs, self.rew = z(n, ctl.num_obs), z(n)
        self.reset, self.terminate = z(n, dtype=torch.long), z(n, dtype=torch.long)
        self.distance = z(n)
        self.ball_traj, self.ball_obs = ctl._ball_traj.clone(), z(n, self.st["L"], 3)
        self.normal = torch.tensor(self.st["grip_normal"], device=dev)
        self.court_min, self.court_max = torch.tensor(self.st["court_min"], device=dev), torch.tensor(self.st["court_max"], device=dev)
        self.rb = ctl.task._rigid_body_state.view(n, 24, 13)

    def step(self):
        c, t, st = self.c, self.t, self.st
        n = c.num_envs
        self.ball_traj = self.ball_traj.roll(-1, dims=1)
        self.ball_traj[:, -1] = 0
        self.tar_time += 1
        self.progress += 1
        ball = t._ball_root_states
        # _update_state_from_sim (humanoid_smpl_im_mvae.py:799-849)
        now = ~self.hit & (ball[:, 8] > 0) & ((ball[:, 8] - self.ball_vel[:, 1]) > 10)
        self.hit_now = now
        self.hit |= now
        root_pos, root_vel = self.rb[:, 0, 0:3].clone(), t._humanoid_root_states[:, 7:10].clone()
        racket_pos = t._racket_rb_state[:, 0:3].clone()
        rot = quat_to_rotmat_wxyz(self.rb[:, 22, 3:7][..., [3, 0, 1, 2]])
        racket_normal = torch.matmul(rot, self.normal)
        ball_pos, self.ball_vel = ball[:, 0:3].clone(), ball[:, 7:10].clone()
        # _update_state (:271-314)
        upd = (c._tar_action == 0) & t._has_bounce_now
        bp = t._bounce_pos[upd]
        self.bounce_in[upd] = (bp[:, 0] > -4.11) & (bp[:, 0] < 4.11) & (bp[:, 1] > 0) & (bp[:, 1] < 11.89)
        if self.hit_now.sum() > 0:
            valid, pos, tm, peak = self.est.estimate(ball[self.hit_now])
            if valid.sum() > 0:
                ids = self.hit_now.nonzero(as_tuple=False).flatten()[valid]
                self.est_pos[ids, :2], self.est_time[ids], self.est_peak[ids] = pos, tm, peak
                self.est_in[ids] = (self.est_pos[ids, 0] > -4.11) & (self.est_pos[ids, 0] < 4.11) & (self.est_pos[ids, 1] > 0) & (self.est_pos[ids, 1] < 11.89)
        # compute_reward_return_w_estimate (:563-602)
        d = ball_pos - racket_pos
        pos_err = torch.sum(d * d, dim=-1)
        phase = c._phase_pred
        contact_phase = torch.where(c._swing_type_cycle >= 2, torch.ones_like(phase) * 3, torch.ones_like(phase) * math.pi)
        pd = phase - contact_phase
        pos_reward = ~self.hit * torch.exp(-st["scale_pos"] * pos_err) * torch.exp(-st["scale_phase"] * (pd * pd)) + self.hit * torch.ones_like(pos_err)
        err = torch.sum((self.est_pos - c._target_bounce_pos) ** 2, dim=-1)
        ball_reward = self.est_in * torch.exp(-st["scale_bounce_pos"] * err) * torch.exp(-st["scale_bounce_time"] * self.est_time)
        self.rew[:] = st["weight_pos"] * pos_reward + st["weight_ball_pos"] * ball_reward
        self.sub = torch.stack([pos_reward, ball_reward], dim=-1)
        # _compute_observations (:316-360)
        body_pos = torch.cat([self.rb[:, 1:, 0:3], racket_pos.unsqueeze(1)], 1)
        m = quat_to_rotmat_wxyz(self.rb[:, :, 3:7].reshape(-1, 4))
        rot6d = torch.cat([m[..., 0], m[..., 1]], dim=-1)
        actor = torch.cat([root_pos, root_vel, (body_pos - root_pos.unsqueeze(-2)).view(-1, 72), rot6d.view(-1, 144), racket_normal], dim=-1)
        if torch.isnan(actor).any():
            print("Found NAN in actor obersavations")
        self.ball_obs = self.ball_obs.roll(-1, dims=1)
        self.ball_obs[:, -1] = ball_pos.clone()
        task_obs = (self.ball_traj[:, :st["L"]] - racket_pos.unsqueeze(-2)).view(n, -1)
        if st["use_target"]:
            task_obs = torch.cat([task_obs, c._target_bounce_pos[:, :2] - root_pos[:, :2]], dim=-1)
        if torch.isnan(task_obs).any():
            print("Found NAN in task obersavations")
        self.obs[:] = torch.cat([actor, task_obs], dim=-1)
        # _compute_reset (:408-436)
        terminated = ((root_pos[:, 0] < self.court_min[0]).logical_or(root_pos[:, 1] < self.court_min[1]).logical_or(root_pos[:, 0] > self.court_max[0])
                      .logical_or(root_pos[:, 1] > self.court_max[1])).long()
        terminated |= torch.isnan(self.obs).any(dim=1)
        self.terminate[:] = terminated
        self.reset[:] = torch.where(self.progress >= st["max_episode_length"] - 1, torch.ones_like(self.reset), terminated)
        self.reaction = self.tar_time == c._tar_time_total
        self.recovery = (c._tar_action == 1) & (self.hit | (ball_pos[:, 1] < root_pos[:, 1] - 1))
        self.distance += root_vel[:, :2].norm(dim=-1)
        term = self.terminate.bool()
        if st["early_termination"]:
            term |= (self.recovery & ~self.hit) | (ball_pos[:, 1] < root_pos[:, 1] - 1)
            term |= self.hit & ~self.est_in
        self.terminate[term] = 1
        self.reset[term] = 1
        self.recovery[term] = 0
        self.reaction = self.reaction | self.reset.bool()


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tennis_controller_bench measures on a GPU; there is none here")
    from tests.gpu_util import synth_tables

    n = args.envs
    rng = np.random.default_rng(1)
    grids = tc.grids_of(MidGrid)
    rows = int(np.prod([ball_traj.grid_cells(g) for g in grids[:3]]))
    tx = rng.uniform(-1.5, 2.5, (rows, ball_traj.grid_cells(grids[3]))).astype(np.float32)
    ty = np.stack([rng.uniform(0, 25, (rows, ball_traj.grid_cells(grids[4]))), rng.uniform(0, 2, (rows, ball_traj.grid_cells(grids[4])))], -1).astype(np.float32)
    gen = ball_traj.TennisBallGenerator({"num_samples": 10000}, device=DEV, seed=3)
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=16, min_frames=60, max_frames=200), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                  "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                  "reset_reaction_nframes": 30, "ball_traj_out_x_file": tx, "ball_traj_out_y_file": ty}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
    ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": 300, "enableEarlyTermination": False}, "v2p": cfg["v2p"]}, params=MidGrid)
    est = ball_traj.TennisBallOutEstimator(tx, ty, device=DEV, params=MidGrid)
    task.reset()
    ctl.reset()
    act = torch.zeros((n, 75), device=DEV)
    phase = torch.as_tensor(rng.uniform(2, 4, n).astype(np.float32), device=DEV)
    swing = torch.as_tensor(rng.integers(-1, 4, n), device=DEV)
    for _ in range(5):  # a few steps of flight, so that the state is one of a rollout
        task.step(act.clone())
        ctl.post_physics_step(phase, swing, swing)
    ref = TorchController(ctl, est)

    def kernel_step():
        ctl.post_physics_step(phase, swing, swing)

    def physics_step():
        task.step(act)

    def both():
        task.step(act)
        ctl.post_physics_step(phase, swing, swing)

    figures = {"kernel_ms": kernel_step, "torch_ms": ref.step, "physics_ms": physics_step, "physics_plus_controller_ms": both}
    res = {k: [] for k in figures}
    for r in range(args.rounds):
        for k, fn in figures.items():
            ms = timed(fn, args.iters, args.warmup)
            res[k].append(ms)
            print(json.dumps({"figure": k, "round": r, "ms_per_step": round(ms, 5), "envs": n, "iters": args.iters}), flush=True)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({"summary": "tennis controller step, %d envs, L = 10, return_w_estimate, 6 substeps" % n, **{k: round(v, 5) for k, v in med.items()},
                      "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in res.items()}, "torch_over_kernel": round(med["torch_ms"] / med["kernel_ms"], 2),
                      "controller_share_of_physics": round(med["kernel_ms"] / med["physics_ms"], 4), "torch_share_of_physics": round(med["torch_ms"] / med["physics_ms"], 4),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
