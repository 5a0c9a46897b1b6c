"""What the imitation target of a control step costs on the GPU (vid2player3d_amd/mvae_target.py):

    target          ImitationTarget.step: one launch of v2p_mvae_target_step (head rule, forward kinematics, conversions, velocities, the
                    packed row)
    target_obs      the same followed by compute_observations (v2p_obs_imitation, the [N,734] observation): `post_mvae_step`
    torch           `_set_target_motion_state` written in torch on device tensors in the reference's form - `_smpl_to_sim` twice with
                    the chain of 24 4x4 `matmul`s, the four-branch `where`s, the gathers (humanoid_smpl_im_mvae.py:600-661, 897-946) - the
                    transcription below; it lives here, not in the product.  (The observation is not transcribed: `torch` stands against
                    `target`.)
    launch          a one-env launch of v2p_mvae_target_actions, back to back: what a launch costs here
    pair            the 6-substep racket + ball step after the generator's step, and the same with the target in between
                    (target, observation, PD-target actions): what the target adds to vid2player's control step

target, target_obs and torch at 1024 and at 8192 envs, the pair at 8192; head rule on, a residual root.  Every timing is taken with
device events around `--iters` repetitions after `--warmup` repetitions, three rounds each, alternating the candidates; one JSON line per
figure and a summary line at the end, which also states the bytes the step moves per env and their time at the measured HBM rate.
    python tools/mvae_target_bench.py [--envs 8192] [--iters 200] [--warmup 20]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from mvae_bench import DEV, angle_axis_to_rotmat, make_pair, quat_to_angle_axis_konia, rotmat_to_quat, timed  # noqa: E402

from vid2player3d_amd import mvae_target as mt  # noqa: E402

HBM_TB_S = 6.29                     # float4 copy measured on this part
READ_BYTES = 4 * (3 + 216 + 3 + 3 + 3 + 72 + 3 + 96)  # root, matrices, residual, ball, simulated root, bind row, previous root and rb_rot
WRITE_BYTES = 4 * (331 + 18) + 20   # the row, Head and Neck, the three held clocks


def quat_to_rotmat(q):
    """konia_transform.quaternion_to_rotation_matrix of (w, x, y, z)"""
    q = torch.nn.functional.normalize(q, p=2.0, dim=-1, eps=1e-12)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = torch.tensor(1.0, device=q.device)
    return torch.stack((one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)), dim=-1).view(q.shape[:-1] + (3, 3))


def quat_mul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    ww, yy, zz = (z1 + x1) * (x2 + y2), (w1 - y1) * (w2 + z2), (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2), qq - zz + (z1 + y1) * (w2 - x2), qq - ww + (z1 - y1) * (y2 - z2)], dim=-1)


def quat_diff_angle_axis(prev, cur):
    """quat_mul_norm(quat_inverse(prev), cur) -> quat_to_angle_axis (utils/torch_utils.py:14-103)"""
    q = quat_mul(torch.cat([-prev[..., :3], prev[..., 3:]], dim=-1), cur)
    q = (1 - 2 * (q[..., 3:] < 0).float()) * q
    q = q / q.norm(p=2, dim=-1).clamp(min=1e-9).unsqueeze(-1)
    sin_theta = torch.sqrt(1 - q[..., 3] * q[..., 3])
    angle = 2 * torch.acos(q[..., 3])
    angle = torch.atan2(torch.sin(angle), torch.cos(angle))
    axis = q[..., 0:3] / sin_theta.unsqueeze(-1)
    mask = torch.abs(sin_theta) > 1e-5
    default_axis = torch.zeros_like(axis)
    default_axis[..., -1] = 1
    return torch.where(mask, angle, torch.zeros_like(angle)), torch.where(mask.unsqueeze(-1), axis, default_axis)


class TorchTarget:
    """`_set_target_motion_state` of the reference on device tensors (the yardstick: what the step costs without the kernel)."""

    def __init__(self, st, bind, n):
        self.st, self.n = st, n
        self.bind = bind.unsqueeze(0).repeat(n, 1, 1)
        self.parents = torch.tensor(st["smpl_parents"], device=DEV)
        self.order = st["smpl_of_body"]

    def chain(self, rot_mats):
        F = torch.nn.functional
        joints = self.bind.unsqueeze(-1)
        rel = joints.clone()
        rel[:, 1:] -= joints[:, self.parents[1:]].clone()
        tm = torch.cat([F.pad(rot_mats.reshape(-1, 3, 3), [0, 0, 0, 1]), F.pad(rel.reshape(-1, 3, 1), [0, 0, 0, 1], value=1.0)], dim=2).reshape(-1, 24, 4, 4)
        chain = [tm[:, 0]]
        for i in range(1, 24):
            chain.append(torch.matmul(chain[self.st["smpl_parents"][i]], tm[:, i]))
        transforms = torch.stack(chain, dim=1)
        return transforms[:, :, :3, 3], transforms[:, :, :3, :3]

    def smpl_to_sim(self, root_pos, rotmat, prev_root_pos=None, prev_rb_rot=None):
        dt = self.st["control_dt"]
        dof_pos = quat_to_angle_axis_konia(rotmat_to_quat(rotmat))[:, self.order, :][:, 1:, :].reshape(-1, 69)
        posed, grot = self.chain(rotmat)
        rb_rot = rotmat_to_quat(grot.contiguous())[..., [1, 2, 3, 0]][:, self.order, :]
        rb_pos = posed[:, self.order, :] - (self.bind[:, :1] - root_pos.unsqueeze(1))
        if prev_root_pos is None:
            return root_pos, rb_rot[:, 0], dof_pos, None, None, None, rb_pos, rb_rot
        root_vel = (root_pos - prev_root_pos) / dt
        angle, axis = quat_diff_angle_axis(prev_rb_rot, rb_rot)
        dof_vel = axis * angle.unsqueeze(-1) / dt
        return root_pos, rb_rot[:, 0], dof_pos, root_vel, dof_vel[:, 0] / dt, dof_vel[:, 1:].reshape(-1, 69), rb_pos, rb_rot

    def step(self, root_pos, joint_rotmat, residual, ball_pos, sim_root_pos, prev_root_pos, prev_rb_rot):
        st, pi = self.st, math.pi
        target_root = root_pos.clone() + residual
        if st["fix_head_orientation"]:
            _, _, _, _, _, _, rb_pos, rb_rot = self.smpl_to_sim(target_root, joint_rotmat)
            head = quat_to_rotmat(rb_rot[:, st["head_body"], [3, 0, 1, 2]])
            lookat = torch.matmul(head, torch.tensor([0.0, 0.0, 1.0], device=DEV))
            lookat = torch.nn.functional.normalize(lookat[:, :2], dim=-1)
            head_ball = torch.nn.functional.normalize(ball_pos[:, :2] - rb_pos[:, st["head_body"], :2], dim=-1)
            diff = torch.atan2(head_ball[:, 1], head_ball[:, 0]) - torch.atan2(lookat[:, 1], lookat[:, 0])
            diff[diff > pi] -= pi * 2
            diff[diff < -pi] += pi * 2
            miss = (ball_pos[:, 1] < sim_root_pos[:, 1] - 0.5) | (abs(ball_pos[:, 0]) > 4)
            diff[miss] = 0
            hn = [st["smpl_head"], st["smpl_neck"]]
            aa = quat_to_angle_axis_konia(rotmat_to_quat(joint_rotmat[:, hn]))
            aa[:, 0, 1] += diff / 2
            aa[:, 1, 1] += diff / 2
            new = joint_rotmat.clone()
            new[:, hn] = angle_axis_to_rotmat(aa)
            joint_rotmat[:] = new
        return self.smpl_to_sim(target_root, joint_rotmat, prev_root_pos, prev_rb_rot)


def make_batch(n, rng):
    """A racket + ball batch with a seeded generator and the target around them."""
    from tests import mvae_fixture as MF
    from tests.gpu_util import synth_tables
    from vid2player3d_amd import ball_traj
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    w, avg, std = MF.weights()
    player, _, z, res = make_pair(n, w, avg, std, rng)
    gen = ball_traj.TennisBallGenerator({"num_samples": 10000}, device=DEV, seed=3)
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=16, min_frames=60, max_frames=200), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "fix_head_orientation": True, "add_residual_root": True}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
    task.reset()
    bind = task.smpl_rest_joints[0].detach().cpu().numpy()
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    return task, player, target, z, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--small", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("mvae_target_bench measures on a GPU; there is none here")
    rng = np.random.default_rng(1)
    figures = {}
    for n in (args.small, args.envs):
        task, player, target, z, res = make_batch(n, rng)
        root_res = torch.as_tensor(rng.uniform(-0.02, 0.02, (n, 3)).astype(np.float32), device=DEV)
        target.reset(torch.arange(n, device=DEV))
        player.step(z, res)
        ref = TorchTarget(target.settings, target._joint_pos_bind[0], n)
        # the two forms compute the same step: checked once, before anything is timed
        prev = task._target_bufs[1 - task._cur]
        pose = player._joint_rotmat.clone()
        o = ref.step(player._root_pos, pose, root_res, task._ball_root_states[:, 0:3], task._rigid_body_pos[:, 0], prev[:, 0:3], prev[:, 235:331].view(n, 24, 4))
        target.step(root_res)
        torch.cuda.synchronize()
        row = task._target_bufs[task._cur]
        print(json.dumps({"check": "kernel against the torch transcription, one step", "envs": n, "rb_pos_max_abs_diff": float((row[:, 163:235] - o[6].reshape(n, 72)).abs().max()),
                          "dof_pos_max_abs_diff": float((row[:, 7:76] - o[2]).abs().max()), "joint_rotmat_max_abs_diff": float((player._joint_rotmat - pose).abs().max())}), flush=True)

        def torch_step(ref=ref, player=player, task=task, root_res=root_res, n=n):
            prev = task._target_bufs[1 - task._cur]
            ref.step(player._root_pos, player._joint_rotmat, root_res, task._ball_root_states[:, 0:3], task._rigid_body_pos[:, 0], prev[:, 0:3], prev[:, 235:331].view(n, 24, 4))

        def both(target=target, root_res=root_res):
            target.step(root_res)
            target.compute_observations()

        figures["target_ms_%d" % n] = (lambda target=target, root_res=root_res: target.step(root_res))
        figures["target_obs_ms_%d" % n] = both
        figures["torch_ms_%d" % n] = torch_step
    n = args.envs
    act, ll = torch.zeros((n, 75), device=DEV), torch.as_tensor(rng.normal(0, 0.3, (n, 75)).astype(np.float32), device=DEV)
    one_in, one_out = torch.zeros((1, 75), device=DEV), torch.zeros((1, 75), device=DEV)
    tensors = target._tensors(task._target_bufs[task._cur])
    for _ in range(5):
        task.step(act.clone())

    def pair():
        player.step(z, res)
        task.step(act)

    def pair_with_target():
        player.step(z, res)
        target.step(root_res)
        target.compute_observations()
        task.step(target.actions(ll))

    figures["launch_ms"] = lambda: mt.launch_actions(target.settings, tensors, 1, one_in, one_out)
    figures["pair_ms_%d" % n] = pair
    figures["pair_with_target_ms_%d" % n] = pair_with_target
    out = {k: [] for k in figures}
    for r in range(args.rounds):
        for k, fn in figures.items():
            ms = timed(fn, args.iters, args.warmup)
            out[k].append(ms)
            print(json.dumps({"figure": k, "round": r, "ms_per_step": round(ms, 5), "iters": args.iters}), flush=True)
    med = {k: float(np.median(v)) for k, v in out.items()}
    s = args.small
    hbm_ms = n * (READ_BYTES + WRITE_BYTES) / (HBM_TB_S * 1e12) * 1e3
    summary = {"summary": "imitation target of a control step, head rule on, residual root", **{k: round(v, 5) for k, v in med.items()},
               "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()},
               "torch_over_target_%d" % n: round(med["torch_ms_%d" % n] / med["target_ms_%d" % n], 2),
               "torch_over_target_%d" % s: round(med["torch_ms_%d" % s] / med["target_ms_%d" % s], 2),
               "bytes_per_env": {"read": READ_BYTES, "written": WRITE_BYTES}, "hbm_ms_%d_at_%.2f_TB_s" % (n, HBM_TB_S): round(hbm_ms, 5),
               "hbm_plus_one_launch_ms_%d" % n: round(hbm_ms + med["launch_ms"], 5),
               "target_over_hbm_plus_launch_%d" % n: round(med["target_ms_%d" % n] / (hbm_ms + med["launch_ms"]), 2),
               "target_adds_to_pair_ms_%d" % n: round(med["pair_with_target_ms_%d" % n] - med["pair_ms_%d" % n], 5),
               "target_share_of_pair": round((med["pair_with_target_ms_%d" % n] - med["pair_ms_%d" % n]) / med["pair_ms_%d" % n], 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
