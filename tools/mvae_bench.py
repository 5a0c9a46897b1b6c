"""What one control step of the MotionVAE motion generator costs on the GPU (vid2player3d_amd/mvae.py):

    kernel      MotionVAEPlayer.step: one launch of v2p_mvae_step (gate + three expert-blended layers on the fp32 MFMA + state update)
    torch       the same step written in torch on device tensors in the reference's form: the six experts' weights blended PER ENV
                (`torch.matmul(coefficients, flat_weight)`), one `baddbmm` with a weight matrix per env (motion_vae/model.py:237-252),
                then `_update_mvae_state` op by op (players/mvae_player.py:254-422) - the transcription below; it lives here, not in
                the product
    physics     the racket + ball step (HumanoidSMPLIMRacketBall.step) alone, and followed by the generator's kernel step

kernel and torch at 1024 and at 8192 envs, physics at 8192; federer, right-handed, training mode, with residuals.  Every timing is taken
with device events around `--iters` repetitions after `--warmup` repetitions, three rounds each, alternating the candidates; one JSON line
per figure and a summary line at the end.
    python tools/mvae_bench.py [--envs 8192] [--iters 100] [--warmup 10]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vid2player3d_amd import mvae  # noqa: E402

DEV = "cuda:0"


def rot6d_to_rotmat(r6, eps=1e-8):
    a1, a2 = r6[..., :3].clone(), r6[..., 3:].clone()
    a1[torch.norm(a1, dim=-1) < eps] = torch.tensor([1.0, 0.0, 0.0], device=r6.device)
    b1 = a1 / a1.norm(dim=-1).clamp(min=1e-9).unsqueeze(-1)
    u = a2 - (b1 * a2).sum(dim=-1).unsqueeze(-1) * b1
    b2 = u / u.norm(dim=-1).clamp(min=1e-9).unsqueeze(-1)
    b2[torch.norm(b2, dim=-1) < eps] = torch.tensor([0.0, 1.0, 0.0], device=r6.device)
    return torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], dim=-1)


def safe_div(num, den, eps=1e-6):
    den = den.clone()
    den[den.abs() < eps] += eps
    return num / den


def rotmat_to_quat(m, eps=1e-6):
    """konia_transform.rotation_matrix_to_quaternion, op by op (w, x, y, z)"""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., i, j] for i in range(3) for j in range(3)]
    trace = m00 + m11 + m22
    sq = torch.sqrt((trace + 1.0).clamp_min(eps)) * 2.0
    c0 = torch.stack((0.25 * sq, safe_div(m21 - m12, sq), safe_div(m02 - m20, sq), safe_div(m10 - m01, sq)), dim=-1)
    sq = torch.sqrt((1.0 + m00 - m11 - m22).clamp_min(eps)) * 2.0
    c1 = torch.stack((safe_div(m21 - m12, sq), 0.25 * sq, safe_div(m01 + m10, sq), safe_div(m02 + m20, sq)), dim=-1)
    sq = torch.sqrt((1.0 + m11 - m00 - m22).clamp_min(eps)) * 2.0
    c2 = torch.stack((safe_div(m02 - m20, sq), safe_div(m01 + m10, sq), 0.25 * sq, safe_div(m12 + m21, sq)), dim=-1)
    sq = torch.sqrt((1.0 + m22 - m00 - m11).clamp_min(eps)) * 2.0
    c3 = torch.stack((safe_div(m10 - m01, sq), safe_div(m02 + m20, sq), safe_div(m12 + m21, sq), 0.25 * sq), dim=-1)
    w2 = torch.where((m11 > m22).unsqueeze(-1), c2, c3)
    w1 = torch.where(((m00 > m11) & (m00 > m22)).unsqueeze(-1), c1, w2)
    return torch.where((trace > 0.0).unsqueeze(-1), c0, w1)


def quat_to_angle_axis_konia(q, eps=1e-6):
    """konia_transform.quaternion_to_angle_axis of (w, x, y, z), op by op"""
    cos, q1, q2, q3 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    s2 = q1 * q1 + q2 * q2 + q3 * q3
    s = torch.sqrt(s2.clamp_min(eps))
    two_theta = 2.0 * torch.where(cos < 0.0, torch.atan2(-s, -cos), torch.atan2(s, cos))
    k = torch.where(s2 > 0.0, safe_div(two_theta, s), 2.0 * torch.ones_like(s))
    return torch.stack((q1 * k, q2 * k, q3 * k), dim=-1)


def rotmat_to_angle_axis(m):
    """konia_transform.rotation_matrix_to_angle_axis"""
    return quat_to_angle_axis_konia(rotmat_to_quat(m))


def angle_axis_to_rotmat(aa, eps=1e-6):
    """konia_transform.angle_axis_to_rotation_matrix, op by op"""
    shape = aa.shape
    aa = aa.reshape(-1, 3)
    theta2 = (aa * aa).sum(-1, keepdim=True)
    theta = torch.sqrt(theta2.clamp_min(eps))
    wx, wy, wz = torch.chunk(aa / (theta + eps), 3, dim=1)
    c, s = torch.cos(theta), torch.sin(theta)
    normal = torch.cat([c + wx * wx * (1 - c), wx * wy * (1 - c) - wz * s, wy * s + wx * wz * (1 - c), wz * s + wx * wy * (1 - c), c + wy * wy * (1 - c),
                        -wx * s + wy * wz * (1 - c), -wy * s + wx * wz * (1 - c), wx * s + wy * wz * (1 - c), c + wz * wz * (1 - c)], dim=1).view(-1, 3, 3)
    rx, ry, rz = torch.chunk(aa, 3, dim=1)
    one = torch.ones_like(rx)
    taylor = torch.cat([one, -rz, ry, rz, one, -rx, -ry, rx, one], dim=1).view(-1, 3, 3)
    mask = (theta2 > eps).view(-1, 1, 1)
    return (mask.type_as(theta2) * normal + (~mask).type_as(theta2) * taylor).view(shape[:-1] + (3, 3))


class TorchPlayer:
    """`MVAEPlayer.step` of the reference on device tensors (the yardstick: what the step costs without the kernel).  State is its own."""

    def __init__(self, st, w, avg, std, player):
        dev = player.device
        T = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        self.st, self.n = st, player.num_envs
        self.layers = [(T(w["w%d" % i]), T(w["b%d" % i])) for i in range(3)]
        self.gate = [(T(w["gate_w%d" % i]), T(w["gate_b%d" % i])) for i in range(3)]
        self.avg, self.std = T(avg), T(std)
        for k in ("conditions", "root_pos", "root_vel", "joint_rot6d", "joint_rotmat", "joint_rot", "phase_pred", "swing_type", "swing_type_cycle"):
            setattr(self, k, getattr(player, "_" + k).clone())
        self.joints = torch.tensor([mvae.RELBOW, mvae.RWRIST] if st["righthand"] else [mvae.LELBOW, mvae.LWRIST], device=dev)

    def decoder(self, z, c):
        F = torch.nn.functional
        g = torch.cat((z, c), dim=1)
        for i, (W, b) in enumerate(self.gate):
            g = F.linear(g, W, b)
            g = F.elu(g) if i < 2 else g
        coefficients = F.softmax(g, dim=1)
        layer_out = c
        for i, (weight, bias) in enumerate(self.layers):
            flat_weight = weight.flatten(start_dim=1, end_dim=2)
            mixed_weight = torch.matmul(coefficients, flat_weight).view(coefficients.shape[0], *weight.shape[1:3])
            inp = torch.cat((z, layer_out), dim=1).unsqueeze(1)
            mixed_bias = torch.matmul(coefficients, bias).unsqueeze(1)
            out = torch.baddbmm(mixed_bias, inp, mixed_weight).squeeze(1)
            layer_out = F.elu(out) if i < 2 else out
        return layer_out

    def step(self, latents, residual):
        st, n = self.st, self.n
        out = self.decoder(latents.float(), self.conditions.flatten(start_dim=1, end_dim=2)).float().view(-1, 1, mvae.OUT)
        feature, phase = out[:, 0, :-2], out[:, 0, -2:]
        self.conditions = self.conditions.roll(-1, dims=1)
        self.conditions[:, -1] = feature
        feature = feature * self.std + self.avg
        self.root_pos = self.root_pos + feature[:, 3:6]
        self.conditions[:, -1, 0:3] = (self.root_pos - self.avg[0:3]) / self.std[0:3]
        self.root_vel[:] = feature[:, 3:6]
        r6 = feature[:, 144:288].view(-1, 24, 6)
        self.joint_rot6d[:] = r6
        self.joint_rotmat[:] = rot6d_to_rotmat(r6)
        joint_pos = feature[:, 6:75].view(-1, 23, 3)
        self.phase_pred[:] = torch.atan2(phase[:, 0], phase[:, 1])
        self.phase_pred[:] = torch.where(self.phase_pred < 0, self.phase_pred + math.pi * 2, self.phase_pred)
        p, rh = self.phase_pred, st["righthand"]
        self.swing_type[:] = torch.where((self.swing_type == -1) & (p > 2.0) & (p < 3.5),
                                         torch.where(joint_pos[:, mvae.RWRIST - 1, 0] > 0, torch.ones_like(self.swing_type) * (1 if rh else 2),
                                                     torch.ones_like(self.swing_type) * (2 if rh else 1)), self.swing_type)
        self.swing_type[:] = torch.where((self.swing_type != -1) & (p > 3.5), torch.zeros_like(self.swing_type) - 1, self.swing_type)
        self.swing_type_cycle[:] = torch.where(self.swing_type != -1, self.swing_type, self.swing_type_cycle)
        if residual is not None:
            residual = torch.clamp(residual.clone() * 0.25, -0.25, 0.25)
            aa = rotmat_to_angle_axis(self.joint_rotmat[:, self.joints])
            rule = mvae.RESIDUAL_RULES[st["player"]]
            base = {k: torch.zeros(n, device=p.device) for k in ("elbow", "twist", "shake", "swing")}
            for s, lo, hi, ge, values in rule["rows"]:
                m = ((p >= lo) if ge else (p > lo)) & (p < hi) & (self.swing_type == s)
                for k, v in values.items():
                    base[k][m] = v
            if not st["is_train"]:
                (f0, f1), (b0, b1) = rule["swings"]
                swings = ((p > f0) & (p < f1) & (self.swing_type == 1)) | ((p > b0) & (p < b1) & (self.swing_type == 2))
                residual[~swings, :] = 0
            aa[:, 0, 0] = (base["elbow"] + residual[:, 0]) * math.pi
            aa[:, 1, 0] = base["twist"] * math.pi
            aa[:, 1, 1] = (base["shake"] + residual[:, 1]) * math.pi
            aa[:, 1, 2] = (base["swing"] + residual[:, 2]) * math.pi
            self.joint_rotmat[:, self.joints] = angle_axis_to_rotmat(aa)
            m = self.joint_rotmat[:, self.joints]
            self.joint_rot6d[:, self.joints] = torch.cat([m[..., 0], m[..., 1]], dim=-1)
        if not st["is_train"]:
            self.joint_rot[:] = rotmat_to_angle_axis(rot6d_to_rotmat(self.joint_rot6d))


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


def make_pair(n, w, avg, std, rng):
    cfg = {"player": "federer", "righthand": True, "add_residual_dof": "euler"}
    init = (avg + std * rng.normal(0, 0.8, (n, mvae.FRAME))).astype(np.float32)
    player = mvae.MotionVAEPlayer(cfg, n, w, avg, std, init, rng.uniform(-0.3, 0.3, (24, 3)).astype(np.float32), True, DEV)
    player.reset(torch.arange(n, device=DEV))
    player._swing_type.copy_(torch.as_tensor(rng.integers(-1, 4, n)))
    player._swing_type_cycle.copy_(player._swing_type)
    ref = TorchPlayer(player.settings, w, avg, std, player)
    z = torch.as_tensor(np.clip(rng.normal(0, 1, (n, mvae.LATENT)), -3, 3).astype(np.float32), device=DEV)
    res = torch.as_tensor(rng.uniform(-2, 2, (n, 3)).astype(np.float32), device=DEV)
    return player, ref, z, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--small", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-physics", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("mvae_bench measures on a GPU; there is none here")
    from tests import mvae_fixture as FX

    w, avg, std = FX.weights()
    rng = np.random.default_rng(1)
    figures = {}
    players = {}
    for n in (args.small, args.envs):
        player, ref, z, res = make_pair(n, w, avg, std, rng)
        # the two forms compute the same step: checked once, before anything is timed
        player.step(z, res)
        ref.step(z, res)
        torch.cuda.synchronize()
        diff = float((player._conditions - ref.conditions).abs().max())
        same = bool((player._swing_type == ref.swing_type).all())
        print(json.dumps({"check": "kernel against the torch transcription, one step", "envs": n, "conditions_max_abs_diff": diff, "swing_types_equal": same}), flush=True)
        players[n] = (player, z, res)
        figures["kernel_ms_%d" % n] = (lambda p=player, z=z, r=res: p.step(z, r))
        figures["torch_ms_%d" % n] = (lambda p=ref, z=z, r=res: p.step(z, r))
    if not args.no_physics:
        from tests.gpu_util import synth_tables
        from vid2player3d_amd import ball_traj
        from vid2player3d_amd.motion_lib import MotionLib
        from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

        n = args.envs
        gen = ball_traj.TennisBallGenerator({"num_samples": 10000}, device=DEV, seed=3)
        cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=16, min_frames=60, max_frames=200), DEV), sample_first_motions=True,
                          body_shape_mismatch="ignore", contact_solver="tgs")
        cfg["sim"].update({"substeps": 6})
        cfg["sim"]["physx"]["num_position_iterations"] = 2
        cfg["v2p"] = {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5}
        task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
        task.reset()
        act = torch.zeros((n, 75), device=DEV)
        for _ in range(5):
            task.step(act.clone())
        player, z, res = players[n]

        def both():
            player.step(z, res)
            task.step(act)

        figures["physics_ms_%d" % n] = lambda: task.step(act)
        figures["physics_plus_generator_ms_%d" % n] = both
    out = {k: [] for k in figures}
    for r in range(args.rounds):
        for k, fn in figures.items():
            ms = timed(fn, args.iters, args.warmup)
            out[k].append(ms)
            print(json.dumps({"figure": k, "round": r, "ms_per_step": round(ms, 5), "iters": args.iters}), flush=True)
    med = {k: float(np.median(v)) for k, v in out.items()}
    n, s = args.envs, args.small
    summary = {"summary": "MotionVAE generator step, federer, training mode, with residuals", **{k: round(v, 5) for k, v in med.items()},
               "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()},
               "torch_over_kernel_%d" % n: round(med["torch_ms_%d" % n] / med["kernel_ms_%d" % n], 2),
               "torch_over_kernel_%d" % s: round(med["torch_ms_%d" % s] / med["kernel_ms_%d" % s], 2),
               "kernel_tflops_%d" % n: round(2.87e6 * n / (med["kernel_ms_%d" % n] * 1e-3) / 1e12, 2), "device": torch.cuda.get_device_name(0)}
    if not args.no_physics:
        summary["generator_share_of_physics"] = round(med["kernel_ms_%d" % n] / med["physics_ms_%d" % n], 4)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
