"""Time the two-hand backhand fix at a record's size: 4 rallies x 2 sides x 600 frames, a third of them flagged (runs of 20 flagged
frames, 40 between them), 500 steps - `v2p_two_hand_fix`, one launch - against the reference's form in torch on the same GPU.

The reference's form (humanoid_smpl_im_mvae.py:948-1031) per track: every step writes the four joints' matrices into the pose tensor in
place, runs `_smpl_to_sim` over all 24 joints (angle-axis and quaternion outputs included), three L1 losses, `backward(retain_graph=True)`
and Adam.  Because the pose tensor is written in place and the graphs are retained, step k walks back through the k - 1 writes before
it: the cost of a step grows with the step.  It is restated here in torch with the same tensor operations (not the reference's code),
and timed for one track at --ref-iters steps (default 50 and 100: the full 500 would take minutes of GPU time for one figure); the
log gives the measured times and nothing extrapolated.

    python tools/two_hand_fix_bench.py [--reps 5] [--ref-iters 50,100]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vid2player3d_amd import two_hand_fix as thf  # noqa: E402
from vid2player3d_amd.model import load_baked_model  # noqa: E402
from vid2player3d_amd.mvae_target import SMPL_JOINT_NAMES  # noqa: E402

DEV = "cuda:0"
RALLIES, SIDES, FRAMES = 4, 2, 600


def make_record(seed=0):
    rng = np.random.default_rng(seed)
    T = RALLIES * SIDES
    jr = (rng.uniform(-0.4, 0.4, (T, 1, 24, 3)) + np.arange(FRAMES)[None, :, None, None] * rng.uniform(-0.001, 0.001, (T, 1, 24, 3)) +
          rng.uniform(-0.02, 0.02, (T, FRAMES, 24, 3))).astype(np.float32)
    flagged = (np.arange(FRAMES) % 60) < 20
    phase = np.where(flagged, 3.5, 1.0).astype(np.float32)[None].repeat(T, 0)
    swing = np.full((T, FRAMES), 2, np.int64)
    return jr, phase, swing, int(flagged.sum())


def bind_rows(model):
    rest = np.zeros((24, 3))
    for b in range(24):
        p = int(model.parents[b])
        rest[b] = np.asarray(model.local_pos[b], dtype=np.float64) + (rest[p] if p >= 0 else 0.0)
    rest = rest[[list(model.body_names).index(nm) for nm in SMPL_JOINT_NAMES]]
    return np.stack([rest, rest * 1.07]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the reference's form
def aa_to_rotmat(aa):
    theta2 = (aa * aa).sum(-1)
    theta = torch.sqrt(theta2.clamp_min(1e-6))
    w = aa / (theta + 1e-6).unsqueeze(-1)
    wx, wy, wz = w[..., 0], w[..., 1], w[..., 2]
    c, s = torch.cos(theta), torch.sin(theta)
    t = 1 - c
    normal = torch.stack([c + wx * wx * t, wx * wy * t - wz * s, wy * s + wx * wz * t, wz * s + wx * wy * t, c + wy * wy * t, -wx * s + wy * wz * t,
                          -wy * s + wx * wz * t, wx * s + wy * wz * t, c + wz * wz * t], -1)
    o = torch.ones_like(wx)
    rx, ry, rz = aa[..., 0], aa[..., 1], aa[..., 2]
    taylor = torch.stack([o, -rz, ry, rz, o, -rx, -ry, rx, o], -1)
    return torch.where((theta2 > 1e-6).unsqueeze(-1), normal, taylor).reshape(aa.shape[:-1] + (3, 3))


def rotmat_to_quat(m):
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., i, j] for i in range(3) for j in range(3)]
    trace = m00 + m11 + m22

    def szd(a, b):
        return a / torch.where(b.abs() < 1e-6, b + 1e-6, b)

    sq = torch.sqrt((trace + 1).clamp_min(1e-6)) * 2
    c0 = torch.stack([0.25 * sq, szd(m21 - m12, sq), szd(m02 - m20, sq), szd(m10 - m01, sq)], -1)
    sq = torch.sqrt((1 + m00 - m11 - m22).clamp_min(1e-6)) * 2
    c1 = torch.stack([szd(m21 - m12, sq), 0.25 * sq, szd(m01 + m10, sq), szd(m02 + m20, sq)], -1)
    sq = torch.sqrt((1 + m11 - m00 - m22).clamp_min(1e-6)) * 2
    c2 = torch.stack([szd(m02 - m20, sq), szd(m01 + m10, sq), 0.25 * sq, szd(m12 + m21, sq)], -1)
    sq = torch.sqrt((1 + m22 - m00 - m11).clamp_min(1e-6)) * 2
    c3 = torch.stack([szd(m10 - m01, sq), szd(m02 + m20, sq), szd(m12 + m21, sq), 0.25 * sq], -1)
    b1, b2 = ((m00 > m11) & (m00 > m22)).unsqueeze(-1), (m11 > m22).unsqueeze(-1)
    return torch.where((trace > 0).unsqueeze(-1), c0, torch.where(b1, c1, torch.where(b2, c2, c3)))


def quat_to_aa(q):
    w, xyz = q[..., 0], q[..., 1:]
    s2 = (xyz * xyz).sum(-1)
    s = torch.sqrt(s2.clamp_min(1e-6))
    two_theta = 2 * torch.where(w < 0, torch.atan2(-s, -w), torch.atan2(s, w))
    k = torch.where(s2 > 0, two_theta / s, torch.full_like(s, 2.0))
    return xyz * k.unsqueeze(-1)


def smpl_to_sim(rotmat, bind, parents, order):
    """the work of `_smpl_to_sim` with root position 0: dof_pos, the chain over 24 joints, the bodies' quaternions"""
    dof_pos = quat_to_aa(rotmat_to_quat(rotmat))[:, order][:, 1:].reshape(len(rotmat), -1)
    rel = bind.clone()
    rel[:, 1:] = bind[:, 1:] - bind[:, parents[1:]]
    R, p = [rotmat[:, 0]], [rel[:, 0]]
    for i in range(1, 24):
        R.append(torch.matmul(R[parents[i]], rotmat[:, i]))
        p.append(torch.matmul(R[parents[i]], rel[:, i].unsqueeze(-1)).squeeze(-1) + p[parents[i]])
    rb_rot = rotmat_to_quat(torch.stack(R, 1))[..., [1, 2, 3, 0]][:, order]
    rb_pos = torch.stack(p, 1)[:, order] - bind[:, :1]
    return dof_pos, rb_pos, rb_rot


def reference_form(st, jr, bind, righthand, iters):
    """one track's flagged frames jr [F,24,3] through the reference's loop"""
    parents, order = st["smpl_parents"], st["smpl_of_body"]
    hand, wrist, free = thf.BODIES[righthand]
    ik = list(thf.IK_JOINTS[righthand])
    joint_rotmat = aa_to_rotmat(jr)
    bind_f = bind[torch.arange(len(jr), device=jr.device) % len(bind)]
    rb = smpl_to_sim(joint_rotmat, bind_f, parents, order)[1]
    target = 2 * rb[:, hand] - rb[:, wrist] - rb[:, 0]
    origin = quat_to_aa(rotmat_to_quat(joint_rotmat[:, ik])).clone()
    delta = torch.zeros_like(origin, requires_grad=True)
    opt = torch.optim.Adam([delta], lr=0.005, betas=(0.9, 0.999))
    l1 = torch.nn.L1Loss()

    def closure():
        opt.zero_grad()
        joint_rotmat[:, ik] = aa_to_rotmat(origin + delta)
        cur = smpl_to_sim(joint_rotmat, bind_f, parents, order)[1][:, free]
        loss = l1(cur, target.detach()) + l1(delta, torch.zeros_like(delta)) * 0.2 + l1(delta[1:], delta[:-1].detach()) * 0.5
        loss.backward(retain_graph=True)
        return loss

    for _ in range(iters):
        opt.step(closure)
    joint_rotmat[:, ik] = aa_to_rotmat(origin + delta)
    return quat_to_aa(rotmat_to_quat(joint_rotmat.detach()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-iters", default="50,100")
    a = ap.parse_args()
    model = load_baked_model()
    st = thf.fix_settings(model.body_names, model.parents)
    jr, phase, swing, F = make_record()
    T = len(jr)
    dev = lambda x: torch.as_tensor(x, device=DEV)
    t = dict(joint_rot=dev(jr), phase=dev(phase), swing_type=dev(swing), nframes=torch.full((T,), FRAMES, dtype=torch.int32, device=DEV),
             righthand=dev(np.arange(T, dtype=np.int32) % 2), bind=dev(bind_rows(model)))
    print("record: %d rallies x %d sides x %d frames, %d flagged per track, %d tracks in one launch" % (RALLIES, SIDES, FRAMES, F, T))
    for iters in (1, 100, 500):
        times = []
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, overflow = thf.fix_two_hand_backhand(t["joint_rot"], t["phase"], t["swing_type"], t["nframes"], t["righthand"], t["bind"], iters, settings=st, check=False)
            e1.record()
            torch.cuda.synchronize()
            if rep:  # (the first launch loads the code object)
                times.append(e0.elapsed_time(e1))
        assert not bool(overflow.any())
        print("v2p_two_hand_fix, %3d steps: %.3f ms median of %d (min %.3f, max %.3f), the returned tensor's allocation included" % (
            iters, float(np.median(times)), len(times), min(times), max(times)))
    moved = float((out - t["joint_rot"]).abs().max())
    print("largest change of an angle after 500 steps: %.3f rad" % moved)
    flagged = dev((np.arange(FRAMES) % 60) < 20)
    for iters in [int(x) for x in a.ref_iters.split(",") if x]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = reference_form(st, t["joint_rot"][0][flagged].clone(), t["bind"], False, iters)
        torch.cuda.synchronize()
        dt_ = time.perf_counter() - t0
        print("the reference's form in torch, ONE track (%d flagged frames), %3d steps: %.1f ms wall (%.2f ms per step); a record has %d tracks and 500 steps" % (
            F, iters, dt_ * 1e3, dt_ * 1e3 / iters, T))
        if iters == 100:
            mine = thf.fix_two_hand_backhand(t["joint_rot"][:1].contiguous(), t["phase"][:1].contiguous(), t["swing_type"][:1].contiguous(), t["nframes"][:1].contiguous(),
                                             t["righthand"][:1].contiguous(), t["bind"], iters, settings=st)[0][flagged]
            print("  the two after 100 steps: largest difference of an angle %.3g rad (the law takes the sign of rounding noise)" % float((mine - ref).abs().max()))


if __name__ == "__main__":
    main()
