"""The two-hand backhand fix of a record: `HumanoidSMPLIMMVAE.optimize_two_hand_backhand(single=True)`
(vid2player/env/tasks/humanoid_smpl_im_mvae.py:948-1031) as `run.py --test` applies it to every rally it keeps, cfg v2p
`fix_two_hand_backhand_post` (`MVAEControllerVis.render_one_result`, mvae_controller_vis.py:181-190; `MVAEControllerVisDual.render_one_result`,
mvae_controller_vis_dual.py:213-231): the frames of a two-hand backhand get 500 Adam steps of inverse kinematics on the free arm, so
that the free hand lands on the racket handle, and their poses are written back.

`two_hand_fix_reference` states the law once in numpy for one track (dt = numpy.float64 evaluates the same statement in double
precision); `fix_two_hand_backhand` is the launch, `v2p_two_hand_fix` (csrc/two_hand_fix.hip): one workgroup per track, all tracks of a
call in one launch, no allocation beyond the returned tensor and the tracks' `overflow` words, whose read after the launch (the cap's
refusal) is the one host read.  Kernel and statement agree in every bit - the law takes
the sign of rounding noise (after the first step `delta[i] - delta[i-1]` is 0 or an ulp), so a kernel one ulp away would end up
hundredths of a radian away.  For that every operation of the law is `+ - * / sqrt` in the statement's order, sine, cosine and the
closing arctangent are evaluated in double and rounded once (`wide_trig`, `wide_atan2` of ref_rotations.py), and Adam's bias terms come
from running products in double, which give the float32 values of torch's `beta ** step` for every step up to 500 (tests).

The law, per track, with joint_rot [nframes,24,3], phase, swing_type, righthand and bind rows [R,24,3]:
  1. need_fix = (swing_type == 2) & (phase > 2) & (phase < 5); the F flagged frames are compacted in frame order.  Adjacent compacted
     frames may belong to different swings: the reference smooths across them, and so does this.
  2. all 24 joints of a flagged frame go angle_axis_to_rotmat, then (after the optimisation) rotmat_to_angle_axis: the joints that are
     not optimised change by a round trip, as in the reference.  Frames that are not flagged are copied.
  3. forward kinematics is `smpl_to_sim_reference` with root position 0; compacted frame i reads bind row i % R - the reference's
     `joint_pos_bind[:batch_size]`: R = 1 for one shape, R = 2 for `dual_mode: different`, where CONSECUTIVE FLAGGED FRAMES alternate
     between the two players' skeletons whichever side the track belongs to (a quirk of the reference, reproduced), R = N for per-env
     rows; where the reference would run out of rows (F > N) the pattern continues.
  4. bodies (hand, wrist, free hand) are (23, 22, 18) for a right-handed player and (18, 17, 23) otherwise;
     target = 2 rb_pos[hand] - rb_pos[wrist] - rb_pos[0] from the input pose.  The unknowns delta [F,4,3] start at 0 and are added to
     the angle-axis vectors (the round trip's) of the free arm's SMPL joints (wrist, elbow, shoulder, collar) = (20, 18, 16, 13) for a
     right-handed player, (21, 19, 17, 14) otherwise.
  5. loss = mean|p_free - target| + 0.2 mean|delta| + 0.5 mean|delta[1:] - delta[:-1].detach()|: the gradients are signs over the
     counts 3F, 12F, 12(F-1) with sign(0) = 0, the smoothness gradient goes to the later frame only.  F = 1 has no smoothness term.
     The gradient of the first term is written by hand: the free hand is a product of four Rodrigues matrices behind a constant prefix,
     each of the twelve partials is (prefix^T g) . dR/dtheta (suffix), with the `theta + 1e-6` denominator and the constant first-order
     branch at theta^2 <= 1e-6 as `angle_axis_to_rotmat_reference` reads.
  6. Adam as torch's single-tensor form runs it, lr 0.005, betas (0.9, 0.999), eps 1e-8, `num_iters` steps (default 500).

Left out: `single=False` (no caller in the reference, and it dies at its last `print`), `infer_racket_from_smpl`, the SMPL mesh, video.
There is no CPU path: a CPU tensor or a missing library is a RuntimeError."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .ref_rotations import angle_axis_to_rotmat_reference, rotmat_to_angle_axis_reference

NUM_ITERS = 500
LR, BETA1, BETA2, EPS = 0.005, 0.9, 0.999, 1e-8
W_REG, W_SMOOTH = 0.2, 0.5
MAX_FRAMES = _lib.TWO_HAND_FIX_MAX_FRAMES  # flagged frames of one track: eight per thread of the track's workgroup of 256
# (hand, wrist, free hand) bodies and the free arm's SMPL joints (wrist, elbow, shoulder, collar), by righthand
BODIES = {True: (23, 22, 18), False: (18, 17, 23)}
IK_JOINTS = {True: (20, 18, 16, 13), False: (21, 19, 17, 14)}


def fix_settings(body_names, parents):
    """What the kernel's v2p_two_hand_fix_cfg and the statement are made from: the SMPL tree of the body model and `_smpl_2_mujoco`.
    Checked here: each free arm is the chain collar - shoulder - elbow - wrist - hand, and the bodies of the law are those hands."""
    from .mvae_target import tree_from_model

    smpl_parents, smpl_of_body = tree_from_model(body_names, parents)
    for rh in (True, False):
        w, e, s, c = IK_JOINTS[rh]
        hand = smpl_of_body[BODIES[rh][2]]
        if [smpl_parents[hand], smpl_parents[w], smpl_parents[e], smpl_parents[s]] != [w, e, s, c] or smpl_of_body[0] != 0:
            raise ValueError("two-hand fix: the body model's free arm is not the SMPL chain collar - shoulder - elbow - wrist - hand")
        if smpl_parents[smpl_of_body[BODIES[rh][0]]] != smpl_of_body[BODIES[rh][1]]:
            raise ValueError("two-hand fix: the racket wrist's body is not the parent of the racket hand's")
    # (control_dt: nothing of the fix reads it - `smpl_to_sim_reference` takes it from its settings for the velocities, which are not used here)
    return dict(smpl_parents=list(smpl_parents), smpl_of_body=list(smpl_of_body), control_dt=1.0 / 30.0)


def check_frames(F):
    if F > MAX_FRAMES:
        raise ValueError("two-hand fix: %d flagged frames in one track, above the cap of %d" % (F, MAX_FRAMES))


def need_fix_reference(phase, swing_type):
    phase = np.asarray(phase, dtype=np.float32)
    return (np.asarray(swing_type) == 2) & (phase > np.float32(2.0)) & (phase < np.float32(5.0))


def adam_terms(num_iters):
    """(step_size [num_iters], bias_correction2_sqrt [num_iters]) in float64, from running products (what the kernel forms)."""
    b1 = b2 = 1.0
    step, bc2 = np.zeros(num_iters), np.zeros(num_iters)
    for t in range(num_iters):
        b1, b2 = b1 * BETA1, b2 * BETA2
        step[t], bc2[t] = LR / (1.0 - b1), np.sqrt(1.0 - b2)
    return step, bc2


def _matmul(P, m):
    """P @ m as batch_rigid_transform's statement sums it (mvae_target._chain)"""
    return P[:, :, 0:1] * m[:, None, 0, :] + P[:, :, 1:2] * m[:, None, 1, :] + P[:, :, 2:3] * m[:, None, 2, :]


def _matvec(P, t):
    return P[:, :, 0] * t[:, 0:1] + P[:, :, 1] * t[:, 1:2] + P[:, :, 2] * t[:, 2:3]


def _mattvec(P, g):
    return P[:, 0, :] * g[:, 0:1] + P[:, 1, :] * g[:, 1:2] + P[:, 2, :] * g[:, 2:3]


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def rodrigues_partials(r, q, u, dt):
    """d/dr of q^T R(r) u, [F,3], R = angle_axis_to_rotmat_reference (both branches): with theta = |r|, d = theta + 1e-6, w = r / d,
    e = r / theta, b = u x q it is
        e S + t ((q/d - e (r.q)/d^2) (w.u) + (w.q) (u/d - e (r.u)/d^2)) + s (b/d - e (r.b)/d^2),
        S = s ((w.q)(w.u) - q.u) + c (w.b), t = 1 - c,
    and b on the first-order branch."""
    eps, one = dt(1e-6), dt(1)
    b = np.stack([u[:, 1] * q[:, 2] - u[:, 2] * q[:, 1], u[:, 2] * q[:, 0] - u[:, 0] * q[:, 2], u[:, 0] * q[:, 1] - u[:, 1] * q[:, 0]], -1)
    theta2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
    theta = np.sqrt(np.maximum(theta2, eps))
    d = theta + eps
    c, s = np.cos(theta.astype(np.float64)).astype(dt), np.sin(theta.astype(np.float64)).astype(dt)
    t = one - c
    w, e = r / d[:, None], r / theta[:, None]
    wq, wu, qu, wb = _dot(w, q), _dot(w, u), _dot(q, u), _dot(w, b)
    rq, ru, rb = _dot(r, q) / (d * d), _dot(r, u) / (d * d), _dot(r, b) / (d * d)
    S = s * (wq * wu - qu) + c * wb
    normal = (e * S[:, None] + t[:, None] * ((q / d[:, None] - e * rq[:, None]) * wu[:, None] + wq[:, None] * (u / d[:, None] - e * ru[:, None]))
              + s[:, None] * (b / d[:, None] - e * rb[:, None]))
    return np.where((theta2 > eps)[:, None], normal, b).astype(dt)


def free_hand_reference(r, con, dt, grad_scale=None):
    """The free hand's position of r [F,4,3] (the angle-axis vectors of wrist, elbow, shoulder, collar) behind the constants `con`, as
    `smpl_to_sim_reference` computes it: (p_free [F,3], diff = p_free - target, and with grad_scale the gradient [F,4,3] of
    sum(sign(diff) * grad_scale . p_free))."""
    G, p13, off, bind0, target = con["G"], con["p13"], con["off"], con["bind0"], con["target"]
    D, Cm, B, A = [angle_axis_to_rotmat_reference(r[:, k], dt, wide_trig=True) for k in range(4)]
    G13 = _matmul(G, A)
    p16 = _matvec(G13, off[:, 0]) + p13
    G16 = _matmul(G13, B)
    p18 = _matvec(G16, off[:, 1]) + p16
    G18 = _matmul(G16, Cm)
    p20 = _matvec(G18, off[:, 2]) + p18
    G20 = _matmul(G18, D)
    p22 = _matvec(G20, off[:, 3]) + p20
    p_free = p22 - bind0
    diff = p_free - target
    if grad_scale is None:
        return p_free, diff, None
    g = np.sign(diff) * grad_scale
    uD = off[:, 3]
    uC = off[:, 2] + _matvec(D, uD)
    uB = off[:, 1] + _matvec(Cm, uC)
    uA = off[:, 0] + _matvec(B, uB)
    grad = np.stack([rodrigues_partials(r[:, 0], _mattvec(G18, g), uD, dt), rodrigues_partials(r[:, 1], _mattvec(G16, g), uC, dt),
                     rodrigues_partials(r[:, 2], _mattvec(G13, g), uB, dt), rodrigues_partials(r[:, 3], _mattvec(G, g), uA, dt)], 1)
    return p_free, diff, grad.astype(dt)


def fix_constants(st, rotmat, bind_rows, righthand, dt):
    """Per flagged frame, computed once from the input pose: the prefix G (the global rotation of the collar's parent), the collar's
    position p13, the four offsets of the chain, the root's bind position and the target."""
    from .mvae_target import _chain, smpl_to_sim_reference

    F = len(rotmat)
    par = st["smpl_parents"]
    hand_b, wrist_b, free_b = BODIES[bool(righthand)]
    w, e, s, c = IK_JOINTS[bool(righthand)]
    free_j = st["smpl_of_body"][free_b]
    rb = smpl_to_sim_reference(st, np.zeros((F, 3), dt), rotmat, bind_rows, dt=dt)["rb_pos"]
    target = dt(2) * rb[:, hand_b] - rb[:, wrist_b] - rb[:, 0]
    posed, rot = _chain(rotmat, bind_rows, par, dt)
    off = np.stack([bind_rows[:, j] - bind_rows[:, par[j]] for j in (s, e, w, free_j)], 1)
    return dict(G=rot[:, par[c]], p13=posed[:, c], off=off.astype(dt), bind0=bind_rows[:, 0], target=target.astype(dt))


def two_hand_fix_reference(st, joint_rot, phase, swing_type, righthand, bind, num_iters=NUM_ITERS, dt=np.float32, info=None):
    """The law on one track: joint_rot [nframes,24,3], phase / swing_type [nframes], bind [R,24,3] or [24,3].  Returns the fixed copy
    [nframes,24,3] in dt.  info (a dict) receives `delta` [F,4,3], `target_loss` (the first term at the last evaluation, as the
    reference prints it; NaN without one), `first_grad` [F,4,3] (the first step's gradient) and `frames`."""
    joint_rot = np.asarray(joint_rot, dtype=np.float32)
    out = joint_rot.astype(dt).copy()
    frames = np.flatnonzero(need_fix_reference(phase, swing_type))
    F = len(frames)
    check_frames(F)
    if info is not None:
        info.update(frames=frames, delta=np.zeros((F, 4, 3), dt), target_loss=float("nan"), first_grad=np.zeros((F, 4, 3), dt))
    if F == 0:
        return out
    bind = np.asarray(bind, dtype=np.float32).reshape(-1, 24, 3).astype(dt)
    bind_rows = bind[np.arange(F) % len(bind)]
    ik = list(IK_JOINTS[bool(righthand)])
    rotmat = angle_axis_to_rotmat_reference(joint_rot[frames].astype(dt), dt, wide_trig=True)
    trip = rotmat_to_angle_axis_reference(rotmat, dt, wide_atan2=True)
    origin = trip[:, ik]
    con = fix_constants(st, rotmat, bind_rows, righthand, dt)
    delta, m, v = np.zeros((F, 4, 3), dt), np.zeros((F, 4, 3), dt), np.zeros((F, 4, 3), dt)
    g_target = dt(1) / dt(3 * F)
    g_reg = dt(W_REG) / dt(12 * F)
    g_smooth = dt(W_SMOOTH) / dt(12 * (F - 1)) if F > 1 else dt(0)
    step_size, bc2_sqrt = adam_terms(int(num_iters))
    for t in range(int(num_iters)):
        _, diff, grad = free_hand_reference(origin + delta, con, dt, g_target)
        g = grad + np.sign(delta) * g_reg
        if F > 1:
            sm = np.zeros_like(delta)
            sm[1:] = np.sign(delta[1:] - delta[:-1]) * g_smooth
            g = g + sm
        if info is not None:
            info["target_loss"] = float(np.abs(diff.astype(np.float64)).mean())
            if t == 0:
                info["first_grad"] = g.copy()
        m = m + (g - m) * dt(1.0 - BETA1)
        v = v * dt(BETA2) + dt(1.0 - BETA2) * g * g
        denom = np.sqrt(v) / dt(bc2_sqrt[t]) + dt(EPS)
        delta = delta - dt(step_size[t]) * m / denom
    if info is not None:
        info["delta"] = delta.copy()
    rotmat[:, ik] = angle_axis_to_rotmat_reference(origin + delta, dt, wide_trig=True)
    out[frames] = rotmat_to_angle_axis_reference(rotmat, dt, wide_atan2=True)
    return out


# ------------------------------------------------------------------------------------------------------------------ the launch
def cfg_struct(st, num_iters, num_bind):
    c = _lib.TwoHandFixCfg(num_iters=int(num_iters), num_bind=int(num_bind))
    c.smpl_parents[:] = st["smpl_parents"]
    c.smpl_of_body[:] = st["smpl_of_body"]
    return c


def launch_fix(st, tensors, num_iters=NUM_ITERS):
    """v2p_two_hand_fix over a dict of device tensors under _lib.TWO_HAND_FIX_BUFFER_NAMES: joint_rot [T,L,24,3] float32, phase [T,L]
    float32, swing_type [T,L] int64, nframes [T] int32, righthand [T] int32, bind [R,24,3] float32, out [T,L,24,3] float32 (another
    tensor than joint_rot), overflow [T] int32.  Every size is checked here: the kernel trusts them."""
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    joint_rot = tensors.get("joint_rot")
    if not torch.is_tensor(joint_rot) or not joint_rot.is_cuda:
        raise RuntimeError("two-hand fix: joint_rot must be a GPU tensor (there is no CPU path)")
    if joint_rot.dim() != 4 or tuple(joint_rot.shape[2:]) != (24, 3):
        raise ValueError("two-hand fix: joint_rot must be [T,L,24,3], got %s" % (tuple(joint_rot.shape),))
    T, L = int(joint_rot.shape[0]), int(joint_rot.shape[1])
    if int(num_iters) < 0:
        raise ValueError("two-hand fix: num_iters %d < 0" % int(num_iters))
    dev = joint_rot.device
    want = dict(joint_rot=(f32, T * L * 72), phase=(f32, T * L), swing_type=(i64, T * L), nframes=(i32, T), righthand=(i32, T), out=(f32, T * L * 72), overflow=(i32, T))
    unknown = set(tensors) - set(_lib.TWO_HAND_FIX_BUFFER_NAMES)
    if unknown:
        raise ValueError("not buffers of v2p_two_hand_fix_buffers: %s" % sorted(unknown))
    for k, (dtype, count) in want.items():
        t = tensors.get(k)
        if not torch.is_tensor(t) or t.device != dev or not t.is_contiguous() or t.dtype != dtype or t.numel() != count:
            raise RuntimeError("two-hand fix: %s must be a contiguous %s tensor of %d elements on %s" % (k, str(dtype).replace("torch.", ""), count, dev))
    bind = tensors.get("bind")
    if not torch.is_tensor(bind) or bind.device != dev or not bind.is_contiguous() or bind.dtype != f32 or bind.dim() != 3 or tuple(bind.shape[1:]) != (24, 3) or bind.shape[0] < 1:
        raise RuntimeError("two-hand fix: bind must be a contiguous float32 tensor [R,24,3] on %s" % dev)
    if T == 0 or L == 0:
        return
    c = cfg_struct(st, num_iters, bind.shape[0])
    b = _lib.TwoHandFixBuffers(**{k: tensors[k].data_ptr() for k in _lib.TWO_HAND_FIX_BUFFER_NAMES})
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_two_hand_fix(C.byref(c), T, L, C.byref(b), _lib.current_stream(dev)), "v2p_two_hand_fix")


_BAKED = []


def baked_settings():
    """fix_settings(...) of the package's baked body model, made once"""
    if not _BAKED:
        from .model import load_baked_model

        m = load_baked_model()
        _BAKED.append(fix_settings(m.body_names, m.parents))
    return _BAKED[0]


def fix_two_hand_backhand(joint_rot, phase, swing_type, nframes, righthand, bind, num_iters=NUM_ITERS, settings=None, check=True):
    """The fix of T tracks in one launch.  settings: fix_settings(...) of the task's body model, None: the baked model's; device tensors joint_rot [T,L,24,3] float32, phase [T,L] float32,
    swing_type [T,L] int64, nframes [T] int32 (the frames of each track, at most L; what lies behind them is not read), righthand [T]
    int32 (non-zero: right-handed), bind [R,24,3] float32.  Returns a new [T,L,24,3] tensor - the reference works on a copy too: the
    fixed frames, every other frame copied, zeros behind nframes.  The launch waits for nothing; check (default) then reads the
    tracks' `overflow` - the one host read - and refuses a track above the cap of MAX_FRAMES flagged frames with the statement's
    message.  check=False returns (out, overflow [T] int32) instead: a track above the cap is copied whole, overflow[t] = its F."""
    if not torch.is_tensor(joint_rot) or not joint_rot.is_cuda:
        raise RuntimeError("two-hand fix: joint_rot must be a GPU tensor (there is no CPU path)")
    out = torch.zeros_like(joint_rot)
    overflow = torch.zeros(joint_rot.shape[0], dtype=torch.int32, device=joint_rot.device)
    launch_fix(baked_settings() if settings is None else settings, dict(joint_rot=joint_rot, phase=phase, swing_type=swing_type, nframes=nframes, righthand=righthand, bind=bind, out=out, overflow=overflow), num_iters)
    if not check:
        return out, overflow
    check_frames(int(overflow.max().item()) if overflow.numel() else 0)
    return out


def bind_rows_of(target):
    """The reference's `_smpl.joint_pos_bind`, a row per env, of an `ImitationTarget`: [N,24,3], or [1,24,3] for one body shape."""
    ids = target._env_shape_id
    return target._joint_pos_bind[:1].contiguous() if ids is None else target._joint_pos_bind[ids.long()].contiguous()


def skips_fix(player):
    """the reference's rule (mvae_controller_vis_dual.py:224): a side whose player name starts with `federer` is left as it is"""
    return str(player).startswith("federer")
