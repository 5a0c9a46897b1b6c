"""The imitation target from the motion generator's pose (vid2player/env/tasks/humanoid_smpl_im_mvae.py).

What turns the kinematic pose the MotionVAE generator writes every control step (`MotionVAEPlayer._root_pos`, `_joint_rotmat`) into the
target the low-level policy's humanoid tracks: `post_mvae_step` / `_set_target_motion_state` with the `fix_head_orientation` rule
(:593-661), `_smpl_to_sim` / `_forward_kinematics` (:897-946), the pose reset of `_reset_actors` / `_set_env_state` (:463-501) and
`_action_to_pd_targets` (:693-709).  One control step is ONE kernel launch, `v2p_mvae_target_step` (csrc/mvae_target.hip), plus the
existing `v2p_obs_imitation` for the [N,734] observation; the reset of a list of envs is `v2p_mvae_target_reset`, the PD-target actions
are `v2p_mvae_target_actions`.  The engine's target buffers belong to the task: the step kernel overwrites the row the engine sampled
from the env's clip, and zeroes the wrapped imitation task's own clip clock, progress and reset flag so that they neither end an episode
the controller owns nor mask its actions.

`smpl_to_sim_reference`, `target_step_reference`, `target_reset_reference` and `target_actions_reference` are the numpy statement of
the same calls on arrays - the checker of the tests, as `mvae.mvae_step_reference` is for the generator; the product never calls them.
There is no CPU path: a CPU device or a missing library is a RuntimeError.

A two-player task (`dual_mode: different`, env i is player i % 2) takes joint_pos_bind [2,24,3] - the task's `_env_shape_ids` are the
parities - and `smpl_beta` as a list of two; `pd_action_scale` / `pd_action_offset` stay one [69] pair for the batch, as in the reference.
Not built: per-clip body shapes x two players (refused by the task), `obs_type: joint_pos`, `update_mvae_from_sim` (`optimize_two_hand_backhand` with single=True is two_hand_fix.py); `pd_action_scale` / `pd_action_offset`
are the caller's arrays (the reference derives them from the actors' DoF limits, humanoid_smpl.py:368-410).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .ref_rotations import angle_axis_to_rotmat_reference, rotmat_to_angle_axis_reference, rotmat_to_quat_reference
from .body_shapes import SMPL_JOINT_NAMES

NUM_JOINTS = 24
NUM_DOF = _lib.NUM_DOF
ROW = _lib.MOTION_STATE_DIM
NUM_OBS_IM = 734
# the packed row (csrc/v2p_internal.hpp MS_*; `HumanoidSMPLIM._SLICES` is the task's view of the same row)
SLICES = {"root_pos": (0, 3), "root_rot": (3, 7), "dof_pos": (7, 76), "root_vel": (76, 79), "root_ang_vel": (79, 82), "dof_vel": (82, 151), "key_pos": (151, 163),
          "rb_pos": (163, 235), "rb_rot": (235, 331)}
PD_TARGET_BASES = _lib.PD_TARGET_BASES


def tree_from_model(body_names, parents):
    """(smpl_parents [24], smpl_of_body [24]) of a body model whose 24 bodies carry the SMPL joint names: the SMPL tree in SMPL joint
    order, and `_smpl_2_mujoco` (:218-237) - body b of the engine is SMPL joint smpl_of_body[b]."""
    names = list(body_names)
    if len(names) != NUM_JOINTS or sorted(names) != sorted(SMPL_JOINT_NAMES):
        raise ValueError("the imitation target needs a body model with the 24 SMPL joint names")
    smpl_of_body = [SMPL_JOINT_NAMES.index(nm) for nm in names]
    body_of_smpl = [names.index(nm) for nm in SMPL_JOINT_NAMES]
    par = [int(p) for p in parents]
    smpl_parents = [-1 if par[b] < 0 else smpl_of_body[par[b]] for b in body_of_smpl]
    return smpl_parents, smpl_of_body


def target_settings(cfg_v2p, cfg_env, control_dt, body_names, parents, key_body_ids, two_player=False):
    """What both the kernel's v2p_mvae_target_cfg and the numpy statement are made from.  cfg_v2p: the reference's `fix_head_orientation`,
    `add_residual_root`, `residual_root_scale` (and `dual_mode`: 'different' goes with a two-player task, two_player, and is refused
    without one); cfg_env: `pd_target_base`, `no_scale_action` (and `obs_type`)."""
    v2p, env = dict(cfg_v2p or {}), dict(cfg_env or {})
    # (`True`: both sides of a pair share one tree and one body - the single target; 'different': the kernels take a shape per env)
    if v2p.get("dual_mode") and v2p["dual_mode"] is not True and not (v2p["dual_mode"] == "different" and two_player):
        raise NotImplementedError("ImitationTarget: dual_mode %r is not built over a single-player task ('different' takes a two-player one)" % (v2p["dual_mode"],))
    if two_player and v2p.get("dual_mode") != "different":
        raise ValueError("ImitationTarget: a two-player task goes with cfg v2p.dual_mode 'different', got %r" % (v2p.get("dual_mode"),))
    if env.get("obs_type", "joint_pos_and_angle") != "joint_pos_and_angle":
        raise NotImplementedError("ImitationTarget: obs_type %r is not built (only joint_pos_and_angle)" % (env.get("obs_type"),))
    base = env.get("pd_target_base", "target_pos")
    if base not in PD_TARGET_BASES:
        raise ValueError("ImitationTarget: pd_target_base %r is none of %s" % (base, sorted(PD_TARGET_BASES)))
    keys = [int(k) for k in key_body_ids]
    if len(keys) != 4:
        raise ValueError("ImitationTarget: four key bodies are needed, got %d" % len(keys))
    smpl_parents, smpl_of_body = tree_from_model(body_names, parents)
    return dict(control_dt=float(control_dt), fix_head_orientation=bool(v2p.get("fix_head_orientation", False)), head_body=list(body_names).index("Head"),
                smpl_head=SMPL_JOINT_NAMES.index("Head"), smpl_neck=SMPL_JOINT_NAMES.index("Neck"), key_bodies=keys, smpl_parents=smpl_parents,
                smpl_of_body=smpl_of_body, pd_target_base=base, no_scale_action=bool(env.get("no_scale_action", False)),
                add_residual_root=bool(v2p.get("add_residual_root", False)), residual_root_scale=float(v2p.get("residual_root_scale", 0.02)))


def cfg_struct(st, num_shapes=1):
    c = _lib.MvaeTargetCfg(dt=st["control_dt"], fix_head_orientation=int(st["fix_head_orientation"]), head_body=st["head_body"], smpl_head=st["smpl_head"],
                           smpl_neck=st["smpl_neck"], num_shapes=int(num_shapes), pd_target_base=PD_TARGET_BASES[st["pd_target_base"]],
                           no_scale_action=int(st["no_scale_action"]))
    c.key_bodies[:] = st["key_bodies"]
    c.smpl_parents[:] = st["smpl_parents"]
    c.smpl_of_body[:] = st["smpl_of_body"]
    return c


def buffers_struct(tensors):
    """v2p_mvae_target_buffers of a dict name -> device tensor (names of _lib.MVAE_TARGET_BUFFER_NAMES; absent or None = NULL)."""
    unknown = set(tensors) - set(_lib.MVAE_TARGET_BUFFER_NAMES)
    if unknown:
        raise ValueError("not buffers of v2p_mvae_target_buffers: %s" % sorted(unknown))
    for k, t in tensors.items():
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise RuntimeError("imitation target: buffer %s must be a contiguous GPU tensor (there is no CPU path)" % k)
    return _lib.MvaeTargetBuffers(**{k: t.data_ptr() for k, t in tensors.items() if t is not None})


def launch_step(st, tensors, n, num_shapes=1):
    dev = tensors["target"].device
    c, b = cfg_struct(st, num_shapes), buffers_struct(tensors)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_mvae_target_step(C.byref(c), int(n), C.byref(b), _lib.current_stream(dev)), "v2p_mvae_target_step")


def launch_reset(st, tensors, num_envs, env_ids, num_shapes=1):
    dev = tensors["target"].device
    c, b = cfg_struct(st, num_shapes), buffers_struct(tensors)
    ids = env_ids.to(device=dev, dtype=torch.long).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_mvae_target_reset(C.byref(c), int(num_envs), C.byref(b), _lib.ptr(ids), int(ids.numel()), _lib.current_stream(dev)),
                   "v2p_mvae_target_reset")


def launch_reset_flagged(st, tensors, num_envs, flags, num_shapes=1):
    """v2p_mvae_target_reset_flagged: the reset of the envs whose flag ([num_envs] int64, non-zero) is up, one launch over all envs."""
    dev = tensors["target"].device
    if flags.dtype != torch.int64 or flags.device != dev or not flags.is_contiguous() or flags.numel() != int(num_envs):
        raise RuntimeError("imitation target: flags must be a contiguous int64 tensor [%d] on %s" % (num_envs, dev))
    c, b = cfg_struct(st, num_shapes), buffers_struct(tensors)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_mvae_target_reset_flagged(C.byref(c), int(num_envs), C.byref(b), _lib.ptr(flags), _lib.current_stream(dev)),
                   "v2p_mvae_target_reset_flagged")


def launch_actions(st, tensors, n, actions_in, actions_out, num_shapes=1):
    dev = actions_in.device
    c, b = cfg_struct(st, num_shapes), buffers_struct(tensors)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_mvae_target_actions(C.byref(c), int(n), _lib.ptr(actions_in), C.byref(b), _lib.ptr(actions_out), _lib.current_stream(dev)),
                   "v2p_mvae_target_actions")


# ------------------------------------------------------------------------------------------------------------------ the checker
def _probe(probes, key, v):
    if probes is not None:
        probes.setdefault(key, []).append(np.asarray(v, dtype=np.float64).ravel())


def _chain(rotmat, bind, parents, dt):
    """batch_rigid_transform (utils/hybrik.py:598-652): (posed joints [n,24,3], global matrices [n,24,3,3]), the parent first in every
    product, sums in the order of the matrix product's k."""
    rel = bind.copy()
    for i in range(1, NUM_JOINTS):
        rel[:, i] = bind[:, i] - bind[:, parents[i]]
    R, p = [rotmat[:, 0]], [rel[:, 0]]
    for i in range(1, NUM_JOINTS):
        P, pp, m, t = R[parents[i]], p[parents[i]], rotmat[:, i], rel[:, i]
        R.append(P[:, :, 0:1] * m[:, None, 0, :] + P[:, :, 1:2] * m[:, None, 1, :] + P[:, :, 2:3] * m[:, None, 2, :])
        p.append(P[:, :, 0] * t[:, 0:1] + P[:, :, 1] * t[:, 1:2] + P[:, :, 2] * t[:, 2:3] + pp)
    return np.stack(p, 1).astype(dt), np.stack(R, 1).astype(dt)


def _quat_diff_velocity(prev, cur, step, dt, probes):
    """quat_mul_norm(quat_inverse(prev), cur) -> quat_to_angle_axis -> axis * angle / step (utils/torch_utils.py:14-103), (x, y, z, w)."""
    x1, y1, z1, w1 = -prev[..., 0], -prev[..., 1], -prev[..., 2], prev[..., 3]
    x2, y2, z2, w2 = cur[..., 0], cur[..., 1], cur[..., 2], cur[..., 3]
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = dt(0.5) * (xx + (z1 - x1) * (x2 - y2))
    w = qq - ww + (z1 - y1) * (y2 - z2)
    x = qq - xx + (x1 + w1) * (x2 + w2)
    y = qq - yy + (w1 - x1) * (y2 + z2)
    z = qq - zz + (z1 + y1) * (w2 - x2)
    q = np.stack([x, y, z, w], -1)
    q = (dt(1) - dt(2) * (q[..., 3:] < 0).astype(dt)) * q
    q = q / np.maximum(np.sqrt((q * q).sum(-1)), dt(1e-9))[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        sin_theta = np.sqrt(dt(1) - q[..., 3] * q[..., 3])
        angle = dt(2) * np.arccos(q[..., 3])
        angle = np.arctan2(np.sin(angle), np.cos(angle))
        axis = q[..., :3] / sin_theta[..., None]
        mask = np.abs(sin_theta) > dt(1e-5)
    _probe(probes, "sin_theta", np.where(np.isnan(sin_theta), 0.0, sin_theta))
    angle = np.where(mask, angle, dt(0))
    axis = np.where(mask[..., None], axis, np.array([0, 0, 1], dt))
    return (axis * angle[..., None] / step).astype(dt)


def smpl_to_sim_reference(st, root_pos, joint_rotmat, bind, prev_root_pos=None, prev_rb_rot=None, dt=np.float32, probes=None):
    """`_smpl_to_sim` (:897-926) with `_forward_kinematics` (:928-946) on arrays: root_pos [n,3], joint_rotmat [n,24,3,3] (SMPL order),
    bind [n,24,3] (every env's row of joint_pos_bind).  Returns a dict root_pos, root_rot, dof_pos, root_vel, root_ang_vel, dof_vel,
    rb_pos, rb_rot in the engine's body order.  dt = numpy.float64 evaluates the same statement in double precision."""
    root_pos, joint_rotmat, bind = np.asarray(root_pos, dtype=dt), np.asarray(joint_rotmat, dtype=dt), np.asarray(bind, dtype=dt)
    n, order, step = len(root_pos), list(st["smpl_of_body"]), dt(st["control_dt"])
    local = probes.setdefault("local", {}) if probes is not None else None
    glob = probes.setdefault("global", {}) if probes is not None else None
    dof_pos = rotmat_to_angle_axis_reference(joint_rotmat, dt, local)[:, order][:, 1:].reshape(n, NUM_DOF)
    posed, rot = _chain(joint_rotmat, bind, st["smpl_parents"], dt)
    q = rotmat_to_quat_reference(rot, dt, glob)
    rb_rot = q[..., [1, 2, 3, 0]][:, order]
    rb_pos = posed[:, order] - (bind[:, :1] - root_pos[:, None])
    o = dict(root_pos=root_pos.copy(), root_rot=rb_rot[:, 0].copy(), dof_pos=dof_pos, rb_pos=rb_pos, rb_rot=rb_rot)
    if prev_root_pos is not None:
        o["root_vel"] = (root_pos - np.asarray(prev_root_pos, dtype=dt)) / step
        v = _quat_diff_velocity(np.asarray(prev_rb_rot, dtype=dt).reshape(n, NUM_JOINTS, 4), rb_rot, step, dt, probes)
        o["root_ang_vel"] = v[:, 0] / step  # (divided by dt once more, as the reference has it, :919)
        o["dof_vel"] = v[:, 1:].reshape(n, NUM_DOF)
    else:
        o["root_vel"], o["root_ang_vel"], o["dof_vel"] = np.zeros((n, 3), dt), np.zeros((n, 3), dt), np.zeros((n, NUM_DOF), dt)
    return {k: v.astype(dt) for k, v in o.items()}


def pack_row(st, o, dt=np.float32):
    """The packed row [n,331] of a `_smpl_to_sim` result; key_pos is rb_pos of the key bodies."""
    n = len(o["root_pos"])
    row = np.zeros((n, ROW), dt)
    for k, (a, b) in SLICES.items():
        row[:, a:b] = (o["rb_pos"][:, st["key_bodies"]] if k == "key_pos" else o[k]).reshape(n, b - a)
    return row


def unpack_row(row):
    return {k: np.asarray(row)[:, a:b] for k, (a, b) in SLICES.items()}


def _normalize2(v, dt):
    return v / np.maximum(np.sqrt((v * v).sum(-1)), dt(1e-12))[..., None]


def _bind_rows(s, n, dt):
    bind = np.asarray(s["joint_pos_bind"], dtype=dt).reshape(-1, NUM_JOINTS, 3)
    ids = np.zeros(n, np.int64) if s.get("env_shape_id") is None else np.asarray(s["env_shape_id"], dtype=np.int64)
    return bind[ids]


def target_step_reference(st, s, dt=np.float32, probes=None):
    """`_set_target_motion_state` (:600-661) on arrays.  st: target_settings(...); s: root_pos [n,3], joint_rotmat [n,24,3,3],
    residual_root [n,3] or None (already scaled), ball_pos [n,3], sim_root_pos [n,3] (the simulated root, body 0 of rb_state),
    joint_pos_bind [S,24,3], env_shape_id [n] or None, prev_target [n,331].  Returns dict(target [n,331], joint_rotmat) and the row's
    pieces by name; nothing in `s` is modified.  `probes` (a dict) receives the floats that are compared with a threshold."""
    root = np.asarray(s["root_pos"], dtype=dt).copy()
    n = len(root)
    if s.get("residual_root") is not None:
        root = root + np.asarray(s["residual_root"], dtype=dt)
    rotmat = np.asarray(s["joint_rotmat"], dtype=dt).reshape(n, NUM_JOINTS, 3, 3).copy()
    bind = _bind_rows(s, n, dt)
    prev = unpack_row(np.asarray(s["prev_target"], dtype=dt))
    if st["fix_head_orientation"]:
        first = smpl_to_sim_reference(st, root, rotmat, bind, dt=dt)
        hq = first["rb_rot"][:, st["head_body"]]
        w, x, y, z = hq[:, 3], hq[:, 0], hq[:, 1], hq[:, 2]
        qn = np.maximum(np.sqrt(w * w + x * x + y * y + z * z), dt(1e-12))
        w, x, y, z = w / qn, x / qn, y / qn, z / qn
        tx, ty, tz = dt(2) * x, dt(2) * y, dt(2) * z
        lookat = _normalize2(np.stack([tz * x + ty * w, tz * y - tx * w], -1), dt)
        ball, sim_root = np.asarray(s["ball_pos"], dtype=dt), np.asarray(s["sim_root_pos"], dtype=dt)
        head_ball = _normalize2(ball[:, :2] - first["rb_pos"][:, st["head_body"], :2], dt)
        diff = np.arctan2(head_ball[:, 1], head_ball[:, 0]) - np.arctan2(lookat[:, 1], lookat[:, 0])
        _probe(probes, "angle_diff", diff)
        pi = dt(np.float32(math.pi)) if dt is np.float32 else dt(math.pi)
        diff = np.where(diff > pi, diff - dt(2) * pi, diff)
        diff = np.where(diff < -pi, diff + dt(2) * pi, diff)
        _probe(probes, "miss_y", ball[:, 1] - (sim_root[:, 1] - dt(0.5)))
        _probe(probes, "miss_x", np.abs(ball[:, 0]) - dt(4))
        miss = (ball[:, 1] < sim_root[:, 1] - dt(0.5)) | (np.abs(ball[:, 0]) > dt(4))
        diff = np.where(miss, dt(0), diff).astype(dt)
        joints = [st["smpl_head"], st["smpl_neck"]]
        aa = rotmat_to_angle_axis_reference(rotmat[:, joints], dt, probes.setdefault("local", {}) if probes is not None else None)
        aa[:, 0, 1] += diff / dt(2)
        aa[:, 1, 1] += diff / dt(2)
        rotmat[:, joints] = angle_axis_to_rotmat_reference(aa, dt)
        if probes is not None:
            probes["angle_diff_applied"] = diff.astype(np.float64)
    o = smpl_to_sim_reference(st, root, rotmat, bind, prev["root_pos"], prev["rb_rot"], dt, probes)
    o["key_pos"] = o["rb_pos"][:, st["key_bodies"]]
    o["target"] = pack_row(st, o, dt)
    o["joint_rotmat"] = rotmat
    return o


def target_reset_reference(st, s, env_ids, dt=np.float32, probes=None):
    """`_reset_actors` + `_set_env_state` (:463-501) on arrays for env_ids (ids outside the batch are skipped).  s: root_pos, joint_rotmat,
    joint_pos_bind, env_shape_id, and the arrays that receive rows: target [N,331], root_states [N,13], dof_state [N,69,2], rb_state
    [N,24,13] (each may be absent).  Returns copies of those with the ids' rows written."""
    N = len(s["root_pos"])
    ids = np.asarray(env_ids, dtype=np.int64)
    ids = ids[(ids >= 0) & (ids < N)]
    out = {k: np.array(s[k], dtype=dt) for k in ("target", "root_states", "dof_state", "rb_state") if s.get(k) is not None}
    if len(ids) == 0:
        return out
    bind = _bind_rows(s, N, dt)[ids]
    o = smpl_to_sim_reference(st, np.asarray(s["root_pos"], dtype=dt)[ids], np.asarray(s["joint_rotmat"], dtype=dt).reshape(N, NUM_JOINTS, 3, 3)[ids], bind, dt=dt,
                              probes=probes)
    if "target" in out:
        out["target"][ids] = pack_row(st, o, dt)
    if "root_states" in out:
        out["root_states"][ids] = np.concatenate([o["root_pos"], o["root_rot"], np.zeros((len(ids), 6), dt)], 1)
    if "dof_state" in out:
        out["dof_state"] = out["dof_state"].reshape(N, NUM_DOF, 2)
        out["dof_state"][ids] = np.stack([o["dof_pos"], np.zeros_like(o["dof_pos"])], -1)
    if "rb_state" in out:
        out["rb_state"] = out["rb_state"].reshape(N, NUM_JOINTS, 13)
        out["rb_state"][ids] = np.concatenate([o["rb_pos"], o["rb_rot"], np.zeros((len(ids), NUM_JOINTS, 6), dt)], -1)
    return out


def target_reset_flagged_reference(st, s, flags, dt=np.float32, probes=None):
    """`v2p_mvae_target_reset_flagged` on arrays: target_reset_reference over the envs whose flag is not 0."""
    return target_reset_reference(st, s, np.flatnonzero(np.asarray(flags)), dt, probes)


def target_actions_reference(st, actions, target=None, dof_state=None, pd_action_scale=None, pd_action_offset=None, dt=np.float32, probes=None):
    """`_action_to_pd_targets` (:693-703) before its clamp: [n,75] -> [n,75], columns 69.. copied."""
    a = np.asarray(actions, dtype=dt)
    n = len(a)
    base = {"target_pos": lambda: np.asarray(target, dtype=dt)[:, SLICES["dof_pos"][0]:SLICES["dof_pos"][1]],
            "current_pos": lambda: np.asarray(dof_state, dtype=dt).reshape(n, NUM_DOF, 2)[..., 0],
            "none": lambda: np.broadcast_to(np.asarray(pd_action_offset, dtype=dt), (n, NUM_DOF))}[st["pd_target_base"]]()
    out = a.copy()
    out[:, :NUM_DOF] = base + a[:, :NUM_DOF] if st["no_scale_action"] else base + np.asarray(pd_action_scale, dtype=dt) * a[:, :NUM_DOF]
    return out.astype(dt)


# ------------------------------------------------------------------------------------------------------------------ the object
class ImitationTarget:
    """The target half of `HumanoidSMPLIMMVAE` on the device, around a racket + ball task and the motion generator of its batch.
    task: a `HumanoidSMPLIMRacketBall`; player: its `MotionVAEPlayer`; joint_pos_bind [S,24,3] (or [24,3]): rest joints of the SMPL
    bodies (`self._smpl.joint_pos_bind`, one row per body shape; the task's `_env_shape_ids` pick an env's row); cfg: {"v2p": ..., "env": ...}
    with the keys of `target_settings`, and optionally env `pd_action_scale` / `pd_action_offset` [69], v2p `smpl_beta` [10].  Over a
    two-player task (`racket_players`): a player with `dual_mode: 'different'`, joint_pos_bind [2,24,3] (side 0, side 1), `smpl_beta` [2,10]."""

    def __init__(self, task, player, joint_pos_bind, cfg):
        v2p, env = dict(cfg.get("v2p") or {}), dict(cfg.get("env") or {})
        dev = torch.device(task.device)
        if dev.type != "cuda":
            raise RuntimeError("ImitationTarget: the target is written by a HIP kernel - the task must live on a GPU (no CPU fallback)")
        two_player = getattr(task, "racket_players", None) is not None
        if two_player != bool(getattr(player, "_is_dual", False)):
            raise ValueError("ImitationTarget: a two-player task takes a motion generator with dual_mode 'different', a single-player task one without")
        if not hasattr(task, "_ball_root_states"):
            raise TypeError("ImitationTarget wraps a HumanoidSMPLIMRacketBall")
        if abs(float(task.pd_tar_lim) - math.pi / 2) > 1e-6:
            raise ValueError("ImitationTarget: the task's pd_tar_lim must be pi/2 - the engine's clamp is the reference's (humanoid_smpl_im_mvae.py:705-707)")
        if player.num_envs != task.num_envs or torch.device(player.device) != dev:
            raise ValueError("ImitationTarget: the player has %d envs on %s, the task %d on %s" % (player.num_envs, player.device, task.num_envs, dev))
        _lib.load()
        self.task, self.player, self.device, self.num_envs = task, player, dev, task.num_envs
        self.settings = target_settings(v2p, env, task.dt, task.body_names, task.body_model.parents, task._key_body_ids.tolist(), two_player)
        f = dict(dtype=torch.float32, device=dev)
        bind = torch.as_tensor(np.asarray(joint_pos_bind, dtype=np.float32)).to(**f).reshape(-1, NUM_JOINTS, 3).contiguous()
        shape_ids = getattr(task, "_env_shape_ids", None)
        self._env_shape_id = None if shape_ids is None else torch.as_tensor(np.asarray(shape_ids), dtype=torch.int32, device=dev).contiguous()
        if self._env_shape_id is not None and int(self._env_shape_id.max()) >= len(bind):
            raise ValueError("ImitationTarget: joint_pos_bind has %d rows, the task's body shapes go up to %d" % (len(bind), int(self._env_shape_id.max())))
        self._joint_pos_bind = bind
        arr = lambda k: None if env.get(k) is None else torch.as_tensor(np.asarray(env[k], dtype=np.float32)).to(**f).reshape(NUM_DOF).contiguous()
        self._pd_action_scale, self._pd_action_offset = arr("pd_action_scale"), arr("pd_action_offset")
        if not self.settings["no_scale_action"] and self._pd_action_scale is None:
            raise ValueError("ImitationTarget: cfg env.pd_action_scale [69] is required unless no_scale_action")
        if self.settings["pd_target_base"] == "none" and self._pd_action_offset is None:
            raise ValueError("ImitationTarget: cfg env.pd_action_offset [69] is required with pd_target_base 'none'")
        # `_reset_ref_motion_bodies` (:257-264): gender male, then the player's betas
        self._reset_ref_motion_bodies = torch.zeros((self.num_envs, 11), **f)
        self._reset_ref_motion_bodies[:, 0] = 1
        if v2p.get("smpl_beta") is not None and two_player:  # (:260-262: the betas of side 0 and of side 1)
            betas = torch.as_tensor(np.asarray(v2p["smpl_beta"], dtype=np.float32), **f)
            if betas.shape != (2, 10):
                raise ValueError("ImitationTarget: with a two-player task cfg v2p.smpl_beta is a list of two [10], got shape %s" % (tuple(betas.shape),))
            self._reset_ref_motion_bodies[0::2, 1:11], self._reset_ref_motion_bodies[1::2, 1:11] = betas[0], betas[1]
        elif v2p.get("smpl_beta") is not None:
            self._reset_ref_motion_bodies[:, 1:11] = torch.as_tensor(np.asarray(v2p["smpl_beta"], dtype=np.float32).reshape(10), **f)
        self.obs_buf = torch.zeros((self.num_envs, NUM_OBS_IM), **f)
        self._pd_actions = torch.zeros((self.num_envs, _lib.NUM_ACTIONS), **f)

    def _tensors(self, target, prev_target=None):
        t = self.task
        return dict(root_pos=self.player._root_pos, joint_rotmat=self.player._joint_rotmat, ball_state=t._ball_root_states, joint_pos_bind=self._joint_pos_bind,
                    env_shape_id=self._env_shape_id, target=target, prev_target=prev_target, root_states=t._humanoid_root_states, dof_state=t._dof_state,
                    rb_state=t._rigid_body_state, pd_action_scale=self._pd_action_scale, pd_action_offset=self._pd_action_offset)

    def step(self, residual_root=None):
        """`_set_target_motion_state`: `task._target_*` from the player's pose and `task._prev_target_*`; one launch."""
        t = self.task
        tensors = self._tensors(t._target_bufs[t._cur], t._target_bufs[1 - t._cur])
        if residual_root is not None:
            if not self.settings["add_residual_root"]:
                raise RuntimeError("ImitationTarget.step: a residual root needs cfg v2p.add_residual_root")
            if residual_root.shape != (self.num_envs, 3):
                raise RuntimeError("ImitationTarget.step: residual_root must be [%d, 3]" % self.num_envs)
            tensors["residual_root"] = residual_root.to(device=self.device, dtype=torch.float32).contiguous()
        tensors.update(hold_reset=t.reset_buf, hold_progress=t.progress_buf, hold_cur_time=t._cur_ref_motion_times)
        launch_step(self.settings, tensors, self.num_envs, len(self._joint_pos_bind))

    def reset(self, env_ids):
        """`_reset_actors` + `_set_env_state` + `_reset_env_tensors` for env_ids: the generator's pose becomes the previous target and the
        humanoid's state, zero velocities."""
        ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long).contiguous()
        if ids.numel() == 0:
            return
        t = self.task
        launch_reset(self.settings, self._tensors(t._target_bufs[1 - t._cur]), self.num_envs, ids, len(self._joint_pos_bind))
        t._reset_env_tensors(ids, with_rb_state=True)

    def reset_flagged(self, flags):
        """`reset(env_ids)` for the envs whose flag ([N] int64 on the device, non-zero = reset) is up: two launches over all envs
        (`v2p_mvae_target_reset_flagged`, `v2p_env_push_state_flagged`), no id list and no host read."""
        t = self.task
        launch_reset_flagged(self.settings, self._tensors(t._target_bufs[1 - t._cur]), self.num_envs, flags, len(self._joint_pos_bind))
        t._reset_env_tensors_flagged(flags, with_rb_state=True)

    def actions(self, a):
        """`_action_to_pd_targets` before its clamp (the engine's pre-physics clamps): [N,75] -> [N,75] (a buffer of this object)."""
        if a.dtype != torch.float32 or not a.is_cuda or not a.is_contiguous() or tuple(a.shape) != (self.num_envs, _lib.NUM_ACTIONS):
            raise RuntimeError("ImitationTarget.actions: actions must be a contiguous float32 GPU tensor [%d, %d]" % (self.num_envs, _lib.NUM_ACTIONS))
        t = self.task
        launch_actions(self.settings, self._tensors(t._target_bufs[t._cur]), self.num_envs, a, self._pd_actions, len(self._joint_pos_bind))
        return self._pd_actions

    def compute_observations(self):
        """`_compute_observations` (:862-895): the [N,734] imitation observation of the exposed state against the new target."""
        t, n = self.task, self.num_envs
        rb, ds = t._rigid_body_state.view(n, NUM_JOINTS, 13), t._dof_state.view(n, NUM_DOF, 2)
        row = t._target_bufs[t._cur]
        piece = lambda k: row[:, SLICES[k][0]:SLICES[k][1]]
        args = [rb[..., 0:3], rb[..., 3:7], piece("rb_pos"), piece("rb_rot"), ds[..., 0], ds[..., 1], piece("dof_pos"), rb[..., 7:10], rb[..., 10:13],
                self._reset_ref_motion_bodies]
        args = [x.contiguous() for x in args]
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().v2p_obs_imitation(n, *[_lib.ptr(x) for x in args], None, None, 0.0, _lib.ptr(self.obs_buf), _lib.current_stream(self.device)),
                       "v2p_obs_imitation")
        return self.obs_buf
