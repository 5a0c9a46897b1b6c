"""The MotionVAE motion generator on the device (vid2player/players/mvae_player.py `MVAEPlayer`, around the mixture-of-experts decoder
of vid2player/motion_vae/model.py:186-252).

One control step - the gate, the three expert-blended layers and the player's state update (`_update_mvae_state`) - is ONE kernel launch,
`v2p_mvae_step` (csrc/mvae_player.hip); `reset(env_ids)` is `v2p_mvae_reset`.  The decoder computes every expert and blends the results,
out = sum_e c_e (x W_e + b_e), which is the function the reference computes by blending the weights per env; fp32 throughout (the
reference runs the decoder under autocast on CUDA - a reduced-precision path is not built).  Only the shipped architecture
is built: frame 288, latent 32, hidden 256, 6 experts, gate 64, one condition frame, one prediction, predicted phase.  Both dual modes are
built: `True` (one generator for both sides, `reset_dual`) and `different` (a weight set, statistics, hand and player rule per side: env 2k
is side 0, env 2k+1 side 1; `v2p_mvae_dual_step` / `v2p_mvae_dual_reset`, csrc/mvae_player_dual.hip).
`reset_dual_flagged` resets the pairs whose flags are up in one launch over all envs, under either mode (`v2p_mvae_dual_reset_flagged`,
csrc/mvae_player_dual_flagged.hip; `v2p_mvae_reset_flagged` on the per-env table of serve and ready frames).

`mvae_step_reference` / `mvae_reset_reference` (and `mvae_dual_step_reference` / `mvae_dual_reset_reference`, which apply them row-wise
by parity) are the numpy statement of the same calls on arrays - the checker of the tests, as
`tennis_controller.task_step_reference` is for the task step; the product never calls them.  There is no CPU path: a CPU device or a
missing library is a RuntimeError.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .ref_rotations import angle_axis_to_rotmat_reference, rot6d_to_rotmat_reference, rotmat_to_angle_axis_reference

FRAME, LATENT, HIDDEN, EXPERTS, GATE = 288, 32, 256, 6, 64
OUT = FRAME + 2  # the feature and the two phase numbers
NUM_JOINTS = 24
COL_ROOT_VEL, COL_JOINT_POS, COL_ROT6D = 3, 6, 144  # mvae_player.py:77-90 with the full root position
PLAYERS = {"djokovic": 0, "federer": 1, "nadal": 2}
LELBOW, RELBOW, LWRIST, RWRIST = 18, 19, 20, 21  # utils/pose.py
RACKET_CHAIN = {True: (0, 3, 6, 9, 14, 17, 19, 21, 23), False: (0, 3, 6, 9, 13, 16, 18, 20, 22)}  # utils/racket.py:152-161
RACKET_LENGTHS = (0.2, 0.15, 0.15)  # handle, shaft, head radius of the eastern tennis racket (utils/racket.py:10-19)
RACKET_DIR = (-1.0, 0.0, 0.0)  # the canonical racket direction of both tennis grips
RACKET_NORMALS = {"eastern": (0.0, 1.0, 0.0), "semi_western": (0.0, 1.0 / math.sqrt(2), 1.0 / math.sqrt(2))}  # utils/racket.py:10-32, before F.normalize
STATE_NAMES = _lib.MVAE_BUFFER_NAMES
WEIGHT_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2", "gate_w0", "gate_b0", "gate_w1", "gate_b1", "gate_w2", "gate_b2")
# the residual-DoF rule (mvae_player.py:306-408).  A row: (swing type, lo, hi, lo inclusive, {base angle: value}); envs of that swing
# type whose phase lies in (lo, hi) get the base angles, rows applied in order.  "swings": the forehand and backhand windows outside of
# which a residual is zeroed when not training.  Angles in units of pi: elbow twist, wrist twist, wrist shake, wrist swing.
RESIDUAL_RULES = {
    "djokovic": dict(rows=((1, 2.0, 3.2, False, {"elbow": -0.75}), (1, 2.0, 3.1, False, {"swing": -0.25}), (1, 3.1, 3.2, True, {"swing": 0.25}),
                           (2, 2.0, 3.2, False, {"elbow": -0.25}), (2, 2.0, 3.0, False, {"swing": 0.1})), swings=((2.0, 3.2), (2.0, 3.2))),
    "federer": dict(rows=((1, 2.0, 3.2, False, {"elbow": -0.5}), (1, 2.0, 3.1, False, {"swing": -0.25}), (1, 3.1, 3.2, True, {"swing": 0.25}),
                          (2, 2.0, 3.5, False, {"twist": -0.25, "shake": 0.15}), (3, 2.0, 3.5, False, {"twist": -0.1}),
                          (0, 2.0, 3.3, False, {"twist": -0.5, "shake": 0.1, "elbow": -0.25}), (0, 2.0, 3.0, False, {"swing": -0.5})), swings=((2.0, 3.2), (2.0, 3.5))),
    "nadal": dict(rows=((1, 2.5, 3.2, False, {"elbow": -0.75, "swing": 0.25}), (2, 2.0, 3.5, False, {"twist": -0.4}), (2, 2.0, 3.0, False, {"swing": -0.25})),
                  swings=((2.5, 3.2), (2.0, 3.5))),
}


def player_settings(cfg, is_train, num_envs=None):
    """What both the kernel's v2p_mvae_cfg and the numpy statement are made from.  cfg: the reference's cfg_v2p keys `player`, `righthand`,
    `add_residual_dof` (and, refused when they ask for what is not built: `predict_phase`, the sizes of another option set).
    `dual_mode: True` (one generator for both sides of every pair) is the single player's generator with two sets of initial frames,
    `reset_dual`.  `dual_mode: 'different'` (mvae_player.py:23-57): `player`, `righthand` and `grip` are lists of two - side 0: envs 2k,
    side 1: envs 2k+1 - and `serve_from` ('near', the default, or 'far') picks the side whose hand and grip the batch's ONE racket object
    has; the result is dict(dual=True, sides=(settings of side 0, of side 1), racket=racket_settings(...), is_train, add_residual_dof)."""
    cfg = dict(cfg)
    if cfg.get("dual_mode") == "different":
        for k in ("player", "righthand") + (("grip",) if cfg.get("grip") is not None else ()):
            if not isinstance(cfg.get(k), (list, tuple)):  # (one value for both sides: the reference would index into it)
                raise NotImplementedError("MotionVAEPlayer: dual_mode 'different' takes cfg %s as a list of two (side 0, side 1); one value for both sides is not built; got %r" % (k, cfg.get(k)))
            if len(cfg[k]) != 2:
                raise ValueError("MotionVAEPlayer: dual_mode 'different' needs cfg %s as a list of two (side 0, side 1); got %r" % (k, cfg.get(k)))
        if num_envs is not None and int(num_envs) % 2:
            raise ValueError("MotionVAEPlayer: dual_mode 'different' needs an even num_envs (envs 2k and 2k+1 are a pair); got %d" % num_envs)
        residual = cfg.get("add_residual_dof")
        if isinstance(residual, (list, tuple)):
            if len(residual) != 2 or residual[0] != residual[1]:
                raise ValueError("MotionVAEPlayer: add_residual_dof must be common to both sides (one residual tensor serves the batch); got %r" % (residual,))
            residual = residual[0]
        one = {k: v for k, v in cfg.items() if k not in ("dual_mode", "grip", "serve_from")}
        sides = tuple(player_settings(dict(one, player=cfg["player"][i], righthand=cfg["righthand"][i], add_residual_dof=residual), is_train) for i in (0, 1))
        server = 0 if cfg.get("serve_from", "near") != "near" else 1  # (mvae_player.py:56)
        grip = cfg["grip"][server] if cfg.get("grip") is not None else None
        return dict(dual=True, sides=sides, racket=racket_settings(grip, sides[server]["righthand"]), is_train=bool(is_train), add_residual_dof=sides[0]["add_residual_dof"])
    if cfg.get("dual_mode") and cfg["dual_mode"] is not True:
        raise NotImplementedError("MotionVAEPlayer: dual_mode %r is not built (True or 'different')" % (cfg["dual_mode"],))
    if cfg.get("player") not in PLAYERS:
        raise ValueError("MotionVAEPlayer: cfg player %r is none of %s" % (cfg.get("player"), sorted(PLAYERS)))
    if cfg.get("add_residual_dof") not in (None, False, "euler"):
        raise ValueError("MotionVAEPlayer: add_residual_dof %r (only 'euler' exists)" % (cfg.get("add_residual_dof"),))
    sizes = dict(frame_size=FRAME, latent_size=LATENT, hidden_size=HIDDEN, num_experts=EXPERTS, gate_hidden_size=GATE, num_condition_frames=1,
                 num_future_predictions=1, predict_phase=True)
    for k, v in sizes.items():
        if cfg.get(k, v) != v:
            raise NotImplementedError("MotionVAEPlayer: only the shipped architecture is built (%s); got %s = %r" % (", ".join("%s %s" % kv for kv in sizes.items()), k, cfg[k]))
    return dict(player=cfg["player"], righthand=bool(cfg.get("righthand", True)), is_train=bool(is_train), add_residual_dof=bool(cfg.get("add_residual_dof")))


def racket_settings(grip, righthand):
    """`Racket('tennis', grip=grip, righthand=righthand)` (utils/racket.py:148-181) as what the reset reads: the arm of the FK chain and the
    canonical direction and normal, normalised in float32 by the reference's own expression."""
    if grip not in (None,) + tuple(RACKET_NORMALS):
        raise ValueError("MotionVAEPlayer: grip %r is none of %s" % (grip, sorted(RACKET_NORMALS)))
    unit = lambda v: tuple(float(x) for x in torch.nn.functional.normalize(torch.tensor(v, dtype=torch.float32), dim=0))
    return dict(grip=grip or "eastern", righthand=bool(righthand), direction=unit(RACKET_DIR), normal=unit(RACKET_NORMALS[grip or "eastern"]))


def racket_struct(r):
    return _lib.MvaeRacket(righthand=int(r["righthand"]), dir=(C.c_float * 3)(*r["direction"]), normal=(C.c_float * 3)(*r["normal"]))


def cfg_struct(st):
    return _lib.MvaeCfg(frame_size=FRAME, latent_size=LATENT, hidden_size=HIDDEN, num_experts=EXPERTS, gate_hidden_size=GATE, num_condition_frames=1,
                        num_future_predictions=1, predict_phase=1, player=PLAYERS[st["player"]], righthand=int(st["righthand"]), is_train=int(st["is_train"]),
                        add_residual_dof=int(st["add_residual_dof"]))


# ------------------------------------------------------------------------------------------------------------------ weights
def weights_from_state_dict(sd):
    """The decoder's arrays out of a `PoseMixtureVAE` state dict (a mapping of names to tensors or arrays; no pickle of reference classes
    is read): decoder.w0..w2 [6,K,N], decoder.b0..b2 [6,N], decoder.gate.{0,2,4}.{weight,bias}.  Returns a dict of float32 arrays under the
    names of v2p_mvae_weights, in the reference's layouts."""
    def get(k):
        if k not in sd:
            raise KeyError("weights_from_state_dict: the state dict has no %r" % k)
        v = sd[k]
        return np.ascontiguousarray((v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)), dtype=np.float32)

    w = {}
    shapes = {"w0": (EXPERTS, LATENT + FRAME, HIDDEN), "w1": (EXPERTS, LATENT + HIDDEN, HIDDEN), "w2": (EXPERTS, LATENT + HIDDEN, OUT), "b0": (EXPERTS, HIDDEN),
              "b1": (EXPERTS, HIDDEN), "b2": (EXPERTS, OUT), "gate_w0": (GATE, LATENT + FRAME), "gate_b0": (GATE,), "gate_w1": (GATE, GATE), "gate_b1": (GATE,),
              "gate_w2": (EXPERTS, GATE), "gate_b2": (EXPERTS,)}
    for i in range(3):
        w["w%d" % i], w["b%d" % i] = get("decoder.w%d" % i), get("decoder.b%d" % i)
        w["gate_w%d" % i], w["gate_b%d" % i] = get("decoder.gate.%d.weight" % (2 * i)), get("decoder.gate.%d.bias" % (2 * i))
    for k, shape in shapes.items():
        if w[k].shape != shape:
            raise ValueError("weights_from_state_dict: %s has shape %s, the shipped architecture needs %s" % (k, w[k].shape, shape))
    return w


def pack_matrix(W):
    """A stack W[E,K,N] (y = x W) in the layout the kernel reads (v2p_rollout.h, v2p_mvae_weights): [E, ceil(N/32), K/8, 64, 4]."""
    W = np.asarray(W, dtype=np.float32)
    E, K, N = W.shape
    T = (N + 31) // 32
    P = np.zeros((E, K, T * 32), np.float32)
    P[:, :, :N] = W
    # k = 8g + 2q + h, column = 32t + c, lane = 32h + c  ->  [e, t, g, h, c, q]
    P = P.reshape(E, K // 8, 4, 2, T, 32).transpose(0, 4, 1, 3, 5, 2)
    return np.ascontiguousarray(P).reshape(E, T, K // 8, 64, 4)


def pack_bias(b):
    b = np.atleast_2d(np.asarray(b, dtype=np.float32))
    out = np.zeros((b.shape[0], (b.shape[1] + 31) // 32 * 32), np.float32)
    out[:, :b.shape[1]] = b
    return out


def pack_weights(w, avg, std, device):
    """Device tensors under the names of v2p_mvae_weights, made once at load time."""
    t = {}
    for i in range(3):
        t["w%d" % i], t["b%d" % i] = pack_matrix(w["w%d" % i]), pack_bias(w["b%d" % i])
        t["gate_w%d" % i], t["gate_b%d" % i] = pack_matrix(np.asarray(w["gate_w%d" % i], dtype=np.float32).T[None]), pack_bias(w["gate_b%d" % i])
    t["avg"], t["std"] = np.asarray(avg, dtype=np.float32).reshape(FRAME), np.asarray(std, dtype=np.float32).reshape(FRAME)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device).contiguous() for k, v in t.items()}


# ------------------------------------------------------------------------------------------------------------------ the checker
def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def decoder_reference(w, z, c, dt=np.float32, probes=None):
    """`MixedDecoder.forward(z, c)` in the form the kernel computes: every expert, then the blend.  Returns [n, 290]."""
    A = lambda k: np.asarray(w[k], dtype=dt)
    z, c = np.asarray(z, dtype=dt), np.asarray(c, dtype=dt)
    x = np.concatenate([z, c], 1)
    g = _elu(x @ A("gate_w0").T + A("gate_b0"))
    g = _elu(g @ A("gate_w1").T + A("gate_b1"))
    g = g @ A("gate_w2").T + A("gate_b2")
    ex = np.exp(g - g.max(1, keepdims=True))
    coef = ex / ex.sum(1, keepdims=True)
    h = c
    for i in range(3):
        x = np.concatenate([z, h], 1)
        W, b = A("w%d" % i), A("b%d" % i)
        y = np.zeros((len(x), W.shape[2]), dt)
        for e in range(EXPERTS):
            y = y + coef[:, e:e + 1] * (x @ W[e] + b[e])
        if probes is not None:
            probes["pre%d" % i] = y
        h = _elu(y) if i < 2 else y
    if probes is not None:
        probes["coef"] = coef
    return h.astype(dt)


def _residual_bases(st, phase, swing, dt):
    rule = RESIDUAL_RULES[st["player"]]
    base = {k: np.zeros(len(phase), dt) for k in ("elbow", "twist", "shake", "swing")}
    for s, lo, hi, ge, values in rule["rows"]:
        m = (swing == s) & ((phase >= dt(lo)) if ge else (phase > dt(lo))) & (phase < dt(hi))
        for k, v in values.items():
            base[k][m] = dt(v)
    (f0, f1), (b0, b1) = rule["swings"]
    swings = ((swing == 1) & (phase > dt(f0)) & (phase < dt(f1))) | ((swing == 2) & (phase > dt(b0)) & (phase < dt(b1)))
    return base, swings


def mvae_step_reference(st, w, avg, std, s, latents, residual=None, dt=np.float32, probes=None):
    """`MVAEPlayer.step(latents, residual)` on arrays: the decoder, then `_update_mvae_state(init=False)` (mvae_player.py:184-190, 221-223,
    254-422).  st: player_settings(...); s: the state before the step under the names of v2p_mvae_buffers.  Returns a dict with every
    array the step writes; nothing in `s` is modified.  dt = numpy.float64 evaluates the same statement in double precision; `probes`
    (a dict) receives the floats that are compared with a threshold."""
    avg, std = np.asarray(avg, dtype=dt).reshape(FRAME), np.asarray(std, dtype=dt).reshape(FRAME)
    n = len(latents)
    cond = np.asarray(s["conditions"], dtype=dt).reshape(n, FRAME)
    out = decoder_reference(w, latents, cond, dt, probes)
    norm, ph2 = out[:, :FRAME], out[:, FRAME:]
    feat = norm * std + avg
    o = {}
    vel = feat[:, COL_ROOT_VEL:COL_ROOT_VEL + 3]
    root = np.asarray(s["root_pos"], dtype=dt) + vel
    cond = norm.copy()
    cond[:, :3] = (root - avg[:3]) / std[:3]
    r6 = feat[:, COL_ROT6D:].reshape(n, NUM_JOINTS, 6).copy()
    rotmat = rot6d_to_rotmat_reference(r6, dt, probes)
    phase = np.arctan2(ph2[:, 0], ph2[:, 1])
    if probes is not None:
        probes["atan2"] = phase.copy()
    phase = np.where(phase < 0, phase + dt(math.pi * 2), phase).astype(dt)
    swing, cycle = np.array(s["swing_type"], dtype=np.int64), np.array(s["swing_type_cycle"], dtype=np.int64)
    wrist_x = feat[:, COL_JOINT_POS + (RWRIST - 1) * 3]  # the RIGHT wrist, whatever the hand
    a, b = (1, 2) if st["righthand"] else (2, 1)
    swing = np.where((swing == -1) & (phase > dt(2.0)) & (phase < dt(3.5)), np.where(wrist_x > 0, a, b), swing)
    swing = np.where((swing != -1) & (phase > dt(3.5)), -1, swing)
    cycle = np.where(swing != -1, swing, cycle)
    if probes is not None:
        probes["phase"], probes["wrist_x"] = phase, wrist_x
    if residual is not None and len(residual):
        res = np.clip(np.asarray(residual, dtype=dt) * dt(0.25), dt(-0.25), dt(0.25))
        base, swings = _residual_bases(st, phase, swing, dt)
        if not st["is_train"]:
            res[~swings] = 0
        joints = [RELBOW, RWRIST] if st["righthand"] else [LELBOW, LWRIST]
        aa = rotmat_to_angle_axis_reference(rotmat[:, joints], dt, probes)
        pi = dt(math.pi)
        aa[:, 0, 0] = (base["elbow"] + res[:, 0]) * pi
        aa[:, 1, 0] = base["twist"] * pi
        aa[:, 1, 1] = (base["shake"] + res[:, 1]) * pi
        aa[:, 1, 2] = (base["swing"] + res[:, 2]) * pi
        rotmat[:, joints] = angle_axis_to_rotmat_reference(aa, dt, probes)
        r6[:, joints] = np.concatenate([rotmat[:, joints][..., 0], rotmat[:, joints][..., 1]], -1)
    o.update(conditions=cond.reshape(n, 1, FRAME), root_pos=root, root_vel=vel.copy(), joint_rot6d=r6, joint_rotmat=rotmat, phase_pred=phase, swing_type=swing,
             swing_type_cycle=cycle)
    if not st["is_train"]:
        o["joint_rot"] = rotmat_to_angle_axis_reference(rot6d_to_rotmat_reference(r6, dt, probes), dt, probes)
    return {k: (v.astype(dt) if v.dtype.kind == "f" else v) for k, v in o.items()}


def mvae_reset_reference(st, avg, std, s, env_ids, init_feature, root_xy, joint_pos_bind_rel, dt=np.float32, probes=None, racket=None):
    """`MVAEPlayer.reset(env_ids)` on arrays (mvae_player.py:160-165, 212-252, 424-431): returns the whole state after the reset, rows of
    ids outside the batch untouched.  init_feature [len(env_ids), 288], root_xy [len(env_ids), 2] (the caller's draw).
    joint_pos_bind_rel [24,3], or [len(env_ids),24,3]: a row per id.  racket: racket_settings(...) of a player whose racket is not the
    eastern one of st's hand (the two-player batch)."""
    avg, std = np.asarray(avg, dtype=dt).reshape(FRAME), np.asarray(std, dtype=dt).reshape(FRAME)
    o = {k: np.array(s[k]) for k in STATE_NAMES if s.get(k) is not None}
    n = len(o["root_pos"])
    o["conditions"] = o["conditions"].reshape(n, 1, FRAME)
    ids = np.asarray(env_ids, dtype=np.int64)
    keep = (ids >= 0) & (ids < n)
    bind = np.asarray(joint_pos_bind_rel, dtype=dt).reshape(-1, NUM_JOINTS, 3)
    bind = np.broadcast_to(bind, (len(ids), NUM_JOINTS, 3))[keep]
    ids, f, xy = ids[keep], np.asarray(init_feature, dtype=dt)[keep], np.asarray(root_xy, dtype=dt)[keep]
    root = np.concatenate([xy, f[:, 2:3]], 1)
    cond = (f - avg) / std
    cond[:, :3] = (root - avg[:3]) / std[:3]
    r6 = f[:, COL_ROT6D:].reshape(-1, NUM_JOINTS, 6)
    rotmat = rot6d_to_rotmat_reference(r6, dt, probes)
    # the racket: the chain of transforms Pelvis .. Wrist (utils/racket.py:235-269), the eastern vectors in the wrist's frame
    chain = RACKET_CHAIN[st["righthand"] if racket is None else racket["righthand"]]
    R, p = rotmat[:, chain[0]], bind[:, chain[0]].astype(dt)
    for j in chain[1:8]:
        p = (R * bind[:, j][:, None]).sum(-1) + p
        R = R @ rotmat[:, j]
    if racket is None:
        direction, normal = -R[:, :, 0], R[:, :, 1]
    else:
        direction, normal = ((R * np.asarray(racket[k], dtype=np.float32).astype(dt)).sum(-1) for k in ("direction", "normal"))
    pos = p + root
    for length in RACKET_LENGTHS:
        pos = pos + direction * dt(length)
    o["swing_type"][ids], o["swing_type_cycle"][ids] = -1, -1
    o["conditions"][ids, 0], o["root_pos"][ids], o["root_vel"][ids] = cond, root, f[:, COL_ROOT_VEL:COL_ROOT_VEL + 3]
    o["joint_rot6d"][ids], o["joint_rotmat"][ids], o["racket_pos"][ids], o["racket_normal"][ids] = r6, rotmat, pos, normal
    if not st["is_train"]:
        o["joint_rot"][ids] = rotmat_to_angle_axis_reference(rotmat, dt, probes)
    return o


def mvae_reset_flagged_reference(st, avg, std, s, flags, init_feature, root_xy, joint_pos_bind_rel, dt=np.float32, probes=None):
    """`v2p_mvae_reset_flagged` on arrays: mvae_reset_reference over the envs whose flag is not 0.  init_feature [N,288] and root_xy [N,2]
    hold a row per ENV (root_xy: the caller's table, or `device_rng.root_xy_reference(seed, call, N)`, or the centre)."""
    ids = np.flatnonzero(np.asarray(flags))
    return mvae_reset_reference(st, avg, std, s, ids, np.asarray(init_feature)[ids], np.asarray(root_xy)[ids], joint_pos_bind_rel, dt, probes)


def mvae_dual_step_reference(st, w, avg, std, s, latents, residual=None, dt=np.float32, probes=None):
    """`MVAEPlayer.step` under `_is_dual` (mvae_player.py:191-199) on arrays: mvae_step_reference of side 0 on the even rows and of side 1
    on the odd rows - st: player_settings(...) of `dual_mode: different`; w, avg, std: pairs - and then the reference's quirk: its non-init
    branch writes the root-position columns of EVERY env's condition (:254-262) and side 1's call runs last, so those three columns are
    normalised with side 1's avg and std in the even rows too.  probes: a pair of dicts, one per side."""
    n = len(latents)
    out = []
    for i in (0, 1):
        rows = {k: np.asarray(v)[i::2] for k, v in s.items() if v is not None}
        out.append(mvae_step_reference(st["sides"][i], w[i], avg[i], std[i], rows, np.asarray(latents)[i::2], None if residual is None or not len(residual) else np.asarray(residual)[i::2],
                                       dt, None if probes is None else probes[i]))
    o = {}
    for k in out[0]:
        o[k] = np.empty((n,) + out[0][k].shape[1:], out[0][k].dtype)
        o[k][0::2], o[k][1::2] = out[0][k], out[1][k]
    a1, s1 = np.asarray(avg[1], dtype=dt).reshape(FRAME), np.asarray(std[1], dtype=dt).reshape(FRAME)
    o["conditions"][0::2, 0, :3] = (o["root_pos"][0::2] - a1[:3]) / s1[:3]
    return o


def mvae_dual_reset_reference(st, avg, std, s, env_ids, init_feature, root_xy, joint_pos_bind_rel, dt=np.float32, probes=None):
    """`reset_dual` under `_is_dual` (mvae_player.py:175-180) on arrays, for env_ids of whole pairs, ascending: mvae_reset_reference of each
    side on its ids (a row is normalised with its own side's statistics; the init branch writes only those rows), both with the batch's one
    racket.  joint_pos_bind_rel [24,3] or [rows,24,3]: `infer_with_fk` reads joint_pos_bind_rel[:batch] of a side's sub-list, so the pair at
    list positions 2i, 2i+1 reads row i.  probes: a pair of dicts, one per side."""
    ids = np.asarray(env_ids, dtype=np.int64).reshape(-1)
    bind = np.asarray(joint_pos_bind_rel).reshape(-1, NUM_JOINTS, 3)
    o = {k: (np.asarray(v, dtype=dt) if np.asarray(v).dtype.kind == "f" else v) for k, v in s.items() if v is not None}  # (a float64 evaluation is stored as such)
    for i in (0, 1):
        at = np.nonzero(ids % 2 == i)[0]
        o = mvae_reset_reference(st["sides"][i], avg[i], std[i], o, ids[at], np.asarray(init_feature)[at], np.asarray(root_xy)[at], bind[at >> 1] if len(bind) > 1 else bind, dt,
                                 None if probes is None else probes[i], racket=st["racket"])
    return o


def mvae_dual_reset_flagged_reference(st, avg, std, s, flags, init_feature, root_xy, joint_pos_bind_rel, dt=np.float32, probes=None):
    """`v2p_mvae_dual_reset_flagged` on arrays: mvae_dual_reset_reference over the envs whose flag is not 0 - whole pairs, as
    `v2p_ctl_pair_reset_begin` leaves the mask.  init_feature [N,288] and root_xy [N,2] hold a row per ENV (init_feature: the serve and
    ready frames interleaved by parity and serve_from; root_xy: the caller's table, or `device_rng.root_xy_reference(seed, call, N)`);
    joint_pos_bind_rel is one [24,3] row."""
    ids = np.flatnonzero(np.asarray(flags))
    if not whole_pairs(ids):
        raise ValueError("mvae_dual_reset_flagged_reference: the flags of a pair (2k, 2k+1) must both be up or both be 0; flagged: %s" % ids.tolist())
    if np.asarray(joint_pos_bind_rel).size != NUM_JOINTS * 3:
        raise ValueError("mvae_dual_reset_flagged_reference: joint_pos_bind_rel is one [24,3] row (a row per pair is read by list position: not built by flags)")
    return mvae_dual_reset_reference(st, avg, std, s, ids, np.asarray(init_feature)[ids], np.asarray(root_xy)[ids], joint_pos_bind_rel, dt, probes)


def whole_pairs(ids):
    """Is the ascending list `ids` made of whole pairs (2k, 2k+1)?"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    return len(ids) % 2 == 0 and bool((ids[0::2] % 2 == 0).all()) and bool((ids[1::2] == ids[0::2] + 1).all())


def dual_reset_rows(reset_reaction_env_ids, reset_recovery_env_ids):
    """Which envs `reset_dual` (mvae_player.py:167-182) resets and from which frame: (ids ascending, from_ready [len(ids)] bool - True:
    the ready frame of a reaction id, False: the serve frame of a recovery id).  An id in both lists takes the serve frame, which the
    reference writes last - and appears ONCE here, where the reference's `cat(...).sort()` keeps it twice (and draws two root positions for
    it, the second of which stays).  The dual controller's `reset(ids)` never names an env on both sides."""
    rea, rec = np.asarray(reset_reaction_env_ids, dtype=np.int64).reshape(-1), np.asarray(reset_recovery_env_ids, dtype=np.int64).reshape(-1)
    ids = np.unique(np.concatenate([rea, rec]))
    return ids, ~np.isin(ids, rec)


# ------------------------------------------------------------------------------------------------------------------ the player
DUAL_MAP_PARITY, DUAL_MAP_HALVES = 0, 1  # V2P_MVAE_DUAL_MAP_*


class MotionVAEPlayer:
    """`MVAEPlayer` on the device, single player.  Attribute names are the reference's.  cfg: `player`, `righthand`, `add_residual_dof`,
    `test_mode`; weights: weights_from_state_dict(...); avg, std [288]; init_data [M,1,288] or [M,288] (`vae_init_conditions`: fewer rows
    than envs repeat the first row, as the reference does); joint_pos_bind_rel [24,3] of the player's SMPL body.  With cfg `dual_mode: True`
    init_data_ready and init_data_serve (`vae_init_conditions_ready` / `_serve`, mvae_player.py:122-128: the first row of each, for every
    env) are required, and `reset_dual` resets whole pairs from them.

    With cfg `dual_mode: 'different'` (`player`, `righthand`, `grip` lists of two, `serve_from`) the batch holds two players: weights, avg,
    std, init_data_ready and init_data_serve are PAIRS (side 0: envs 2k, side 1: envs 2k+1); the two initial frames are the first row of
    each side's file, interleaved by parity (`init_states`, mvae_player.py:113-121); init_data is not read (pass None).  `step` is
    v2p_mvae_dual_step, `reset_dual` v2p_mvae_dual_reset; `reset(ids)` is refused, as the reference's would fail on its missing `_mvae`.
    joint_pos_bind_rel may be [rows,24,3]: the reset of the pair at list positions 2i, 2i+1 reads row i (v2p_rollout.h)."""

    dual_mapping = DUAL_MAP_HALVES  # (the faster of the two at 8192 envs; tools/mvae_dual_bench.py times both)

    def __init__(self, cfg, num_envs, weights, avg, std, init_data, joint_pos_bind_rel, is_train, device, init_data_ready=None, init_data_serve=None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("MotionVAEPlayer: the motion generator is a HIP kernel - it must live on a GPU (no CPU fallback)")
        _lib.load()
        self.cfg, self.num_envs, self.device, self._is_train = dict(cfg), int(num_envs), dev, bool(is_train)
        self.settings = player_settings(cfg, is_train, num_envs)
        self._is_dual = bool(self.settings.get("dual"))
        self._predict_phase = True
        n = self.num_envs
        f, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.long, device=dev)
        last = lambda d: torch.as_tensor(np.asarray(d, dtype=np.float32) if not torch.is_tensor(d) else d).to(**f).reshape(len(d), -1, FRAME)[:, -1]
        self._init_data = self._init_data_ready = self._init_data_serve = None
        if self._is_dual:
            for name, v in (("weights", weights), ("avg", avg), ("std", std), ("init_data_ready", init_data_ready), ("init_data_serve", init_data_serve)):
                if not isinstance(v, (list, tuple)) or len(v) != 2:
                    raise ValueError("MotionVAEPlayer: dual_mode 'different' takes %s as a pair (side 0, side 1)" % name)
            self._weights = tuple(pack_weights(weights[i], avg[i], std[i], dev) for i in (0, 1))
            # (init_states :113-121: cat(first row of side 0's file, of side 1's).repeat(n / 2))
            pairs = lambda d: torch.cat([last(d[0])[:1], last(d[1])[:1]], 0).repeat(n // 2, 1).contiguous()
            self._init_data_ready, self._init_data_serve = pairs(init_data_ready), pairs(init_data_serve)
            self._joint_pos_bind_rel = torch.as_tensor(np.asarray(joint_pos_bind_rel, dtype=np.float32)).to(**f).reshape(-1, NUM_JOINTS, 3).contiguous()
            self._cfg_struct = (_lib.MvaeCfg * 2)(*(cfg_struct(st) for st in self.settings["sides"]))
            self._weights_struct = (_lib.MvaeWeights * 2)(*(_lib.MvaeWeights(**{k: w[k].data_ptr() for k in _lib.MVAE_WEIGHT_NAMES}) for w in self._weights))
            self._racket_struct = racket_struct(self.settings["racket"])
        else:
            self._weights = pack_weights(weights, avg, std, dev)
            self._avg, self._std = self._weights["avg"], self._weights["std"]
            init = last(init_data)
            self._init_data = (init[:1].repeat(n, 1) if len(init) < n else init[:n]).contiguous()
            if self.cfg.get("dual_mode"):
                if init_data_ready is None or init_data_serve is None:
                    raise ValueError("MotionVAEPlayer: dual_mode needs init_data_ready and init_data_serve")
                first = lambda d: last(d)[:1].repeat(n, 1).contiguous()
                self._init_data_ready, self._init_data_serve = first(init_data_ready), first(init_data_serve)
            self._joint_pos_bind_rel = torch.as_tensor(np.asarray(joint_pos_bind_rel, dtype=np.float32)).to(**f).reshape(NUM_JOINTS, 3).contiguous()
            self._cfg_struct = cfg_struct(self.settings)
            self._weights_struct = _lib.MvaeWeights(**{k: self._weights[k].data_ptr() for k in _lib.MVAE_WEIGHT_NAMES})
        self._conditions = torch.zeros((n, 1, FRAME), **f)
        self._root_pos, self._root_vel = torch.zeros((n, 3), **f), torch.zeros((n, 3), **f)
        self._joint_rot6d, self._joint_rotmat = torch.zeros((n, NUM_JOINTS, 6), **f), torch.zeros((n, NUM_JOINTS, 3, 3), **f)
        self._joint_rot = torch.zeros((n, NUM_JOINTS, 3), **f)
        self._racket_pos, self._racket_normal = torch.zeros((n, 3), **f), torch.zeros((n, 3), **f)
        self._phase_pred = torch.zeros(n, **f)
        self._swing_type = torch.full((n,), -1, **i64)
        self._swing_type_cycle = self._swing_type.clone()
        self._latents = None
        # the key of the kernel's own draw (`reset_flagged` without a table) and the count of its launches: host numbers, never read
        # back from the device
        self.seed = int(self.cfg.get("seed", 0)) & (2 ** 64 - 1)
        self._reset_calls = 0
        self._dual_init_tables = {}  # serve_from -> [N,288]: `dual_init_table`

    def _buffers(self):
        # (built per call: `_swing_type_cycle` may have become another task's tensor, TennisControllerTask.attach_motion_generator)
        t = {k: getattr(self, "_" + k) for k in _lib.MVAE_BUFFER_NAMES}
        for k, v in t.items():
            if not v.is_cuda or not v.is_contiguous():
                raise RuntimeError("MotionVAEPlayer: state tensor _%s must be a contiguous GPU tensor" % k)
        return _lib.MvaeBuffers(**{k: v.data_ptr() for k, v in t.items()})

    def state_arrays(self):
        return {k: getattr(self, "_" + k).detach().cpu().numpy().copy() for k in _lib.MVAE_BUFFER_NAMES}

    def draw_root_xy(self, count):
        """The start of a player near the baseline's centre (mvae_player.py:230-236): a draw, or the centre when evaluating in a test mode
        other than `random`."""
        if self._is_train or self.cfg.get("test_mode", "random") == "random" or self.cfg.get("dual_mode"):  # (the reference: `is not None`, mvae_player.py:230 - a cfg that says `dual_mode: False` keeps what it did here)
            return (torch.rand((count, 2), device=self.device) - 0.5) * torch.tensor([2.0, 1.5], device=self.device) + torch.tensor([0.0, -13.0], device=self.device)
        return torch.tensor([0.0, -13.0], device=self.device).repeat(count, 1)

    def reset(self, env_ids, root_xy=None):
        if self._is_dual:
            raise RuntimeError("MotionVAEPlayer.reset: with dual_mode 'different' envs are reset in whole pairs by reset_dual (the reference's reset reads a `_mvae` it does not have)")
        ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long).contiguous()
        if ids.numel() == 0:
            return
        self._reset_rows(ids, self._init_data[ids.clamp(0, self.num_envs - 1)].contiguous(), root_xy)

    def root_rule(self):
        """'draw' or 'centre': the branch `draw_root_xy` takes, as `reset_flagged` hands it to the kernel."""
        return "draw" if self._is_train or self.cfg.get("test_mode", "random") == "random" else "centre"

    def reset_flagged(self, flags, root_xy=None):
        """`reset(env_ids)` for the envs whose flag ([N] int64 on the device, non-zero = reset) is up, in one launch over all envs
        (`v2p_mvae_reset_flagged`): no id list, no gather of `_init_data`, no host read.  root_xy [N,2] (row e: env e's start) stands in
        for the draw; without it the kernel draws the start itself (`root_rule()`: or takes the centre) from (seed, call, env) - cfg
        `seed`, and the count of such launches - as `device_rng.root_xy_reference` states it."""
        if self._is_dual or self.cfg.get("dual_mode"):
            raise NotImplementedError("MotionVAEPlayer.reset_flagged: the reset by flags is not built with dual_mode (pairs are reset by reset_dual, from an id list)")
        n = self.num_envs
        if not torch.is_tensor(flags) or flags.dtype != torch.int64 or flags.device != self.device or not flags.is_contiguous() or flags.numel() != n:
            raise RuntimeError("MotionVAEPlayer.reset_flagged: flags must be a contiguous int64 tensor [%d] on %s" % (n, self.device))
        xy, rule = None, None
        if root_xy is not None:
            xy = root_xy
            if not torch.is_tensor(xy) or xy.dtype != torch.float32 or xy.device != self.device or not xy.is_contiguous() or tuple(xy.shape) != (n, 2):
                raise RuntimeError("MotionVAEPlayer.reset_flagged: root_xy must be a contiguous float32 tensor [%d, 2] on %s" % (n, self.device))
        else:
            rule = _lib.MvaeRootRule(rule=_lib.MVAE_ROOT_RULES[self.root_rule()], seed=self.seed, call=self._reset_calls & (2 ** 64 - 1))
            self._reset_calls += 1
        b = self._buffers()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().v2p_mvae_reset_flagged(C.byref(self._cfg_struct), n, C.byref(self._weights_struct), C.byref(b), _lib.ptr(flags), _lib.ptr(self._init_data),
                                                          _lib.ptr(xy), None if rule is None else C.byref(rule), _lib.ptr(self._joint_pos_bind_rel),
                                                          _lib.current_stream(self.device)), "v2p_mvae_reset_flagged")

    def dual_init_table(self, serve_from=None):
        """[N,288] by env: the ready frame where the env receives, the serve frame where it serves - of every pair the even env receives
        with serve_from 'near' and the odd env with 'far' (physics_mvae_controller_dual.py:31-36).  Built once per serve_from (default:
        the player's cfg `serve_from`, 'near' where it has none)."""
        if self._init_data_ready is None:
            raise RuntimeError("MotionVAEPlayer.dual_init_table: the player was not made with cfg dual_mode: True or 'different'")
        serve_from = self.cfg.get("serve_from", "near") if serve_from is None else serve_from
        if serve_from not in _lib.SERVE_FROM:
            raise ValueError("MotionVAEPlayer: serve_from %r is neither 'near' nor 'far'" % (serve_from,))
        tables = self._dual_init_tables
        if serve_from not in tables:
            receives = (torch.arange(self.num_envs, device=self.device) % 2 == _lib.SERVE_FROM[serve_from]).view(-1, 1)
            tables[serve_from] = torch.where(receives, self._init_data_ready, self._init_data_serve).contiguous()
        return tables[serve_from]

    def reset_dual_flagged(self, flags, root_xy=None, serve_from=None):
        """`reset_dual(receivers, servers)` for the pairs whose flags ([N] int64 on the device, non-zero = reset; BOTH words of a pair up,
        as `v2p_ctl_pair_reset_begin` leaves them) are up, in one launch over all envs: `v2p_mvae_dual_reset_flagged` under `dual_mode:
        different`, `v2p_mvae_reset_flagged` on the per-env table of serve and ready frames (`dual_init_table`) under `dual_mode: True`.
        No id list, no gather, no host read.  root_xy [N,2] (row e: env e's start) stands in for the draw; without it the kernel draws
        the start itself from (seed, call, env) as `device_rng.root_xy_reference` states it - always a draw, never the centre:
        `draw_root_xy` draws whenever `dual_mode` is set.  joint_pos_bind_rel with a row per pair is refused (the id-list form reads
        the row of a pair's position in the list)."""
        if self._init_data_ready is None:
            raise RuntimeError("MotionVAEPlayer.reset_dual_flagged: the player was not made with cfg dual_mode: True or 'different'")
        n = self.num_envs
        if not torch.is_tensor(flags) or flags.dtype != torch.int64 or flags.device != self.device or not flags.is_contiguous() or flags.numel() != n:
            raise RuntimeError("MotionVAEPlayer.reset_dual_flagged: flags must be a contiguous int64 tensor [%d] on %s" % (n, self.device))
        xy, rule = None, None
        if root_xy is not None:
            xy = root_xy
            if not torch.is_tensor(xy) or xy.dtype != torch.float32 or xy.device != self.device or not xy.is_contiguous() or tuple(xy.shape) != (n, 2):
                raise RuntimeError("MotionVAEPlayer.reset_dual_flagged: root_xy must be a contiguous float32 tensor [%d, 2] on %s" % (n, self.device))
        bind = self._joint_pos_bind_rel
        if self._is_dual and len(bind) > 1:
            raise NotImplementedError("MotionVAEPlayer.reset_dual_flagged: joint_pos_bind_rel has %d rows; the id-list reset reads the row of a pair's position in the "
                                      "list, which by flags would need a prefix count of the flagged pairs: not built (one [24,3] row is)" % len(bind))
        table = self.dual_init_table(serve_from)
        if xy is None:
            rule = _lib.MvaeRootRule(rule=_lib.MVAE_ROOT_RULES["draw"], seed=self.seed, call=self._reset_calls & (2 ** 64 - 1))
            self._reset_calls += 1
        b = self._buffers()
        stream, rule_p = _lib.current_stream(self.device), None if rule is None else C.byref(rule)
        with torch.cuda.device(self.device):
            if self._is_dual:
                _lib.check(_lib.load().v2p_mvae_dual_reset_flagged(self._cfg_struct, n, self._weights_struct, C.byref(b), C.byref(self._racket_struct), _lib.ptr(flags),
                                                                   _lib.ptr(table), _lib.ptr(xy), rule_p, _lib.ptr(bind), len(bind), stream), "v2p_mvae_dual_reset_flagged")
            else:
                _lib.check(_lib.load().v2p_mvae_reset_flagged(C.byref(self._cfg_struct), n, C.byref(self._weights_struct), C.byref(b), _lib.ptr(flags), _lib.ptr(table),
                                                              _lib.ptr(xy), rule_p, _lib.ptr(bind), stream), "v2p_mvae_reset_flagged")

    def reset_dual(self, reset_reaction_env_ids, reset_recovery_env_ids, root_xy=None):
        """`reset_dual` (mvae_player.py:167-182) with `dual_mode: True` or 'different': the envs of both lists, in ascending order, start from the ready
        frame (reaction ids: the receivers) or the serve frame (recovery ids: the servers) through the launch of `reset`.  root_xy
        [len(both),2], in that ascending order, replaces the draw near the baseline's centre."""
        if self._init_data_ready is None:
            raise RuntimeError("MotionVAEPlayer.reset_dual: the player was not made with cfg dual_mode: True or 'different'")
        as_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else x
        ids, from_ready = dual_reset_rows(as_np(reset_reaction_env_ids), as_np(reset_recovery_env_ids))
        if self._is_dual and not whole_pairs(ids):
            # (the reference splits the sorted list by position, `env_ids[::2]` / `[1::2]`: that is the env's side only for whole pairs)
            raise ValueError("MotionVAEPlayer.reset_dual: with dual_mode 'different' the two lists together must be whole pairs (2k, 2k+1); got %s" % ids.tolist())
        if len(ids) == 0:
            return
        ids = torch.from_numpy(ids).to(self.device)
        rows = ids.clamp(0, self.num_envs - 1)
        feature = torch.where(torch.from_numpy(from_ready).to(self.device).view(-1, 1), self._init_data_ready[rows], self._init_data_serve[rows])
        self._reset_rows(ids.contiguous(), feature.contiguous(), root_xy)

    def _reset_rows(self, ids, feature, root_xy):
        xy = self.draw_root_xy(ids.numel()) if root_xy is None else torch.as_tensor(root_xy, dtype=torch.float32, device=self.device)
        xy = xy.to(torch.float32).reshape(ids.numel(), 2).contiguous()
        b = self._buffers()
        if self._is_dual:
            bind = self._joint_pos_bind_rel
            if len(bind) > 1 and 2 * len(bind) < ids.numel():
                raise ValueError("MotionVAEPlayer.reset_dual: joint_pos_bind_rel has %d rows, %d pairs are reset" % (len(bind), ids.numel() // 2))
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().v2p_mvae_dual_reset(self._cfg_struct, self.num_envs, self._weights_struct, C.byref(b), C.byref(self._racket_struct), _lib.ptr(ids),
                                                           int(ids.numel()), _lib.ptr(feature), _lib.ptr(xy), _lib.ptr(bind), len(bind), _lib.current_stream(self.device)),
                           "v2p_mvae_dual_reset")
            return
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().v2p_mvae_reset(C.byref(self._cfg_struct), self.num_envs, C.byref(self._weights_struct), C.byref(b), _lib.ptr(ids), int(ids.numel()),
                                                  _lib.ptr(feature), _lib.ptr(xy), _lib.ptr(self._joint_pos_bind_rel), _lib.current_stream(self.device)), "v2p_mvae_reset")

    def step(self, latents, residual=None):
        if not latents.is_cuda or latents.shape != (self.num_envs, LATENT):
            raise RuntimeError("MotionVAEPlayer.step: latents must be a GPU tensor [%d, %d]" % (self.num_envs, LATENT))
        self._latents = latents
        z = latents.to(torch.float32).contiguous()
        r = None
        if residual is not None and len(residual) != 0:
            if not self.settings["add_residual_dof"]:
                raise RuntimeError("MotionVAEPlayer.step: a residual needs cfg add_residual_dof = 'euler'")
            if residual.shape != (self.num_envs, 3):
                raise RuntimeError("MotionVAEPlayer.step: residual must be [%d, 3]" % self.num_envs)
            r = residual.to(device=self.device, dtype=torch.float32).contiguous()
        b = self._buffers()
        if self._is_dual:
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().v2p_mvae_dual_step(self._cfg_struct, self.num_envs, self._weights_struct, C.byref(b), _lib.ptr(z), _lib.ptr(r), self.dual_mapping,
                                                          _lib.current_stream(self.device)), "v2p_mvae_dual_step")
            return
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().v2p_mvae_step(C.byref(self._cfg_struct), self.num_envs, C.byref(self._weights_struct), C.byref(b), _lib.ptr(z), _lib.ptr(r),
                                                 _lib.current_stream(self.device)), "v2p_mvae_step")
