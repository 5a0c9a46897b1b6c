"""The tennis controller's task step on the device (vid2player/env/tasks/physics_mvae_controller.py, `PhysicsMVAEController`).

What consumes the racket + ball batch (`HumanoidSMPLIMRacketBall`), the pool of incoming launches and the outgoing estimator tables
(`ball_traj.py`): the actor and task observations (:316-360), the three reward laws (:368-406, 492-602), the true and estimated bounce
bookkeeping (:271-314), the reaction / recovery / termination logic (:408-436) and the ball-trajectory window (:362-366).  One control
step of it is ONE kernel launch, `v2p_tennis_task_step` (csrc/tennis_task.hip), without a host synchronisation; the observation of
freshly reset envs is `v2p_tennis_task_obs`.  The racket hit at more than 2 substeps - read from the ball's velocity change
(humanoid_smpl_im_mvae.py:800-808), which the racket task itself does not do - is part of that step.

The MVAE motion generator is `vid2player3d_amd.mvae.MotionVAEPlayer` (one more launch per control step, `v2p_mvae_step`).  Attached with
`attach_motion_generator(player)`, it is stepped by `pre_physics_step(actions)` and reset where the reference resets it, and
`post_physics_step()` reads the swing phase and the swing type from it.  Without one, they come in as tensors from whoever drives the
step (`post_physics_step(phase_pred, swing_type, swing_type_cycle)`).

What turns the generator's kinematic pose into the imitation target of the low-level policy (`post_mvae_step` / `_smpl_to_sim`) is
`vid2player3d_amd.mvae_target.ImitationTarget` (one more launch, `v2p_mvae_target_step`, and the imitation observation).  Attached with
`attach_imitation_target(target)`, `pre_physics_step` ends with `post_mvae_step()`, the reset puts the humanoid into the generator's
pose, and `physics_step(ll_actions)` steps the wrapped task on the PD targets of the low-level policy's actions: `pre_physics_step` ->
`physics_step` -> `post_physics_step` is vid2player's control step.  Without one, every path is as before.  The dual controller is
`tasks.tennis_controller_dual.DualTennisControllerTask`.  `optimize_two_hand_backhand` (single=True) is two_hand_fix.py.  Not built: `update_mvae_from_sim`.

The low-level policy network is `vid2player3d_amd.policies.LowLevelPolicy` (two launches around the dense layers).  Attached with
`attach_low_level_policy(policy)`, `physics_step()` takes no argument: the policy computes the imitation observation in place, runs its
network(s) and hands the PD targets to the engine.  `step(actions)` is then the reference's `PhysicsMVAEController.step(actions)`.

With cfg v2p `random_walk_in_recovery` (every shipped controller config sets it) the action part of `pre_physics_step` is ONE launch,
`v2p_controller_actions` (csrc/controller_actions.hip): the copy of the actions, the scaled latent and residual columns, and the latent
of envs in recovery (`_tar_action == 0`) replaced by clamp(N(0,1), -5, 5) (:252-257).  The normals come from the counter-based generator
of csrc/philox.hpp under the controller's `seed` and a call counter kept on the host; `controller_actions_reference` with
`device_rng.philox_words` states them in numpy.  A departure from the reference: it deals draw k of a step to the k-th env in recovery
(a host read sizes the slice), here env i owns its draws whatever the other envs do.  Both are iid draws.  Without the key the
torch lines run as before.

With cfg v2p `task_reset: 'device'` the flag-driven half of `_reset_envs` - ball draw from the offline pool, `_reset_recovery_tasks`,
`_reset_reaction_tasks`, the observation of the flagged envs - is ONE launch over all envs, `v2p_tennis_task_reset`
(csrc/tennis_reset.hip), without a `nonzero()` or any other host read; `task_reset_reference` states it in numpy.  Its draws come from
the same generator (stream RESET), with the same departure.  The default `'torch'` is the indexed torch code with torch's own random
stream, as before.  `'device'` needs the task's ball generator to be a `TennisBallGeneratorOffline` on the task's device.

Under `'device'` the humanoid half runs by flags too: `reset_by_flags()` resets the envs whose `reset_buf` is up - the controller's
bookkeeping, the generator's initial frame, the target's pose, the engine's push (csrc/flag_reset.hip, csrc/mvae_player_flagged.hip) around
that launch - as one fixed sequence of six launches over all envs, without an id list or a host read.  `reset(env_ids)` stays as it is
and is the default of the PPO agent (`reset_mode`).  `_reset_root_xy` [N,2] (default None) gives every env a start that stands in for
the generator's draw in both.

Evaluation (`run.py --test`) is `TennisControllerEval`, the reference's `MVAEControllerVis` (env/tasks/mvae_controller_vis.py) without
the viewer: the same task with the test-mode episode law (:64-79: an episode ends only past `episodeLength`; the reaction flag waits for
the bounce of a returned ball, the recovery flag also rises on a slow ball), the four per-env meters `hit_rate`, `fh_ratio`,
`bounce_in_rate`, `bounce_in_pos_error` (:81-95) and the record the evaluation hands on (:140-146, `_joint_rot` of the simulated body
included) - all in the step's ONE launch, `v2p_tennis_eval_step` (csrc/tennis_eval.hip), without a host read.  `select_best()` and
`summary()` read them after the run; `eval_player.ControllerEvalPlayer` is the loop.  `eval_step_reference` / `eval_record_reference`
state it in numpy; `fixed_joint_rot(env_ids)` is cfg v2p `fix_two_hand_backhand_post` (two_hand_fix.py).  Not built: rendering, video and HTML output, `vis_pd_target`, `MVAEControllerVisDual`,
the reference's frame 0 of the record (taken after the first reset, before any step).

`task_step_reference` is a numpy statement of the same step on arrays - the checker of the tests, as `ball_traj.resample_reference`
and `body_shapes` have theirs; the product never calls it.  There is no CPU path: a CPU device or a missing library is a RuntimeError.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from ..ball_traj import NET_HEIGHT, traj_out_params
from ..mvae import LATENT

NUM_ACTOR_OBS = 3 + 3 + 24 * 3 + 24 * 6 + 3  # physics_mvae_controller.py:148
TRAJ_FRAMES = 100
REWARD_TYPES = {"reach": 0, "return": 1, "return_w_estimate": 2}
SUB_REWARD_NAMES = {"reach": "pos_reward", "return": "pos_reward,ball_pos_reward", "return_w_estimate": "pos_reward,ball_pos_reward"}
GRIP_NORMALS = {"eastern": (0.0, 1.0, 0.0), "semi_western": (0.0, 1.0 / math.sqrt(2), 1.0 / math.sqrt(2))}  # humanoid_smpl_im_mvae.py:835-838
COURT = (-4.11, 4.11, 0.0, 11.89)  # the bounce tests' court (:285-286): x0, x1, y0, y1


def grids_of(params=traj_out_params):
    """The five (lo, hi, step) ranges of the out-estimator in the order of v2p_tennis_cfg.grid."""
    return np.array([params.VEL_X_RANGE, params.VEL_Y_RANGE, params.VSPIN_RANGE, params.TRAJ_X_RANGE, params.TRAJ_Y_RANGE], dtype=np.float64)


def task_settings(reward_type="return", obs_ball_traj_length=100, use_history_ball_obs=False, use_random_ball_target=False, contact_by_velocity=False,
                  enable_early_termination=False, max_episode_length=300, grip="eastern", court_min=(-20.0, -40.0), court_max=(20.0, 0.0),
                  reward_scales=None, reward_weights=None, grids=None):
    """The settings of one task step as a plain dict (what both the kernel's v2p_tennis_cfg and task_step_reference are made from);
    defaults of scales and weights are the reference's (:512-516, 529, 543-544, 594-595)."""
    if reward_type not in REWARD_TYPES:
        raise ValueError("reward_type %r is none of %s" % (reward_type, sorted(REWARD_TYPES)))
    L = int(obs_ball_traj_length)
    if not 1 <= L <= TRAJ_FRAMES:
        raise ValueError("obs_ball_traj_length %d outside 1..%d" % (L, TRAJ_FRAMES))
    sc, w = dict(reward_scales or {}), dict(reward_weights or {})
    return dict(reward_type=reward_type, L=L, use_history=bool(use_history_ball_obs), use_target=bool(use_random_ball_target),
                contact_by_velocity=bool(contact_by_velocity), early_termination=bool(enable_early_termination), max_episode_length=int(max_episode_length),
                grip_normal=tuple(float(x) for x in (GRIP_NORMALS[grip] if isinstance(grip, str) else grip)),
                court_min=tuple(float(x) for x in court_min[:2]), court_max=tuple(float(x) for x in court_max[:2]),
                scale_pos=float(sc.get("pos", 5.0)), scale_phase=float(sc.get("phase", 10.0)), scale_bounce_pos=float(sc.get("bounce_pos", 0.05)),
                scale_bounce_time=float(sc.get("bounce_time", 0.1)), weight_pos=float(w.get("pos", 1.0 if reward_type == "reach" else 0.0)),
                weight_ball_pos=float(w.get("ball_pos", 0.0)), grids=np.asarray(grids_of() if grids is None else grids, dtype=np.float64))


def obs_width(st):
    return NUM_ACTOR_OBS + 3 * st["L"] + (2 if st["use_target"] else 0)


def num_sub_rewards(st):
    return 1 if st["reward_type"] == "reach" else 2


def cfg_struct(st, table_shape_x, table_shape_y):
    """v2p_tennis_cfg of a settings dict and the shapes of the two tables ([B,nx], [B,ny,2])."""
    c = _lib.TennisCfg(reward_type=REWARD_TYPES[st["reward_type"]], obs_ball_traj_length=st["L"], use_history_ball_obs=int(st["use_history"]),
                       use_random_ball_target=int(st["use_target"]), contact_by_velocity=int(st["contact_by_velocity"]),
                       enable_early_termination=int(st["early_termination"]), max_episode_length=st["max_episode_length"],
                       scale_pos=st["scale_pos"], scale_phase=st["scale_phase"], scale_bounce_pos=st["scale_bounce_pos"], scale_bounce_time=st["scale_bounce_time"],
                       weight_pos=st["weight_pos"], weight_ball_pos=st["weight_ball_pos"], table_rows=int(table_shape_x[0]), table_nx=int(table_shape_x[1]),
                       table_ny=int(table_shape_y[1]))
    c.grip_normal[:] = st["grip_normal"]
    c.court_min[:] = st["court_min"]
    c.court_max[:] = st["court_max"]
    for g in range(5):
        c.grid[g][:] = [float(x) for x in st["grids"][g]]
    return c


def buffers_struct(tensors):
    """v2p_tennis_buffers of a dict name -> device tensor (names of _lib.TENNIS_BUFFER_NAMES; absent or None = NULL)."""
    unknown = set(tensors) - set(_lib.TENNIS_BUFFER_NAMES)
    if unknown:
        raise ValueError("not buffers of v2p_tennis_buffers: %s" % sorted(unknown))
    for k, t in tensors.items():
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise RuntimeError("tennis task step: buffer %s must be a contiguous GPU tensor (there is no CPU path)" % k)
    return _lib.TennisBuffers(**{k: t.data_ptr() for k, t in tensors.items() if t is not None})


def launch_step(st, tensors, n):
    """v2p_tennis_task_step on a dict of device tensors; returns the names string of the reward law."""
    lib = _lib.load()
    c = cfg_struct(st, tensors["traj_out_x"].shape, tensors["traj_out_y"].shape)
    b = buffers_struct(tensors)
    names = C.c_char_p()
    dev = tensors["obs"].device
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_tennis_task_step(C.byref(c), int(n), C.byref(b), C.byref(names), _lib.current_stream(dev)), "v2p_tennis_task_step")
    return names.value.decode()


def launch_obs(st, tensors, num_envs, env_ids):
    """v2p_tennis_task_obs for env_ids (int64 device tensor)."""
    lib = _lib.load()
    tx, ty = tensors.get("traj_out_x"), tensors.get("traj_out_y")
    c = cfg_struct(st, (1, 1) if tx is None else tx.shape, (1, 1, 2) if ty is None else ty.shape)
    b = buffers_struct(tensors)
    dev = tensors["obs"].device
    ids = env_ids.to(device=dev, dtype=torch.long).contiguous()
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_tennis_task_obs(C.byref(c), int(num_envs), C.byref(b), _lib.ptr(ids), int(ids.numel()), _lib.current_stream(dev)), "v2p_tennis_task_obs")


# ------------------------------------------------------------------------------------------------------------------ the checker
_f = np.float32


def _rotmat_rows(w, x, y, z):
    """quaternion_to_rotation_matrix (utils/konia_transform.py:474-549) of already unpacked numbers, float32: the 9 entries, row-major."""
    n = np.maximum(np.sqrt(w * w + x * x + y * y + z * z), _f(1e-12))
    w, x, y, z = w / n, x / n, y / n, z / n
    tx, ty, tz = _f(2) * x, _f(2) * y, _f(2) * z
    one = _f(1)
    return [one - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w, ty * x + tz * w, one - (tx * x + tz * z), tz * y - tx * w, tz * x - ty * w, tz * y + tx * w,
            one - (tx * x + ty * y)]


def _index(v, r):
    """round((clamp(v, lo, hi - step) - lo) / step) on float32 with the scalars rounded to float32 (ball_traj._index_f32)."""
    lo, top, step = _f(r[0]), _f(r[1] - r[2]), _f(r[2])
    return np.rint((np.clip(v, lo, top) - lo) / step)


def _in_court(x, y):
    return (x > _f(COURT[0])) & (x < _f(COURT[1])) & (y > _f(COURT[2])) & (y < _f(COURT[3]))


def observation_reference(st, s, env_ids=None):
    """`_compute_observations(env_ids)` (:316-360) in numpy float32 on a dict of arrays named like v2p_tennis_buffers.  Returns
    (obs rows [len(env_ids), W], ball_obs after the roll or None, racket_pos, racket_normal) for those envs."""
    ids = np.arange(len(s["ball_state"])) if env_ids is None else np.asarray(env_ids, dtype=np.int64)
    rb = np.asarray(s["rb_state"], dtype=_f).reshape(-1, 24, 13)[ids]
    rk = np.asarray(s["racket_state"], dtype=_f)[ids]
    root, rvel = rb[:, 0, 0:3], np.asarray(s["root_states"], dtype=_f)[ids, 7:10]
    rpos = rk[:, 0:3]
    L = st["L"]
    # racket normal: the wrist link's rotation, converted xyzw -> wxyz properly (humanoid_smpl_im_mvae.py:831-845)
    q = rb[np.arange(len(ids)), np.asarray(s["wrist_link"], dtype=np.int64)[ids], 3:7]
    m = _rotmat_rows(q[:, 3], q[:, 0], q[:, 1], q[:, 2])
    g = [_f(x) for x in st["grip_normal"]]
    rnorm = np.stack([m[3 * i] * g[0] + m[3 * i + 1] * g[1] + m[3 * i + 2] * g[2] for i in range(3)], -1)
    # quat_to_rot6d on the (x, y, z, w) numbers read as (w, x, y, z): columns 0 and 1 of that matrix
    q = rb[:, :, 3:7]
    m = _rotmat_rows(q[..., 0], q[..., 1], q[..., 2], q[..., 3])
    rot6d = np.stack([m[0], m[3], m[6], m[1], m[4], m[7]], -1).reshape(len(ids), 144)
    rel = (np.concatenate([rb[:, 1:, 0:3], rpos[:, None]], 1) - root[:, None]).reshape(len(ids), 72)
    hist = None
    if s.get("ball_obs") is not None:
        old = np.asarray(s["ball_obs"], dtype=_f).reshape(-1, L, 3)[ids]
        hist = np.concatenate([old[:, 1:], np.asarray(s["ball_state"], dtype=_f)[ids, None, 0:3]], 1)
    if st["use_history"]:
        window = hist
    else:
        traj = np.concatenate([np.asarray(s["ball_traj"], dtype=_f).reshape(-1, TRAJ_FRAMES, 3)[ids], np.zeros((len(ids), TRAJ_FRAMES + L, 3), _f)], 1)
        cur = np.clip(np.asarray(s["traj_cursor"], dtype=np.int64)[ids], 0, TRAJ_FRAMES)
        window = traj[np.arange(len(ids))[:, None], cur[:, None] + np.arange(L)[None]]
    cols = [root, rvel, rel, rot6d, rnorm, (window - rpos[:, None]).reshape(len(ids), 3 * L)]
    if st["use_target"]:
        cols.append(np.asarray(s["target_bounce_pos"], dtype=_f)[ids, 0:2] - root[:, 0:2])
    with np.errstate(invalid="ignore"):
        return np.concatenate(cols, 1).astype(_f), hist, rpos.copy(), rnorm.astype(_f)


def task_step_reference(st, s):
    """One control step of the task on arrays (post_physics_step :441-452 + the roll of physics_step :365-366), numpy float32.
    `st`: task_settings(...); `s`: arrays named like v2p_tennis_buffers (inputs and state before the step).  Returns a dict with every
    array the step writes: the updated state and the outputs.  Nothing in `s` is modified."""
    n = len(s["ball_state"])
    A = lambda k, dt=None: np.array(s[k], dtype=dt)
    o = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tar_time, progress, tar_action = A("tar_time", np.int64) + 1, A("progress", np.int64) + 1, A("tar_action", np.int64)
        ball = A("ball_state", _f)
        rb = A("rb_state", _f).reshape(n, 24, 13)
        root, rvel = rb[:, 0, 0:3], A("root_states", _f)[:, 7:10]
        hit, now = A("has_racket_contact").astype(bool), A("has_racket_contact_now").astype(bool)
        vy = ball[:, 8]
        if st["contact_by_velocity"]:
            now = ~hit & (vy > 0) & ((vy - A("prev_ball_vy", _f)) > _f(10))
            hit = hit | now
        # ---- _update_state
        bp = A("bounce_pos", _f)
        upd = (tar_action == 0) & A("has_bounce_now").astype(bool)
        bounce_in = np.where(upd, _in_court(bp[:, 0], bp[:, 1]), A("bounce_in").astype(bool))
        est, est_time, est_peak, est_in = A("est_bounce_pos", _f), A("est_bounce_time", _f), A("est_max_height", _f), A("est_bounce_in").astype(bool)
        G = st["grids"]
        VX, VY, VS, TX, TY = G
        tx, ty = np.asarray(s["traj_out_x"], dtype=_f), np.asarray(s["traj_out_y"], dtype=_f)
        valid = now & (ball[:, 8] > _f(VX[0])) & (ball[:, 9] > _f(VY[0])) & (ball[:, 9] < _f(VY[1])) & (ball[:, 2] < _f(TY[1]))
        x_net = ball[:, 0] + ball[:, 7] * np.abs(ball[:, 1] / ball[:, 8])
        valid &= (x_net > _f(-4)) & (x_net < _f(4))
        overflow = 0
        for e in np.nonzero(valid)[0]:  # TennisBallOutEstimator.estimate (tennis_ball_out_estimator.py:164-205), ball by ball
            b = ball[e]
            vel_x = np.sqrt(b[7] * b[7] + b[8] * b[8])
            overflow += int(vel_x >= _f(VX[1]))
            vspin = np.sqrt(b[10] * b[10] + b[11] * b[11] + b[12] * b[12]) / _f(math.pi * 2)
            dim1, dim2 = _f((VY[1] - VY[0]) / VY[2]), _f((VS[1] - VS[0]) / VS[2])
            ti = int(np.clip(int(_index(vel_x, VX) * dim1 * dim2 + _index(b[9], VY) * dim2 + _index(vspin, VS)), 0, len(tx) - 1))
            hi = int(np.clip(int(_index(b[2], TY)), 0, ty.shape[1] - 1))
            bx, by, bt = b[0] + ty[ti, hi, 0] * b[7] / vel_x, b[1] + ty[ti, hi, 0] * b[8] / vel_x, ty[ti, hi, 1]
            ni = int(np.clip(int(_index(-b[1] / b[8] * vel_x, TX)), 0, tx.shape[1] - 1))
            if tx[ti, ni] + b[2] < _f(NET_HEIGHT):
                bx = by = bt = _f(0)
            est[e, 0], est[e, 1], est_time[e], est_peak[e] = bx, by, bt, b[2] + tx[ti].max()
            est_in[e] = bool(_in_court(_f(bx), _f(by)))
        # ---- the reward
        rpos, bpos = A("racket_state", _f)[:, 0:3], ball[:, 0:3]
        d = bpos - rpos
        pos_err = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        phase = A("phase_pred", _f)
        rt = st["reward_type"]
        swing = A("swing_type_cycle" if rt == "return_w_estimate" else "swing_type", np.int64)
        early = (swing == -1) if rt == "reach" else (swing >= 2)
        pd = phase - np.where(early, _f(3), _f(math.pi))
        near = np.exp(-_f(st["scale_pos"]) * pos_err) * np.exp(-_f(st["scale_phase"]) * (pd * pd))
        tg = A("target_bounce_pos", _f)
        sq = lambda u: u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]
        if rt == "reach":
            sub = ((tar_action == 1).astype(_f) * near)[:, None]
            rew = sub[:, 0] * _f(st["weight_pos"])
        else:
            sub0 = (~hit).astype(_f) * near + hit.astype(_f)
            if rt == "return":
                err = np.where(A("has_bounce").astype(bool), sq(bp - tg), sq(bpos - tg))
                sub1 = hit.astype(_f) * np.clip((_f(400) - err) / _f(400), _f(0), _f(1))
            else:
                sub1 = est_in.astype(_f) * np.exp(-_f(st["scale_bounce_pos"]) * sq(est - tg)) * np.exp(-_f(st["scale_bounce_time"]) * est_time)
            sub = np.stack([sub0, sub1], -1)
            rew = _f(st["weight_pos"]) * sub0 + _f(st["weight_ball_pos"]) * sub1
        # ---- the observation
        obs, hist, _, rnorm = observation_reference(st, s)
        # ---- _compute_reset
        cmin, cmax = [_f(x) for x in st["court_min"]], [_f(x) for x in st["court_max"]]
        terminated = (root[:, 0] < cmin[0]) | (root[:, 1] < cmin[1]) | (root[:, 0] > cmax[0]) | (root[:, 1] > cmax[1])
        terminated |= np.isnan(obs).any(axis=1)
        reset = np.where(progress >= st["max_episode_length"] - 1, True, terminated)
        reaction = tar_time == A("tar_time_total", np.int64)
        behind = bpos[:, 1] < root[:, 1] - _f(1)
        recovery = (tar_action == 1) & (hit | behind)
        distance = A("distance", _f) + np.sqrt(rvel[:, 0] * rvel[:, 0] + rvel[:, 1] * rvel[:, 1])
        terminate = terminated.copy()
        if st["early_termination"]:
            terminate |= (recovery & ~hit) | behind
            if rt.startswith("return_w_estimate"):
                terminate |= hit & ~est_in
        terminated = terminated | terminate
        reset = reset | terminate
        recovery = recovery & ~terminate
        reaction = reaction | reset
    o.update(tar_time=tar_time, progress=progress, has_racket_contact=hit, has_racket_contact_now=now, prev_ball_vy=vy.copy(), bounce_in=bounce_in,
             est_bounce_pos=est, est_bounce_time=est_time, est_max_height=est_peak, est_bounce_in=est_in, distance=distance.astype(_f),
             vel_x_overflow=np.int64(np.asarray(s.get("vel_x_overflow", 0)).reshape(-1)[0] + overflow), racket_pos=rpos.copy(), racket_normal=rnorm, obs=obs,
             rew=rew.astype(_f), sub_rewards=sub.astype(_f), reset=reset.astype(np.int64), terminate=terminated.astype(np.int64), reset_reaction=reaction,
             reset_recovery=recovery, sub_rewards_names=SUB_REWARD_NAMES[rt])
    if hist is not None:
        o["ball_obs"] = hist
    if not st["use_history"]:
        o["traj_cursor"] = np.minimum(np.clip(A("traj_cursor", np.int64), 0, TRAJ_FRAMES) + 1, TRAJ_FRAMES).astype(np.int32)
    return o


# ------------------------------------------------------------------------------------------------------------------ the evaluation step
METER_NAMES = _lib.TENNIS_METER_NAMES  # the order of v2p_tennis_eval_buffers.meter_*: hit_rate, fh_ratio, bounce_in_rate, bounce_in_pos_error
METER_FIELDS = ("meter_sum", "meter_count", "meter_avg", "meter_max")
RECORD_NAMES = ("joint_rot", "root_pos", "ball_pos", "target_pos", "phase", "swing_type_cycle")


def eval_settings(episode_length=600, body_of_smpl=None):
    """The settings of `v2p_tennis_eval_step` on top of task_settings(...), as a plain dict.  episode_length: cfg env.episodeLength
    (mvae_controller_vis.py:66, default 600); body_of_smpl [24]: `_mujoco_2_smpl`, the engine's body of SMPL joint s - the record needs it."""
    if body_of_smpl is not None:
        body_of_smpl = tuple(int(b) for b in body_of_smpl)
        if sorted(body_of_smpl) != list(range(24)) or body_of_smpl[0] != 0:
            raise ValueError("eval_settings: body_of_smpl must be a permutation of 0..23 with the root first")
    return dict(episode_length=int(episode_length), body_of_smpl=body_of_smpl)


def meters_reset(n):
    """The four meters before their first update (`AverageMeterUnSync.reset`, utils/common.py:46-50) as arrays [4,n]: avg 1, the rest 0."""
    return dict(meter_sum=np.zeros((4, n), _f), meter_count=np.zeros((4, n), np.int64), meter_avg=np.ones((4, n), _f), meter_max=np.zeros((4, n), _f))


def eval_step_reference(st, est, s, dt=np.float32):
    """One evaluation step on arrays: `task_step_reference` with `MVAEControllerVis._compute_reset` (mvae_controller_vis.py:64-79) in
    place of the training law and `_compute_stats` (:81-95) in place of the `_distance` sum.  `est`: eval_settings(...); `s`: the
    arrays of task_step_reference plus the four meter arrays [4,n] (METER_FIELDS, rows in the order of METER_NAMES).  dt float64 states
    the float meter values (bounce error, sums, avg) in double.  Returns every array the step writes; nothing in `s` is modified."""
    A = lambda k, t=None: np.array(s[k], dtype=t)
    o = task_step_reference(dict(st, early_termination=False), s)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        hit, tar_action = o["has_racket_contact"].astype(bool), A("tar_action", np.int64)
        ball, root = A("ball_state", _f), A("rb_state", _f).reshape(len(hit), 24, 13)[:, 0, 0:3]
        terminate = o["progress"] > est["episode_length"]
        in_time = o["tar_time"] >= A("tar_time_total", np.int64)
        reaction = (hit & (tar_action == 0) & A("has_bounce").astype(bool) & in_time) | (~hit & in_time)
        recovery = (tar_action == 1) & (hit | (ball[:, 1] < root[:, 1] - _f(1)) | (np.abs(ball[:, 8]) < _f(2)))
        reaction, recovery = reaction | terminate, recovery & ~terminate
        est_in = o["est_bounce_in"].astype(bool)
        g = o["est_bounce_pos"].astype(dt) - A("target_bounce_pos", dt)
        err = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
        vals = [hit.astype(dt), (A("swing_type_cycle", np.int64) == 1).astype(dt), est_in.astype(dt), err]
        m = {k: A(k, np.int64 if k == "meter_count" else dt) for k in METER_FIELDS}
        for k, (val, on) in enumerate(zip(vals, (recovery, recovery, recovery, recovery & est_in))):
            m["meter_sum"][k] = np.where(on, m["meter_sum"][k] + val, m["meter_sum"][k])
            m["meter_count"][k] += on
            m["meter_avg"][k] = np.where(on, m["meter_sum"][k] / m["meter_count"][k].astype(dt), m["meter_avg"][k])
            m["meter_max"][k] = np.where(on & (val > m["meter_max"][k]), val, m["meter_max"][k])
    o.update(m, reset=terminate.astype(np.int64), terminate=terminate.astype(np.int64), reset_reaction=reaction, reset_recovery=recovery, distance=A("distance", _f))
    return o


def pose_row_reference(body_of_smpl, rb_state, dof_pos, dt=np.float32):
    """`_joint_rot` [n,24,3] of `_update_state_from_sim` with `_is_train` false (humanoid_smpl_im_mvae.py:813-820) from `rb_state`
    [n,24,13] and `dof_pos` [n,69]: joint 0 from the root link's quaternion, joints 1..23 the DoF positions of body_of_smpl[j].  The one
    statement of the device lines in csrc/tennis_pose_dev.hpp, which the evaluation step and the match record share."""
    from ..ref_rotations import quat_to_angle_axis_reference

    rb = np.asarray(rb_state, dtype=_f).reshape(-1, 24, 13)
    n = len(rb)
    root_rot = quat_to_angle_axis_reference(rb[:, 0][:, [6, 3, 4, 5]], dt, wide_atan2=True)  # (as the kernel: one rounding, whatever the library)
    return np.concatenate([root_rot[:, None], np.asarray(dof_pos, dtype=_f).reshape(n, 23, 3).astype(dt)], 1)[:, list(body_of_smpl)]


def eval_record_reference(est, s, dt=np.float32):
    """The frame the evaluation keeps of a step (mvae_controller_vis.py:140-146) on arrays: `_joint_rot` of `_update_state_from_sim` with
    `_is_train` false (humanoid_smpl_im_mvae.py:813-820) from `rb_state` and `dof_pos` [n,69], root, ball and target positions, phase and
    swing type.  Returns a dict under RECORD_NAMES, arrays [n, ...]."""
    if est["body_of_smpl"] is None:
        raise ValueError("eval_record_reference: eval_settings(body_of_smpl=...) is required for the record")
    rb = np.asarray(s["rb_state"], dtype=_f).reshape(-1, 24, 13)
    joints = pose_row_reference(est["body_of_smpl"], rb, s["dof_pos"], dt)
    return dict(joint_rot=joints, root_pos=rb[:, 0, 0:3].copy(), ball_pos=np.array(s["ball_state"], dtype=_f)[:, 0:3], target_pos=np.array(s["target_bounce_pos"], dtype=_f),
                phase=np.array(s["phase_pred"], dtype=_f), swing_type_cycle=np.array(s["swing_type_cycle"], dtype=np.int64))


def eval_structs(est, n, meters, record=None, dof_state=None):
    """(v2p_tennis_eval_cfg, v2p_tennis_eval_buffers) of eval_settings(...), the four meter tensors [4,n] (dict under METER_FIELDS) and,
    for a record, its six tensors [F,n,...] (dict under RECORD_NAMES) with the engine's `dof_state` [n,69,2].  Every size is checked against
    n here: the kernel trusts them."""
    want = dict(meter_sum=torch.float32, meter_count=torch.int64, meter_avg=torch.float32, meter_max=torch.float32)
    for k, dtype in want.items():
        t = meters.get(k)
        if t is None:
            raise ValueError("evaluation step: meter array %s is missing" % k)
        if not t.is_cuda or not t.is_contiguous() or t.dtype != dtype or tuple(t.shape) != (4, n):
            raise RuntimeError("evaluation step: %s must be a contiguous %s GPU tensor [4,%d] (there is no CPU path)" % (k, dtype, n))
    ec = _lib.TennisEvalCfg(episode_length=est["episode_length"], num_frames=0)
    x = _lib.TennisEvalBuffers()
    for k in METER_FIELDS:
        getattr(x, k)[:] = [meters[k][i].data_ptr() for i in range(4)]
    if record is not None:
        if est["body_of_smpl"] is None or dof_state is None:
            raise ValueError("evaluation step: a record needs eval_settings(body_of_smpl=...) and the engine's dof_state")
        F = int(record["phase"].shape[0])
        shapes = dict(joint_rot=(F, n, 24, 3), root_pos=(F, n, 3), ball_pos=(F, n, 3), target_pos=(F, n, 3), phase=(F, n), swing_type_cycle=(F, n), dof_state=(n * 69, 2))
        for k, t in list(record.items()) + [("dof_state", dof_state)]:
            if not t.is_cuda or not t.is_contiguous() or t.dtype != (torch.int64 if k == "swing_type_cycle" else torch.float32):
                raise RuntimeError("evaluation step: %s must be a contiguous GPU tensor of its type (there is no CPU path)" % k)
            if t.numel() != int(np.prod(shapes[k])) or (k != "dof_state" and tuple(t.shape) != shapes[k]):
                raise ValueError("evaluation step: %s is %s, not %s" % (k, tuple(t.shape), shapes[k]))
        ec.num_frames = F
        ec.body_of_smpl[:] = est["body_of_smpl"]
        x.dof_state = dof_state.data_ptr()
        for k in RECORD_NAMES:
            setattr(x, k, record[k].data_ptr())
    return ec, x


def launch_eval_step(st, est, tensors, n, meters, record=None, dof_state=None, frame=0, structs=None):
    """v2p_tennis_eval_step on a dict of device tensors named like v2p_tennis_buffers; returns the names string of the reward law.
    structs: what `eval_structs` made of the same meters and record before (a caller that steps every frame keeps it)."""
    lib = _lib.load()
    ec, x = structs or eval_structs(est, int(n), meters, record, dof_state)  # (refusals first: nothing below touches a device)
    c = cfg_struct(st, tensors["traj_out_x"].shape, tensors["traj_out_y"].shape)
    b = buffers_struct(tensors)
    names = C.c_char_p()
    dev = tensors["obs"].device
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_tennis_eval_step(C.byref(c), C.byref(ec), int(n), C.byref(b), C.byref(x), int(frame), C.byref(names), _lib.current_stream(dev)),
                   "v2p_tennis_eval_step")
    return names.value.decode()


# ------------------------------------------------------------------------------------------------------------------ the actions
def action_settings(num_res_dof=0, num_res_root=0, vae_action_scale=1.0, residual_dof_scale=0.1, residual_root_scale=0.02, random_walk=True, clamp=5.0, seed=0):
    """The settings of `v2p_controller_actions` as a plain dict (defaults: the reference's, physics_mvae_controller.py:249-266)."""
    if num_res_dof < 0 or num_res_root < 0:
        raise ValueError("action_settings: negative column counts")
    return dict(num_res_dof=int(num_res_dof), num_res_root=int(num_res_root), vae_action_scale=float(vae_action_scale), residual_dof_scale=float(residual_dof_scale),
                residual_root_scale=float(residual_root_scale), random_walk=bool(random_walk), clamp=float(clamp), seed=int(seed) & (2 ** 64 - 1))


def action_width(st):
    return LATENT + st["num_res_dof"] + st["num_res_root"]


def action_outputs(st, n, **kw):
    """The four output tensors of `v2p_controller_actions` for n envs (rows of zero width are kept as empty tensors)."""
    return dict(actions_out=torch.zeros((n, action_width(st)), **kw), mvae_actions=torch.zeros((n, LATENT), **kw),
                res_dof_actions=torch.zeros((n, st["num_res_dof"]), **kw), res_root_actions=torch.zeros((n, st["num_res_root"]), **kw))


def launch_actions(st, n, actions, tar_action, out, call=0, words=None):
    """v2p_controller_actions on device tensors: `actions` [>= n, W] float32 with unit column stride (rows may be strided), `tar_action`
    [n] int64, `out` the dict of action_outputs; `words` [n,32] int32 / uint32 bits stands in for the generator's words."""
    lib = _lib.load()
    dev = out["mvae_actions"].device
    for k, t in list(out.items()) + [("tar_action", tar_action), ("words", words)]:
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.device != dev):
            raise RuntimeError("controller actions: buffer %s must be a contiguous tensor on %s (there is no CPU path)" % (k, dev))
    if not actions.is_cuda or actions.device != dev or actions.dtype != torch.float32 or actions.dim() != 2 or actions.stride(1) != 1:
        raise RuntimeError("controller actions: actions must be float32 rows on %s with unit column stride (there is no CPU path)" % (dev,))
    c = _lib.ControllerActionsCfg(num_res_dof=st["num_res_dof"], num_res_root=st["num_res_root"], random_walk=int(st["random_walk"]),
                                  vae_action_scale=st["vae_action_scale"], residual_dof_scale=st["residual_dof_scale"], residual_root_scale=st["residual_root_scale"],
                                  clamp=st["clamp"], seed=st["seed"], call=int(call) & (2 ** 64 - 1))
    nul = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    b = _lib.ControllerActionsBuffers(actions=nul(actions), actions_stride=int(actions.stride(0)) if actions.shape[0] > 1 else int(actions.shape[1]),
                                      tar_action=nul(tar_action), words=nul(words), actions_out=nul(out["actions_out"]), mvae_actions=nul(out["mvae_actions"]),
                                      res_dof_actions=nul(out["res_dof_actions"]), res_root_actions=nul(out["res_root_actions"]))
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_controller_actions(C.byref(c), int(n), C.byref(b), _lib.current_stream(dev)), "v2p_controller_actions")


def controller_actions_reference(st, actions, tar_action, words, dt=np.float32):
    """The action part of pre_physics_step (:247-266) on arrays: `actions` [n, >= width], `tar_action` [n], `words` [n,32] uint32 (the
    generator's: `device_rng.philox_words(seed, call, STREAM_WALK, n, 8)`).  dt float64 is the same law in double (the scatter of the
    normals).  Returns the four arrays `v2p_controller_actions` writes."""
    from .. import device_rng

    a = np.asarray(actions, dtype=np.float32)
    nr, nroot = st["num_res_dof"], st["num_res_root"]
    z = a[:, :LATENT].astype(dt) * dt(st["vae_action_scale"])
    if st["random_walk"]:
        walk = np.asarray(tar_action) == 0
        z[walk] = device_rng.clamped_normals(np.asarray(words, dtype=np.uint32)[walk], st["clamp"], dt)
    return dict(actions_out=a[:, :LATENT + nr + nroot].copy(), mvae_actions=z, res_dof_actions=a[:, LATENT:LATENT + nr].astype(dt) * dt(st["residual_dof_scale"]),
                res_root_actions=a[:, LATENT + nr:LATENT + nr + nroot].astype(dt) * dt(st["residual_root_scale"]))


# ------------------------------------------------------------------------------------------------------------------ the task reset
RESET_WRITES = ("ball_state", "has_bounce", "bounce_pos", "has_racket_contact", "ball_traj", "traj_cursor", "prev_ball_vy", "tar_action", "tar_time", "tar_time_total",
                "num_reset_reaction", "bounce_in", "est_bounce_pos", "est_bounce_time", "est_bounce_in", "est_max_height", "swing_type_cycle", "target_bounce_pos",
                "ball_obs", "sample_idx", "obs", "racket_pos", "racket_normal")  # what v2p_tennis_task_reset may write
RESET_WORDS = 8  # words of an env per call: pool row, near offset, reaction-time offset, target uniform, the whole call's three target uniforms, one spare


def reset_settings(reset_reaction_nframes, use_random_ball_target=False, sample_random=True, target_min=(-3.0, 9.0, 0.0), target_max=(3.0, 11.0, 0.0), seed=0):
    """The settings of `v2p_tennis_task_reset` on top of task_settings(...), as a plain dict (target bounds: :84-85)."""
    mode = use_random_ball_target if use_random_ball_target == "continuous" else bool(use_random_ball_target)
    return dict(reset_reaction_nframes=int(reset_reaction_nframes), target_mode=mode, pool_rule="random" if sample_random else "round_robin",
                target_min=tuple(float(x) for x in target_min), target_max=tuple(float(x) for x in target_max), seed=int(seed) & (2 ** 64 - 1))


def launch_reset(st, tensors, n, pool, num_reset_reaction, sample_idx=None, call=0, words=None):
    """v2p_tennis_task_reset on a dict of device tensors named like v2p_tennis_buffers; `st`: task_settings merged with reset_settings;
    `pool` [rows, 7 + 3 frames] float32, `num_reset_reaction` [n] int64, `sample_idx` [n] int64 (round robin), `words` [n,8] int32 bits."""
    lib = _lib.load()
    tx, ty = tensors.get("traj_out_x"), tensors.get("traj_out_y")
    c = cfg_struct(st, (1, 1) if tx is None else tx.shape, (1, 1, 2) if ty is None else ty.shape)
    b = buffers_struct(tensors)
    dev = tensors["obs"].device
    extra = dict(pool=pool, num_reset_reaction=num_reset_reaction, sample_idx=sample_idx, words=words)
    for k, t in extra.items():
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.device != dev):
            raise RuntimeError("tennis task reset: buffer %s must be a contiguous tensor on %s (there is no CPU path)" % (k, dev))
    if pool.dim() != 2 or pool.dtype != torch.float32 or (pool.shape[1] - 7) % 3:
        raise ValueError("tennis task reset: the pool must be float32 [rows, 7 + 3 frames]")
    rc = _lib.TennisResetCfg(reset_reaction_nframes=st["reset_reaction_nframes"], target_mode=_lib.TENNIS_TARGET_MODES[st["target_mode"]],
                             pool_rule=_lib.TENNIS_POOL_RULES[st["pool_rule"]], pool_rows=int(pool.shape[0]), pool_frames=min((int(pool.shape[1]) - 7) // 3, TRAJ_FRAMES),
                             pool_stride=int(pool.shape[1]), seed=st["seed"], call=int(call) & (2 ** 64 - 1))
    rc.target_min[:] = st["target_min"]
    rc.target_max[:] = st["target_max"]
    shared = {k: tensors.get(k) for k in _lib.TENNIS_RESET_BUFFER_NAMES if k not in extra}
    r = _lib.TennisResetBuffers(**{k: t.data_ptr() for k, t in dict(shared, **extra).items() if t is not None})
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_tennis_task_reset(C.byref(c), C.byref(rc), int(n), C.byref(b), C.byref(r), _lib.current_stream(dev)), "v2p_tennis_task_reset")


def task_reset_reference(st, s, words):
    """The flag-driven half of `_reset_envs` (:167-242 with `_reset_balls` and `TennisBallGeneratorOffline.generate`) on arrays, numpy
    float32.  `st`: task_settings merged with reset_settings; `s`: arrays named like v2p_tennis_buffers plus `pool` [rows, 7 + 3 F],
    `num_reset_reaction` and, for the round robin, `sample_idx`; `words` [n,8] uint32: `device_rng.philox_words(seed, call, STREAM_RESET,
    n, 1)` in columns 0..3 and, for the continuous target, the whole call's block in columns 4..7 of every row.  Returns every array the
    launch may write (RESET_WRITES) and `pool_rows`, the row each reacting env drew (-1 elsewhere).  Nothing in `s` is modified."""
    from .. import device_rng as R

    n = len(s["ball_state"])
    A = lambda k, dt=None: np.array(s[k], dtype=dt)
    w = np.asarray(words, dtype=np.uint32).reshape(n, RESET_WORDS)
    rx, rc = A("reset_reaction").astype(bool), A("reset_recovery").astype(bool)
    pool = np.asarray(s["pool"], dtype=_f)
    rows, frames = len(pool), min((pool.shape[1] - 7) // 3, TRAJ_FRAMES)
    L = st["L"]
    o = dict(ball_state=A("ball_state", _f), has_bounce=A("has_bounce").astype(bool), bounce_pos=A("bounce_pos", _f), has_racket_contact=A("has_racket_contact").astype(bool),
             ball_traj=A("ball_traj", _f).reshape(n, TRAJ_FRAMES, 3), traj_cursor=A("traj_cursor", np.int32), prev_ball_vy=A("prev_ball_vy", _f),
             tar_action=A("tar_action", np.int64), tar_time=A("tar_time", np.int64), tar_time_total=A("tar_time_total", np.int64),
             num_reset_reaction=A("num_reset_reaction", np.int64), bounce_in=A("bounce_in").astype(bool), est_bounce_pos=A("est_bounce_pos", _f),
             est_bounce_time=A("est_bounce_time", _f), est_bounce_in=A("est_bounce_in").astype(bool), est_max_height=A("est_max_height", _f),
             swing_type_cycle=A("swing_type_cycle", np.int64), target_bounce_pos=A("target_bounce_pos", _f), obs=A("obs", _f), racket_pos=A("racket_pos", _f),
             racket_normal=A("racket_normal", _f))
    if s.get("ball_obs") is not None:
        o["ball_obs"] = A("ball_obs", _f).reshape(n, L, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # ---- TennisBallGeneratorOffline.indices
        if st["pool_rule"] == "round_robin":
            o["sample_idx"] = A("sample_idx", np.int64)
            idx = np.clip(o["sample_idx"], 0, rows - 1)
            o["sample_idx"][rx] = (idx[rx] + 1) % rows
        else:
            idx = R.integer(w[:, 0], 0, rows)
            x, y = o["ball_state"][:, 0], o["ball_state"][:, 1]
            nf = (x + _f(4)) / _f(8) * _f(rows)
            base = np.where((nf >= _f(-1e15)) & (nf <= _f(1e15)), nf, _f(-1e15)).astype(np.int64)  # (trunc toward zero, as .long())
            idx = np.where(y > 0, np.clip(base + R.integer(w[:, 1], -1000, 1000), 0, rows - 1), idx)
        # ---- reset_balls and the trajectory row
        row = pool[idx]
        vel, vspin = row[:, 3:6], row[:, 6]
        cr = np.stack([vel[:, 1] * _f(-1) - vel[:, 2] * _f(0), vel[:, 2] * _f(0) - vel[:, 0] * _f(-1), vel[:, 0] * _f(0) - vel[:, 1] * _f(0)], -1)
        nrm = np.maximum(np.sqrt(cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1] + cr[:, 2] * cr[:, 2]), _f(1e-12))
        mag = vspin * _f(math.pi) * _f(2)
        state = np.concatenate([row[:, 0:3], np.tile(np.array([0, 0, 0, 1], _f), (n, 1)), vel, mag[:, None] * (cr / nrm[:, None])], 1).astype(_f)
        o["ball_state"][rx] = state[rx]
        o["has_bounce"][rx], o["bounce_pos"][rx], o["has_racket_contact"][rx] = False, 0, False
        o["ball_traj"][rx] = 0
        o["ball_traj"][rx, :frames] = row[rx, 7:7 + 3 * frames].reshape(-1, frames, 3)
        o["traj_cursor"][rx] = 0
        o["prev_ball_vy"][rx] = state[rx, 8]
        # ---- _reset_recovery_tasks, then _reset_reaction_tasks
        o["tar_action"][rc] = 0
        o["has_bounce"][rc], o["bounce_pos"][rc] = False, 0
        if st["use_history"]:
            o["ball_obs"][rx] = o["ball_state"][rx, None, 0:3]
        o["tar_time"][rx], o["tar_action"][rx] = 0, 1
        o["num_reset_reaction"][rx] += 1
        o["bounce_in"][rx], o["est_bounce_pos"][rx], o["est_bounce_time"][rx], o["est_bounce_in"][rx], o["est_max_height"][rx] = False, 0, 0, False, 0
        o["swing_type_cycle"][rx] = -1
        o["tar_time_total"][rx] = st["reset_reaction_nframes"] + R.integer(w[rx, 2], -5, 5)
        if st["target_mode"] == "continuous":
            lo, hi = np.array(st["target_min"], _f), np.array(st["target_max"], _f)
            o["target_bounce_pos"][rx] = R.uniform(w[rx, 4:7]) * (hi - lo) + lo
        elif st["target_mode"]:
            u = R.uniform(w[rx, 3])
            o["target_bounce_pos"][rx] = np.stack([np.where(u < _f(0.33), _f(-3), np.where(u > _f(0.67), _f(3), _f(0))), np.full_like(u, 10), np.zeros_like(u)], -1)
        # ---- the observation of the flagged envs on the new state
        ids = np.nonzero(rx | rc)[0]
        if len(ids):
            s2 = dict(s, **{k: v for k, v in o.items() if k in ("ball_state", "ball_traj", "traj_cursor", "target_bounce_pos", "ball_obs")})
            obs, hist, rpos, rnorm = observation_reference(st, s2, ids)
            o["obs"][ids], o["racket_pos"][ids], o["racket_normal"][ids] = obs, rpos, rnorm
            if hist is not None:
                o["ball_obs"][ids] = hist
    o["pool_rows"] = np.where(rx, idx, -1)
    return o


# ------------------------------------------------------------------------------------------------------------------ the task
class TennisControllerTask:
    """`PhysicsMVAEController` without the MVAE player, on top of a single-player `HumanoidSMPLIMRacketBall`.  Attribute names are the
    reference's.  cfg: `cfg["env"]` (episodeLength, enableEarlyTermination) and `cfg["v2p"]` (reward_type / _weights / _scales, court_min /
    _max, obs_ball_traj_length, use_history_ball_obs, use_random_ball_target, reset_reaction_nframes, grip, ball_traj_out_x_file / _y_file -
    file names or arrays).  `_ball_traj` [N,100,3] holds every env's drawn trajectory as it was drawn; `_ball_traj_cursor` [N] is the
    first frame of its window (the reference rolls the tensor instead, :365-366): `ball_traj_window()` gives the rolled view."""

    def __init__(self, task, cfg, params=traj_out_params, seed=None):
        env, v2p = dict(cfg.get("env") or {}), dict(cfg.get("v2p") or {})
        self._check_mode(task, v2p)
        if not hasattr(task, "_ball_root_states"):
            raise TypeError("TennisControllerTask wraps a HumanoidSMPLIMRacketBall")
        dev = torch.device(task.device)
        if dev.type != "cuda":
            raise RuntimeError("TennisControllerTask: the task step is a HIP kernel - the wrapped task must live on a GPU (no CPU fallback)")
        _lib.load()
        for key in ("court_min", "court_max", "reset_reaction_nframes"):
            if key not in v2p:
                raise ValueError("TennisControllerTask: cfg v2p.%s is required" % key)
        self.task, self.cfg, self.cfg_v2p, self.device, self.num_envs = task, cfg, v2p, dev, task.num_envs
        self._max_episode_length = int(env["episodeLength"])
        self._enable_early_termination = bool(env.get("enableEarlyTermination", False))
        self.settings = task_settings(reward_type=v2p.get("reward_type", "return"), obs_ball_traj_length=v2p.get("obs_ball_traj_length", 100),
                                      use_history_ball_obs=v2p.get("use_history_ball_obs", False), use_random_ball_target=v2p.get("use_random_ball_target", False),
                                      contact_by_velocity=task.sim_params.substeps > 2, enable_early_termination=self._enable_early_termination,
                                      max_episode_length=self._max_episode_length, grip=self._grip(v2p), court_min=v2p["court_min"], court_max=v2p["court_max"],
                                      reward_scales=v2p.get("reward_scales"), reward_weights=v2p.get("reward_weights"), grids=grids_of(params))
        st = self.settings
        self._obs_ball_traj_length = st["L"]
        n = self.num_envs
        f, i64, bl = dict(dtype=torch.float32, device=dev), dict(dtype=torch.long, device=dev), dict(dtype=torch.bool, device=dev)
        load = lambda t: torch.from_numpy(np.load(t) if isinstance(t, str) else np.ascontiguousarray(t)).to(**f).contiguous()
        self._load_tables(v2p, load)
        self.num_obs = obs_width(st)
        self.obs_buf = torch.zeros((n, self.num_obs), **f)
        self.rew_buf = torch.zeros(n, **f)
        self.reset_buf = torch.ones(n, **i64)
        self.progress_buf = torch.zeros(n, **i64)
        self._terminate_buf = torch.ones(n, **i64)
        self.extras = {}
        self._sub_rewards = torch.zeros((n, num_sub_rewards(st)), **f)
        self._sub_rewards_names = SUB_REWARD_NAMES[st["reward_type"]]
        self._racket_pos, self._racket_normal = torch.zeros((n, 3), **f), torch.zeros((n, 3), **f)
        self._ball_traj = torch.zeros((n, TRAJ_FRAMES, 3), **f)
        self._ball_traj_cursor = torch.zeros(n, dtype=torch.int32, device=dev)
        self._ball_obs = torch.zeros((n, st["L"], 3), **f)
        self._bounce_in = torch.zeros(n, **bl)
        self._est_bounce_pos, self._est_bounce_time = torch.zeros((n, 3), **f), torch.zeros(n, **f)
        self._est_bounce_in, self._est_max_height = torch.zeros(n, **bl), torch.zeros(n, **f)
        self._tar_time, self._tar_time_total, self._tar_action = torch.zeros(n, **i64), torch.zeros(n, **i64), torch.zeros(n, **i64)
        self._target_bounce_pos = torch.zeros((n, 3), **f)
        self._target_bounce_pos[:] = torch.tensor([0.0, 10.0, 0.0], **f)
        self._target_bounce_min, self._target_bounce_max = torch.tensor([-3.0, 9.0, 0.0], **f), torch.tensor([3.0, 11.0, 0.0], **f)
        self._reset_reaction_buf, self._reset_recovery_buf = torch.ones(n, **bl), torch.zeros(n, **bl)  # all envs start with a reaction task
        self._num_reset_reaction, self._num_reset = torch.zeros(n, **i64), torch.zeros(n, **i64)
        self._distance = torch.zeros(n, **f)
        self._prev_ball_vy = torch.zeros(n, **f)
        self.vel_x_overflow = torch.zeros(1, **i64)
        self._phase_pred, self._swing_type, self._swing_type_cycle = torch.zeros(n, **f), torch.zeros(n, **i64), torch.full((n,), -1, **i64)
        wl = task._racket_wrist_body_id
        self._wrist_link = (wl.to(**i64) if torch.is_tensor(wl) else torch.full((n,), int(wl), **i64)).contiguous()
        self._has_init = False
        self._mvae_player = None
        self._imitation_target = None
        self._ll_policy = None
        self._num_res_root_action = 0
        self._res_root_actions = None
        # the device generator's key and the count of `v2p_controller_actions` launches: host numbers, never read back from the device
        self.seed = int((cfg.get("params") or {}).get("seed", 0) if seed is None else seed) & (2 ** 64 - 1)
        self._walk_calls = 0
        self._walk_buffers = None
        # cfg v2p.task_reset: 'torch' (default) is the reference's indexed torch code, random stream and all; 'device' is one launch
        self._task_reset = v2p.get("task_reset", "torch")
        if self._task_reset not in ("torch", "device"):
            raise ValueError("TennisControllerTask: cfg v2p.task_reset %r is neither 'torch' nor 'device'" % (self._task_reset,))
        self._reset_calls = 0
        self._no_ids = torch.zeros(0, **i64)
        self._reset_root_xy = None  # [N,2]: a per-env start that stands in for the generator's draw, in `reset(env_ids)` and `reset_by_flags()` alike
        if self._task_reset == "device":
            self._init_device_reset(v2p)

    def _init_device_reset(self, v2p):
        from ..ball_traj import TennisBallGeneratorOffline

        gen = getattr(self.task, "_ball_generator", None)
        if not isinstance(gen, TennisBallGeneratorOffline) or torch.device(gen.device) != self.device:
            raise NotImplementedError("TennisControllerTask: cfg v2p.task_reset 'device' draws from the pool of a TennisBallGeneratorOffline on %s "
                                      "(cfg v2p.ball_traj_file); the task's ball generator is %s" % (self.device, "none" if gen is None else
                                                                                                   "%s on %s" % (type(gen).__name__, gen.device)))
        self._pool = gen.data.contiguous()
        self.reset_settings = reset_settings(v2p["reset_reaction_nframes"], v2p.get("use_random_ball_target", False), gen.sample_random,
                                             tuple(self._target_bounce_min.tolist()), tuple(self._target_bounce_max.tolist()), self.seed)

    def _check_mode(self, task, v2p):
        if v2p.get("dual_mode") or getattr(task, "racket_players", None) is not None:
            raise NotImplementedError("TennisControllerTask: dual_mode (the two-player controller and its ball hand-over) is not built here: "
                                      "tasks.tennis_controller_dual.DualTennisControllerTask")

    def _grip(self, v2p):
        return v2p.get("grip", "eastern")

    def _load_tables(self, v2p, load):
        self._ball_traj_out_x = load(v2p.get("ball_traj_out_x_file", "vid2player/data/ball_traj_out_x_v0.npy"))
        self._ball_traj_out_y = load(v2p.get("ball_traj_out_y_file", "vid2player/data/ball_traj_out_y_v0.npy"))
        if self._ball_traj_out_x.dim() != 2 or self._ball_traj_out_y.dim() != 3 or len(self._ball_traj_out_x) != len(self._ball_traj_out_y):
            raise ValueError("the outgoing tables must be [B,nx] and [B,ny,2]")

    def _launch_step(self):
        return launch_step(self.settings, self._tensors(), self.num_envs)

    # ------------------------------------------------------------------ the motion generator
    def attach_motion_generator(self, player):
        """Make `player` (a `MotionVAEPlayer` of this batch) the `_mvae_player` of the controller.  Its phase and swing-type tensors become
        the task's: the step kernel reads what the generator wrote, and the `-1` a reaction reset puts into `_swing_type_cycle`
        (physics_mvae_controller.py:223) reaches the player."""
        if player.num_envs != self.num_envs or torch.device(player.device) != self.device:
            raise ValueError("attach_motion_generator: the player has %d envs on %s, the task %d on %s" % (player.num_envs, player.device, self.num_envs, self.device))
        self._refuse_unbuilt()
        if bool(self.cfg_v2p.get("add_residual_dof")) != player.settings["add_residual_dof"]:
            raise ValueError("attach_motion_generator: cfg v2p.add_residual_dof and the player's disagree")
        if self._imitation_target is not None and self._imitation_target.player is not player:
            raise ValueError("attach_motion_generator: the attached imitation target belongs to another player")
        self._mvae_player = player
        self._phase_pred, self._swing_type, self._swing_type_cycle = player._phase_pred, player._swing_type, player._swing_type_cycle
        self._num_mvae_action, self._num_res_dof_action = LATENT, 3 if player.settings["add_residual_dof"] else 0

    def _refuse_unbuilt(self):
        """(`add_residual_root` moves the target's root: it needs an imitation target, attached before the step - or before the generator)"""
        if self.cfg_v2p.get("add_residual_root") and self._imitation_target is None:
            raise NotImplementedError("TennisControllerTask: add_residual_root is not built without an imitation target (attach_imitation_target)")

    def attach_imitation_target(self, target):
        """Make `target` (an `ImitationTarget` around the wrapped task and the motion generator of this batch) the physics player's task
        side of `post_mvae_step` (:264-269), of the pose reset and of the PD targets.  With cfg v2p.add_residual_root attach it before the
        motion generator; its three action columns follow the latent and the residual DoFs."""
        if target.task is not self.task:
            raise ValueError("attach_imitation_target: the target wraps another task")
        if self._mvae_player is not None and target.player is not self._mvae_player:
            raise ValueError("attach_imitation_target: the target belongs to another player than the attached motion generator")
        if bool(self.cfg_v2p.get("add_residual_root")) != target.settings["add_residual_root"]:
            raise ValueError("attach_imitation_target: cfg v2p.add_residual_root and the target's disagree")
        self._imitation_target = target
        self._num_res_root_action = 3 if target.settings["add_residual_root"] else 0

    def attach_low_level_policy(self, policy):
        """Make `policy` (a `policies.LowLevelPolicy` around the attached imitation target) the physics player's network: `physics_step()`
        without an argument then takes its actions, and the imitation observation is computed by the policy's input launch."""
        if self._imitation_target is None or policy.target is not self._imitation_target:
            raise ValueError("attach_low_level_policy: the policy wraps another imitation target than the attached one (attach_imitation_target first)")
        self._ll_policy = policy

    def get_action_size(self):
        if self._mvae_player is None:
            raise RuntimeError("TennisControllerTask: no motion generator is attached")
        return self._num_mvae_action + self._num_res_dof_action + self._num_res_root_action

    def pre_physics_step(self, actions):
        """pre_physics_step (:247-263): the latent and the residual-DoF part of the policy's actions, scaled, drive one step of the motion
        generator; with an imitation target attached `post_mvae_step()` then hands the pose to the physics task (:264-269)."""
        if self._mvae_player is None:
            raise RuntimeError("TennisControllerTask.pre_physics_step: no motion generator is attached (attach_motion_generator)")
        self._refuse_unbuilt()
        nz, nr, nroot = self._num_mvae_action, self._num_res_dof_action, self._num_res_root_action
        if actions.dim() != 2 or actions.shape[0] != self.num_envs or actions.shape[1] < nz + nr + nroot:
            raise ValueError("pre_physics_step: actions must be [%d, >= %d]" % (self.num_envs, nz + nr + nroot))
        if self.cfg_v2p.get("random_walk_in_recovery"):
            self._launch_actions(actions)
            self._mvae_player.step(self._mvae_actions, self._res_dof_actions)
            if self._imitation_target is not None:
                self.post_mvae_step()
            return
        self._actions = actions.clone()
        self._mvae_actions = actions[:, :nz].clone() * self.cfg_v2p.get("vae_action_scale", 1.0)
        self._res_dof_actions = torch.empty(0, device=self.device)
        if nr:
            self._res_dof_actions = actions[:, nz:nz + nr].clone() * self.cfg_v2p.get("residual_dof_scale", 0.1)
        self._mvae_player.step(self._mvae_actions, self._res_dof_actions)
        if self._imitation_target is not None:
            self._res_root_actions = None
            if nroot:
                self._res_root_actions = actions[:, nz + nr:nz + nr + nroot].clone() * self._imitation_target.settings["residual_root_scale"]
            self.post_mvae_step()

    def action_settings(self):
        """What `v2p_controller_actions` and `controller_actions_reference` are made from, of the cfg and what is attached."""
        root_scale = self._imitation_target.settings["residual_root_scale"] if self._num_res_root_action else 0.0
        return action_settings(num_res_dof=self._num_res_dof_action, num_res_root=self._num_res_root_action,
                               vae_action_scale=self.cfg_v2p.get("vae_action_scale", 1.0), residual_dof_scale=self.cfg_v2p.get("residual_dof_scale", 0.1),
                               residual_root_scale=root_scale, random_walk=self.cfg_v2p.get("random_walk_in_recovery", False), seed=self.seed)

    def _launch_actions(self, actions):
        """`_actions`, `_mvae_actions`, `_res_dof_actions`, `_res_root_actions` of this step in one launch, into tensors allocated once;
        the call counter advances by one per launch."""
        st = self.action_settings()
        key = (st["num_res_dof"], st["num_res_root"])
        if self._walk_buffers is None or self._walk_buffers[0] != key:
            f = dict(dtype=torch.float32, device=self.device)
            self._walk_buffers = (key, action_outputs(st, self.num_envs, **f))
        out = self._walk_buffers[1]
        launch_actions(st, self.num_envs, actions, self._tar_action, out, call=self._walk_calls)
        self._walk_calls += 1
        self._actions, self._mvae_actions = out["actions_out"], out["mvae_actions"]
        self._res_dof_actions = out["res_dof_actions"] if st["num_res_dof"] else torch.empty(0, device=self.device)
        self._res_root_actions = out["res_root_actions"] if st["num_res_root"] and self._imitation_target is not None else None

    def post_mvae_step(self):
        """`HumanoidSMPLIMMVAE.post_mvae_step` (humanoid_smpl_im_mvae.py:593-598): the new imitation target and the low-level policy's
        observation (`_imitation_target.obs_buf`)."""
        if self._imitation_target is None:
            raise RuntimeError("TennisControllerTask.post_mvae_step: no imitation target is attached (attach_imitation_target)")
        if self._num_res_root_action and self._res_root_actions is None:
            raise RuntimeError("TennisControllerTask.post_mvae_step: add_residual_root needs the actions of a pre_physics_step first")
        self._imitation_target.step(self._res_root_actions)
        if self._ll_policy is None:  # (an attached policy computes the observation in its own input launch, from the same state)
            self._imitation_target.compute_observations()

    def physics_step(self, ll_actions=None):
        """The physics player's control step on the low-level policy's actions [N,75]: `_action_to_pd_targets` (the engine clamps), then
        the wrapped task's step.  Without an argument the attached low-level policy makes the actions (`ImitatorPlayer.run_one_step`)."""
        if self._imitation_target is None:
            raise RuntimeError("TennisControllerTask.physics_step: no imitation target is attached (attach_imitation_target)")
        if ll_actions is None:
            if self._ll_policy is None:
                raise RuntimeError("TennisControllerTask.physics_step: no low-level policy is attached (attach_low_level_policy) and no actions are given")
            self.task.step(self._ll_policy.step())
            return
        self.task.step(self._imitation_target.actions(ll_actions))

    def step(self, actions):
        """`PhysicsMVAEController.step(actions)` (:244-246 with the base task's step): pre_physics_step -> physics_step ->
        post_physics_step with the attached generator, target and low-level policy.  Returns (obs_buf, rew_buf, reset_buf, extras)."""
        self.pre_physics_step(actions)
        self.physics_step()
        self.post_physics_step()
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras

    # ------------------------------------------------------------------ sizes
    def get_actor_obs_size(self):
        return NUM_ACTOR_OBS

    def get_task_obs_size(self):
        return 3 * self.settings["L"] + (2 if self.settings["use_target"] else 0)

    def ball_traj_window(self):
        """The reference's rolled `_ball_traj`: frame k of the view is frame cursor + k of the drawn trajectory, zeros past its end."""
        idx = self._ball_traj_cursor.long().view(-1, 1) + torch.arange(TRAJ_FRAMES, device=self.device).view(1, -1)
        padded = torch.cat([self._ball_traj, torch.zeros_like(self._ball_traj)], 1)
        return padded[torch.arange(self.num_envs, device=self.device).view(-1, 1), idx.clamp(max=2 * TRAJ_FRAMES - 1)]

    def _tensors(self):
        t, rb = self.task, self.task._rigid_body_state
        return dict(rb_state=rb, root_states=t._humanoid_root_states, racket_state=t._racket_rb_state, ball_state=t._ball_root_states, wrist_link=self._wrist_link,
                    has_bounce=t._has_bounce, has_bounce_now=t._has_bounce_now, bounce_pos=t._bounce_pos, phase_pred=self._phase_pred, swing_type=self._swing_type,
                    swing_type_cycle=self._swing_type_cycle, traj_out_x=self._ball_traj_out_x, traj_out_y=self._ball_traj_out_y, tar_time_total=self._tar_time_total,
                    tar_action=self._tar_action, target_bounce_pos=self._target_bounce_pos, ball_traj=self._ball_traj, has_racket_contact=t._has_racket_ball_contact,
                    has_racket_contact_now=t._has_racket_ball_contact_now, tar_time=self._tar_time, progress=self.progress_buf, prev_ball_vy=self._prev_ball_vy,
                    traj_cursor=self._ball_traj_cursor, ball_obs=self._ball_obs, bounce_in=self._bounce_in, est_bounce_pos=self._est_bounce_pos,
                    est_bounce_time=self._est_bounce_time, est_max_height=self._est_max_height, est_bounce_in=self._est_bounce_in, distance=self._distance,
                    vel_x_overflow=self.vel_x_overflow, racket_pos=self._racket_pos, racket_normal=self._racket_normal, obs=self.obs_buf, rew=self.rew_buf,
                    sub_rewards=self._sub_rewards, reset=self.reset_buf, terminate=self._terminate_buf, reset_reaction=self._reset_reaction_buf,
                    reset_recovery=self._reset_recovery_buf)

    def state_arrays(self):
        """Every tensor of the step as a numpy array, named like v2p_tennis_buffers (what task_step_reference takes)."""
        return {k: v.detach().cpu().numpy().copy() for k, v in self._tensors().items()}

    # ------------------------------------------------------------------ reset (:167-242, without the MVAE call)
    def reset(self, env_ids=None):
        if env_ids is None:
            if self._has_init and self.num_envs > 1:
                return
            env_ids = torch.arange(self.num_envs, device=self.device, dtype=torch.long)
        if not torch.is_tensor(env_ids) and len(env_ids) == 0:
            env_ids = self._no_ids  # (the rally path: no tensor is made)
        self._reset_envs(torch.as_tensor(env_ids, device=self.device, dtype=torch.long))

    def _reset_envs_device(self, env_ids):
        """`_reset_envs` under cfg v2p.task_reset 'device': the humanoid part for `env_ids` as ever, then `v2p_tennis_task_reset` for all
        envs by their flags, then the two flags of `env_ids` are cleared.  No host read of a device result."""
        some = env_ids.numel() > 0
        if some:
            self._reset_env_tensors(env_ids, keep_flags=True)
            if self._mvae_player is not None:
                self._mvae_player.reset(env_ids, self._root_xy_rows(env_ids))
                if self._imitation_target is not None:
                    self._imitation_target.reset(env_ids)
            self._num_reset[env_ids] += 1
        gen = self.task._ball_generator
        launch_reset(dict(self.settings, **self.reset_settings), self._tensors(), self.num_envs, self._pool, self._num_reset_reaction,
                     sample_idx=None if gen.sample_random else gen.sample_idx, call=self._reset_calls)
        self._reset_calls += 1
        if some:
            self._reset_reaction_buf[env_ids] = False
            self._reset_recovery_buf[env_ids] = False
        self._has_init = True

    def _root_xy_rows(self, env_ids):
        """the rows of the per-env start table `_reset_root_xy` ([N,2], default None: the generator draws) for env_ids"""
        return None if self._reset_root_xy is None else self._reset_root_xy[env_ids]

    def _ctl_reset_buffers(self):
        t = dict(progress=self.progress_buf, terminate=self._terminate_buf, num_reset_reaction=self._num_reset_reaction, num_reset=self._num_reset,
                 distance=self._distance, reset_reaction=self._reset_reaction_buf, reset_recovery=self._reset_recovery_buf)
        for k, v in t.items():
            if not v.is_cuda or not v.is_contiguous() or v.numel() != self.num_envs:
                raise RuntimeError("TennisControllerTask.reset_by_flags: %s must be a contiguous GPU tensor [%d]" % (k, self.num_envs))
        return _lib.CtlResetBuffers(**{k: v.data_ptr() for k, v in t.items()})

    def reset_by_flags(self):
        """`reset(done ids)` for the envs whose `reset_buf` is up, without knowing them on the host: `_reset_envs_device` as ONE fixed
        sequence of launches over all envs, the same whether 0 or N envs are done - `v2p_ctl_reset_begin` (the bookkeeping),
        `v2p_mvae_reset_flagged` (the generator), `v2p_mvae_target_reset_flagged` and `v2p_env_push_state_flagged` (the target and the
        engine), `v2p_tennis_task_reset` (by its own two flags), `v2p_ctl_reset_end` (the two flags of the reset envs, then `reset_buf`).
        No host read of a device result, no id list, no allocation, no torch op.  `_reset_root_xy` [N,2] stands in for the generator's
        draw, as in `reset(env_ids)`; without it the generator's kernel draws (`MotionVAEPlayer.reset_flagged`)."""
        if self._task_reset != "device":
            raise NotImplementedError("TennisControllerTask.reset_by_flags: the reset by flags needs cfg v2p.task_reset 'device' (a flag form of the "
                                      "'torch' task reset is not built); got %r" % (self._task_reset,))
        lib, flags, n = _lib.load(), self.reset_buf, self.num_envs
        if flags.dtype != torch.int64 or not flags.is_contiguous():
            raise RuntimeError("TennisControllerTask.reset_by_flags: reset_buf must be a contiguous int64 tensor")
        b = self._ctl_reset_buffers()
        stream = lambda: _lib.current_stream(self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.v2p_ctl_reset_begin(n, _lib.ptr(flags), C.byref(b), stream()), "v2p_ctl_reset_begin")
        if self._mvae_player is not None:
            self._mvae_player.reset_flagged(flags, self._reset_root_xy)
            if self._imitation_target is not None:
                self._imitation_target.reset_flagged(flags)
        gen = self.task._ball_generator
        launch_reset(dict(self.settings, **self.reset_settings), self._tensors(), n, self._pool, self._num_reset_reaction,
                     sample_idx=None if gen.sample_random else gen.sample_idx, call=self._reset_calls)
        self._reset_calls += 1
        with torch.cuda.device(self.device):
            _lib.check(lib.v2p_ctl_reset_end(n, _lib.ptr(flags), C.byref(b), stream()), "v2p_ctl_reset_end")
        self._has_init = True

    def _reset_envs(self, env_ids):
        if self._task_reset == "device":
            return self._reset_envs_device(env_ids)
        reaction_ids = self._reset_reaction_buf.nonzero(as_tuple=False).flatten()  # (include env_ids)
        recovery_ids = self._reset_recovery_buf.nonzero(as_tuple=False).flatten()
        all_ids = (self._reset_reaction_buf | self._reset_recovery_buf).nonzero(as_tuple=False).flatten()
        if len(env_ids) > 0:
            self._reset_env_tensors(env_ids)
            if self._mvae_player is not None:
                self._mvae_player.reset(env_ids, self._root_xy_rows(env_ids))  # (:182-183)
                if self._imitation_target is not None:
                    self._imitation_target.reset(env_ids)  # (`_reset_actors` of the physics player's task, :186)
            self._num_reset[env_ids] += 1
        if len(reaction_ids) > 0:
            new_traj = self.task.reset_balls(reaction_ids)
            frames = min(new_traj.shape[1], TRAJ_FRAMES)
            self._ball_traj[reaction_ids] = 0
            self._ball_traj[reaction_ids, :frames] = new_traj[:, :frames].to(self.device)
            self._ball_traj_cursor[reaction_ids] = 0
            # (`_reset_balls` refreshes `_ball_vel` with the launch velocity, humanoid_smpl_im_mvae.py:522: the velocity rule's previous vy)
            self._prev_ball_vy[reaction_ids] = self.task._ball_root_states[reaction_ids, 8]
        if len(recovery_ids) > 0:
            self._reset_recovery_tasks(recovery_ids)
        if len(reaction_ids) > 0:
            self._reset_reaction_tasks(reaction_ids)
        if len(all_ids) > 0:
            launch_obs(self.settings, self._tensors(), self.num_envs, all_ids)
        self._has_init = True

    def _reset_env_tensors(self, env_ids, keep_flags=False):
        self.progress_buf[env_ids] = 0
        self.reset_buf[env_ids] = 0
        self._terminate_buf[env_ids] = 0
        if not keep_flags:
            self._reset_reaction_buf[env_ids] = False
            self._reset_recovery_buf[env_ids] = False
        self._num_reset_reaction[env_ids] = 0
        self._distance[env_ids] = 0

    def _reset_reaction_tasks(self, env_ids):
        if self.settings["use_history"]:
            self._ball_obs[env_ids] = self.task._ball_root_states[env_ids, 0:3].view(-1, 1, 3).repeat(1, self._obs_ball_traj_length, 1)
        self._tar_time[env_ids] = 0
        self._tar_action[env_ids] = 1
        self._num_reset_reaction[env_ids] += 1
        self._bounce_in[env_ids] = False
        self._est_bounce_pos[env_ids, :] = 0
        self._est_bounce_time[env_ids] = 0
        self._est_bounce_in[env_ids] = False
        self._est_max_height[env_ids] = 0
        self._swing_type_cycle[env_ids] = -1
        self._tar_time_total[env_ids] = int(self.cfg_v2p["reset_reaction_nframes"]) + torch.randint(-5, 5, (len(env_ids),), device=self.device)
        target = self.cfg_v2p.get("use_random_ball_target")
        if target:
            if target == "continuous":  # (the same target for the envs to be reset)
                self._target_bounce_pos[env_ids] = torch.rand((3,), device=self.device) * (self._target_bounce_max - self._target_bounce_min) + self._target_bounce_min
            else:
                seed = torch.rand((len(env_ids),), device=self.device)
                x = torch.where(seed < 0.33, -3.0, torch.where(seed > 0.67, 3.0, 0.0))
                self._target_bounce_pos[env_ids] = torch.stack([x, torch.full_like(x, 10.0), torch.zeros_like(x)], -1)

    def _reset_recovery_tasks(self, env_ids):
        self._tar_action[env_ids] = 0
        self.task._has_bounce[env_ids] = False
        self.task._bounce_pos[env_ids] = 0

    # ------------------------------------------------------------------ the step
    def post_physics_step(self, phase_pred=None, swing_type=None, swing_type_cycle=None):
        """post_physics_step (:441-452) and the roll of physics_step (:365-366) after the wrapped task has stepped its physics: one kernel
        launch.  phase_pred [N] float, swing_type [N] int: what the motion generator predicts for this step; swing_type_cycle [N] (the
        reaction resets put -1 into the kept copy) is needed by `return_w_estimate` only.  With a motion generator attached the three may
        be left out: its tensors are the task's."""
        if phase_pred is None or swing_type is None:
            if self._mvae_player is None or phase_pred is not None or swing_type is not None:
                raise TypeError("post_physics_step: phase_pred and swing_type are required (both may be left out with a motion generator attached)")
        else:
            self._phase_pred.copy_(phase_pred)
            self._swing_type.copy_(swing_type)
        if swing_type_cycle is not None:
            self._swing_type_cycle.copy_(swing_type_cycle)
        self._sub_rewards_names = self._launch_step()
        self.extras["terminate"] = self._terminate_buf
        self.extras["sub_rewards"] = self._sub_rewards
        self.extras["sub_rewards_names"] = self._sub_rewards_names


# ------------------------------------------------------------------------------------------------------------------ the evaluation
class Meter:
    """One `AverageMeterUnSync` (utils/common.py:34-63) of the evaluation: `.sum`, `.avg`, `.max` float32 and `.count` int64, device
    tensors [N] - rows of the controller's four [4,N] arrays, which the step kernel updates."""

    def __init__(self, sum, count, avg, max):
        self.sum, self.count, self.avg, self.max = sum, count, avg, max


class TennisControllerEval(TennisControllerTask):
    """`MVAEControllerVis` (vid2player/env/tasks/mvae_controller_vis.py, what `run.py --test` builds) without the viewer: the training task
    with the test-mode episode law, the four meters `hit_rate`, `fh_ratio`, `bounce_in_rate`, `bounce_in_pos_error` and the record of
    what the evaluation hands on, all in the step's one launch (`v2p_tennis_eval_step`).  cfg env.episodeLength (default 600) is the
    strict bound of the law; enableEarlyTermination is refused - the law ignores it.  Everything else is `TennisControllerTask`'s: the
    generator (built with is_train false), the target, the low-level policy, `reset(ids)`, `reset_by_flags()`.  The meters are not
    zeroed when an env resets (the reference does not); `_distance` stands still."""

    def __init__(self, task, cfg, params=traj_out_params, seed=None):
        env = dict(cfg.get("env") or {})
        if env.get("enableEarlyTermination"):
            raise ValueError("TennisControllerEval: cfg env.enableEarlyTermination is set, and the test-mode episode law (MVAEControllerVis._compute_reset) "
                             "ignores it: an episode ends only when progress_buf > episodeLength")
        env.setdefault("episodeLength", 600)
        super().__init__(task, dict(cfg, env=env), params, seed)
        from ..mvae_target import tree_from_model

        smpl_of_body = tree_from_model(task.body_names, task.body_model.parents)[1]
        self.eval_settings = eval_settings(self._max_episode_length, [smpl_of_body.index(j) for j in range(24)])
        n = self.num_envs
        self._meters = {k: torch.as_tensor(v, device=self.device) for k, v in meters_reset(n).items()}
        for i, name in enumerate(METER_NAMES):
            setattr(self, name, Meter(*(self._meters[k][i] for k in METER_FIELDS)))
        self.frame_index = 0
        self._record = self._eval_structs = None

    def start_record(self, num_frames):
        """Allocate the record for `num_frames` steps (cfg env.num_rec_frames of the reference) and start at frame 0; rows of frames not
        yet written are NaN / -1.  The arrays are frame-major [F,N,...]: the `*_all` properties give the reference's [N,f,...] views."""
        F, n = int(num_frames), self.num_envs
        if F < 1:
            raise ValueError("start_record: num_frames %d < 1" % F)
        f = dict(dtype=torch.float32, device=self.device)
        nan = float("nan")
        self._record = dict(joint_rot=torch.full((F, n, 24, 3), nan, **f), root_pos=torch.full((F, n, 3), nan, **f), ball_pos=torch.full((F, n, 3), nan, **f),
                            target_pos=torch.full((F, n, 3), nan, **f), phase=torch.full((F, n), nan, **f),
                            swing_type_cycle=torch.full((F, n), -1, dtype=torch.long, device=self.device))
        self.frame_index, self._eval_structs = 0, None

    def _launch_step(self):
        rec = self._record
        if rec is not None and self.frame_index >= rec["phase"].shape[0]:
            raise RuntimeError("TennisControllerEval: the record holds %d frames and all are written (start_record)" % rec["phase"].shape[0])
        if self._eval_structs is None:  # (the meters and the record stay where they are between two `start_record`s)
            self._eval_structs = eval_structs(self.eval_settings, self.num_envs, self._meters, rec, None if rec is None else self.task._dof_state)
        names = launch_eval_step(self.settings, self.eval_settings, self._tensors(), self.num_envs, self._meters, frame=self.frame_index, structs=self._eval_structs)
        self.frame_index += 1  # (a host count, as the reference's)
        return names

    def _frames(self, name):
        if self._record is None:
            raise RuntimeError("TennisControllerEval: no record (start_record)")
        t = self._record[name][:self.frame_index]
        return t.permute(1, 0, *range(2, t.dim()))

    joint_rot_all = property(lambda self: self._frames("joint_rot"))      # [N,f,24,3]
    root_pos_all = property(lambda self: self._frames("root_pos"))        # [N,f,3]
    ball_pos_all = property(lambda self: self._frames("ball_pos"))
    target_pos_all = property(lambda self: self._frames("target_pos"))
    phase_all = property(lambda self: self._frames("phase"))              # [N,f]
    swing_type_all = property(lambda self: self._frames("swing_type_cycle"))

    def select_best(self):
        """The candidate env ids of mvae_controller_vis.py:149-156 (device tensor): envs with `bounce_in_rate.avg > 0.95` and
        `fh_ratio.avg < 0.6`, sorted by the distance their root travelled over the record, descending.  Torch, once, after the run."""
        return select_best(self.root_pos_all, self.bounce_in_rate.avg, self.fh_ratio.avg)

    def fixed_joint_rot(self, env_ids, num_iters=None):
        """`joint_rot_all[env_ids]` [T,f,24,3] with the two-hand backhand fix of `render_one_result` (mvae_controller_vis.py:181-190,
        cfg v2p `fix_two_hand_backhand_post`) applied, for the envs `select_best()` names: one launch for all of them
        (`two_hand_fix.fix_two_hand_backhand`, num_iters None: its 500), cfg v2p `righthand` (default True) for every env.  A new
        tensor; the record stays as written."""
        from .. import two_hand_fix as thf

        target = self._imitation_target
        if target is None:
            raise RuntimeError("TennisControllerEval: the two-hand fix reads joint_pos_bind of the imitation target, and none is attached")
        ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long).reshape(-1)
        joint_rot = self.joint_rot_all[ids].contiguous()
        T, f = joint_rot.shape[0], joint_rot.shape[1]
        i32 = dict(dtype=torch.int32, device=self.device)
        st = thf.fix_settings(self.task.body_names, self.task.body_model.parents)
        bind = thf.bind_rows_of(target)
        return thf.fix_two_hand_backhand(joint_rot, self.phase_all[ids].contiguous(), self.swing_type_all[ids].contiguous(), torch.full((T,), f, **i32),
                                         torch.full((T,), int(bool(self.cfg_v2p.get("righthand", True))), **i32), bind, thf.NUM_ITERS if num_iters is None else num_iters, settings=st)

    def summary(self):
        """{meter: mean of its `avg` over the envs with count > 0 (NaN without one), meter + '_envs': their number} - how a controller is
        judged.  One host read, after the run."""
        on = self._meters["meter_count"] > 0
        envs = on.sum(1)
        mean = (self._meters["meter_avg"].double() * on).sum(1) / envs
        got = torch.cat([mean, envs.double()]).cpu().tolist()
        out = {name: got[i] for i, name in enumerate(METER_NAMES)}
        out.update({name + "_envs": int(got[4 + i]) for i, name in enumerate(METER_NAMES)})
        return out


def select_best(root_pos_all, bounce_in_rate_avg, fh_ratio_avg):
    """mvae_controller_vis.py:151-154 on tensors: root_pos_all [N,f,3], the two `avg` rows [N]."""
    dist = (root_pos_all[:, 1:] - root_pos_all[:, :-1]).norm(dim=-1).sum(dim=-1)
    candidates = (bounce_in_rate_avg > 0.95) & (fh_ratio_avg < 0.6)
    ids = candidates.nonzero(as_tuple=False).flatten()
    return ids[torch.argsort(dist[candidates], descending=True)]
