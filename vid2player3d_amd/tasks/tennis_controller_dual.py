"""The two-player rally on the device (vid2player/env/tasks/physics_mvae_controller_dual.py, `PhysicsMVAEControllerDual`, with
`HumanoidSMPLIMMVAEDual._reset_balls`, humanoid_smpl_im_mvae_dual.py:52-81, and `TennisBallInEstimator.estimate`,
utils/tennis_ball_in_estimator.py:48-79).  Envs 2k and 2k+1 are opponents (utils/common.py:111-115).

Two launches.  `v2p_tennis_dual_step` is the single player's task step (tasks/tennis_controller.py) without the out-estimator, with the
racket normal of the env's parity and with the dual reset law: a player's recovery is its opponent's reaction, and a miss or a ball
out ends the episode of both.  `v2p_tennis_dual_handover` is what the flags of that step ask for at every hit: the hitter's ball state,
quantised on the in-estimator's grids, becomes the receiver's incoming ball - mirrored state, the table's flight as the receiver's
`_ball_traj`, its reaction task and its observation - for all pairs in one launch, without an id list or a host synchronisation (the
reference has two `.nonzero()`, `terminate.sum() > 0`, `index.cpu()` and a gather from a host table per control step).

`dual_step_reference` and `handover_reference` are the numpy statements of the two launches - the checkers of the tests; the product
never calls them.  `DualTennisControllerTask` is the reference-shaped object.  Training-mode semantics: the extra
`_update_state_from_sim()` "for vis" when not training (humanoid_smpl_im_mvae_dual.py:46-48) is not built.  Under `dual_mode: different`
the attached motion generator is the two-player one (a weight set per side, `v2p_mvae_dual_step` / `_reset`) and the imitation target
takes a body shape per side.

Finished pairs are reset in one of two ways.  `reset(ids)` takes the id list of whole pairs, checks it and gathers by it: the host reads
device results.  `reset_pairs_by_flags()` takes `reset_buf` as the mask - a pair is flagged when either of its two words is up - and is
one fixed sequence of launches over all envs, the same whether 0 or N/2 pairs are done: `v2p_ctl_pair_reset_begin`, the generator's
flagged reset, `v2p_mvae_target_reset_flagged`, `v2p_env_push_state_flagged`, `v2p_tennis_dual_serve_flagged`, the hand-over,
`v2p_ctl_pair_reset_end`; no id list, no host read, no allocation, and the same bits as `reset(ids)` of those pairs.
`pair_reset_begin_reference`, `serve_flagged_reference` and `pair_reset_end_reference` are the numpy statements of the three new
launches.  `match.MatchPlayer` is the loop around either.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from ..ball_traj import traj_in_params, traj_out_params
from . import tennis_controller as tc
from .tennis_controller import GRIP_NORMALS, TRAJ_FRAMES

_f = np.float32
DUAL_TENSOR_NAMES = _lib.TENNIS_BUFFER_NAMES + ("traj_in", "target_draw", "num_reset_reaction")
# buffers of v2p_tennis_buffers that neither dual launch touches
UNUSED_BUFFERS = ("traj_out_x", "traj_out_y", "tar_time_total", "vel_x_overflow", "terminate")


def in_grids_of(params=traj_in_params):
    """The four (lo, hi, step) ranges of the in-estimator in the order of v2p_tennis_dual_cfg.in_grid."""
    return np.array([params.HEIGHT_RANGE, params.VEL_X_RANGE, params.VEL_Y_RANGE, params.VSPIN_RANGE], dtype=np.float64)


def dual_settings(grip=("eastern", "eastern"), in_grids=None, **task_kw):
    """tc.task_settings(...) plus the grips of even and odd envs (names of GRIP_NORMALS or 3-vectors; one value serves both, as
    `dual_mode: True` does) and the in-estimator's grids."""
    one = isinstance(grip, str) or (len(grip) == 3 and all(np.ndim(x) == 0 and not isinstance(x, str) for x in grip))
    grips = [grip, grip] if one else list(grip)
    if len(grips) != 2:
        raise ValueError("dual_settings: grip is one value or one per side of a pair, got %r" % (grip,))
    st = tc.task_settings(grip=grips[0], **task_kw)
    st["grip_normals"] = tuple(tuple(float(x) for x in (GRIP_NORMALS[g] if isinstance(g, str) else g)) for g in grips)
    st["in_grids"] = np.asarray(in_grids_of() if in_grids is None else in_grids, dtype=np.float64).reshape(4, 3)
    return st


def dual_cfg_struct(st, table_shape):
    """v2p_tennis_dual_cfg of a settings dict and the shape of the in-estimator's table [B,F,2]."""
    d = _lib.TennisDualCfg(in_rows=int(table_shape[0]), in_frames=int(table_shape[1]))
    for p in range(2):
        d.grip_normal[p][:] = st["grip_normals"][p]
    for g in range(4):
        d.in_grid[g][:] = [float(x) for x in st["in_grids"][g]]
    return d


def _structs(st, tensors):
    unknown = set(tensors) - set(DUAL_TENSOR_NAMES)
    if unknown:
        raise ValueError("not buffers of the dual launches: %s" % sorted(unknown))
    c = tc.cfg_struct(st, (1, 1), (1, 1, 2))  # (no out-estimator: its tables are not read)
    b = tc.buffers_struct({k: v for k, v in tensors.items() if k in _lib.TENNIS_BUFFER_NAMES})
    table = tensors.get("traj_in")
    d = dual_cfg_struct(st, (1, 1, 2) if table is None else table.shape)
    return c, b, d


def launch_dual_step(st, tensors, n):
    """v2p_tennis_dual_step on a dict of device tensors (names of DUAL_TENSOR_NAMES); returns the names string of the reward law."""
    lib = _lib.load()
    c, b, d = _structs(st, tensors)
    names = C.c_char_p()
    dev = tensors["obs"].device
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_tennis_dual_step(C.byref(c), C.byref(d), int(n), C.byref(b), C.byref(names), _lib.current_stream(dev)), "v2p_tennis_dual_step")
    return names.value.decode()


def launch_handover(st, tensors, n):
    """v2p_tennis_dual_handover on a dict of device tensors (names of DUAL_TENSOR_NAMES)."""
    lib = _lib.load()
    c, b, d = _structs(st, tensors)
    for k in _lib.TENNIS_DUAL_BUFFER_NAMES:
        t = tensors.get(k)
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise RuntimeError("tennis hand-over: buffer %s must be a contiguous GPU tensor (there is no CPU path)" % k)
    db = _lib.TennisDualBuffers(**{k: tensors[k].data_ptr() for k in _lib.TENNIS_DUAL_BUFFER_NAMES if tensors.get(k) is not None})
    dev = tensors["obs"].device
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_tennis_dual_handover(C.byref(c), C.byref(d), int(n), C.byref(b), C.byref(db), _lib.current_stream(dev)), "v2p_tennis_dual_handover")


# ------------------------------------------------------------------------------------------------------------------ the checkers
def _by_parity(st, fn):
    """fn(settings with ONE grip) evaluated for the grip of even and of odd envs."""
    return [fn(dict(st, grip_normal=g)) for g in st["grip_normals"]]


def dual_step_reference(st, s):
    """One control step of the two-player task on arrays: `tc.task_step_reference` (everything up to the observation, with the racket
    normal of the env's parity and the out-estimator out of reach) and `PhysicsMVAEControllerDual._compute_reset` (:96-121).  Returns
    every array the launch writes; `reset` is the input's where the law leaves it alone."""
    n = len(s["ball_state"])
    if n % 2:
        raise ValueError("dual_step_reference: %d envs (opponents are envs 2k and 2k+1)" % n)
    s = dict(s)
    s.setdefault("tar_time_total", np.full(n, -1, np.int64))
    s.setdefault("traj_out_x", np.zeros((1, 1), _f))
    s.setdefault("traj_out_y", np.zeros((1, 1, 2), _f))
    grids = np.array(st["grids"], dtype=np.float64)
    grids[0, 0] = np.inf  # (no ball is faster than that: `valid` of the out-estimator is empty, as under dual_mode :299)
    even, odd = _by_parity(dict(st, grids=grids), lambda one: tc.task_step_reference(one, s))
    side = np.arange(n) % 2 == 1
    o = {}
    for k, v in even.items():
        if k in ("est_bounce_pos", "est_bounce_time", "est_max_height", "est_bounce_in", "vel_x_overflow", "terminate", "reset", "reset_reaction", "reset_recovery"):
            continue
        o[k] = np.where(side.reshape((n,) + (1,) * (np.ndim(v) - 1)), odd[k], v) if np.ndim(v) >= 1 and len(v) == n and not isinstance(v, str) else v
    ball, root = np.asarray(s["ball_state"], dtype=_f), np.asarray(s["rb_state"], dtype=_f).reshape(n, 24, 13)[:, 0, 0:3]
    tar_action, hit = np.asarray(s["tar_action"], dtype=np.int64), o["has_racket_contact"].astype(bool)
    has_bounce = np.asarray(s["has_bounce"]).astype(bool)
    opp = np.arange(n) ^ 1
    recovery = (tar_action == 1) & (hit | (ball[:, 1] < root[:, 1] - _f(1)) | (has_bounce & (ball[:, 2] < _f(0.05))))
    terminate = (recovery & ~hit) | ((tar_action == 0) & has_bounce & ~o["bounce_in"].astype(bool))
    terminate = terminate | terminate[opp]
    o["reset"] = np.where(terminate, 1, np.asarray(s["reset"], dtype=np.int64))
    o["reset_reaction"] = recovery[opp] & ~terminate
    o["reset_recovery"] = recovery & ~terminate
    return o


def in_estimate_reference(grids, table, states, dt=np.float32):
    """`TennisBallInEstimator.estimate` (:22-79) on ball states [m,13] in arithmetic `dt`: (traj_trans [m,F,3], ball_states_in,
    ball_states_out, table rows [m] int64).  float32 restates torch's elementwise order, scalars rounded where torch rounds them."""
    b = np.asarray(states, dtype=dt)
    G = np.asarray(grids, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        vel_x = np.sqrt(b[:, 7] * b[:, 7] + b[:, 8] * b[:, 8])
        d = b[:, 7:9] / vel_x[:, None]
        vspin = np.sqrt(b[:, 10] * b[:, 10] + b[:, 11] * b[:, 11] + b[:, 12] * b[:, 12]) / dt(math.pi * 2)
        cell = lambda v, r: np.rint((np.clip(v, dt(r[0]), dt(r[1] - r[2])) - dt(r[0])) / dt(r[2]))
        ih, ix, iy, iv = cell(b[:, 2], G[0]), cell(vel_x, G[1]), cell(b[:, 9], G[2]), cell(vspin, G[3])
        dim = [dt((r[1] - r[0]) / r[2]) for r in G]
        index = ih * dim[1] * dim[2] * dim[3] + ix * dim[2] * dim[3] + iy * dim[3] + iv
        rows = np.clip(np.nan_to_num(index, nan=0.0).astype(np.int64), 0, len(table) - 1)
        back = lambda i, r: i * dt(r[2]) + dt(r[0])
        height, vel_x, vel_y, vspin = back(ih, G[0]), back(ix, G[1]), back(iy, G[2]), back(iv, G[3])
        t = np.asarray(table)[rows].astype(dt)
        traj = np.concatenate([(t[:, :, :1] * d[:, None, :] + b[:, None, 0:2]) * dt(-1), t[:, :, 1:]], -1)

        def ang_vel(v):
            c = np.stack([v[:, 1] * dt(-1) - v[:, 2] * dt(0), v[:, 2] * dt(0) - v[:, 0] * dt(-1), v[:, 0] * dt(0) - v[:, 1] * dt(0)], -1)
            nrm = np.maximum(np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]), dt(1e-12))
            return (vspin * dt(math.pi) * dt(2))[:, None] * (c / nrm[:, None])

        s_in = b.copy()
        s_in[:, 0:2] = b[:, 0:2] * dt(-1)
        s_in[:, 2] = height
        s_in[:, 7:9] = (-vel_x)[:, None] * d
        s_in[:, 9] = vel_y
        s_in[:, 10:13] = ang_vel(s_in[:, 7:10])
        s_out = s_in.copy()
        s_out[:, 0:2] = s_in[:, 0:2] * dt(-1)
        s_out[:, 7:9] = s_in[:, 7:9] * dt(-1)
        s_out[:, 10:13] = ang_vel(s_out[:, 7:10])
    return traj.astype(dt), s_in, s_out, rows


def handover_reference(st, s, dt=np.float32):
    """The flag-driven half of the dual `_reset_envs` (:42-64, training mode) on arrays named like DUAL_TENSOR_NAMES: the state before
    (`reset_reaction` / `reset_recovery` as the step left them, `traj_in` [B,F,2], `target_draw` [n] with use_random_ball_target).
    Returns every array the launch writes, whole; nothing in `s` is modified.  `table_rows` [n] (-1: no lookup) is returned on top."""
    n = len(s["ball_state"])
    if n % 2:
        raise ValueError("handover_reference: %d envs (opponents are envs 2k and 2k+1)" % n)
    A = lambda k, t=None: np.array(s[k], dtype=t)
    react, recover = A("reset_reaction").astype(bool), A("reset_recovery").astype(bool)
    ids, rec_ids = np.nonzero(react)[0], np.nonzero(recover)[0]
    # get_opponent_env_ids SORTS the opponents (utils/common.py:111-115): where both envs of a pair react, row i of the estimate no
    # longer belongs to the opponent of ids[i] but to ids[i] itself - such an env flies the table row of its OWN state
    contact = np.sort(ids ^ 1)
    table = np.asarray(s["traj_in"])
    F = table.shape[1]
    ball = A("ball_state", dt)
    traj, s_in, s_out, rows = in_estimate_reference(st["in_grids"], table, ball[contact], dt)
    o = {"table_rows": np.full(n, -1, np.int64)}
    o["table_rows"][ids] = rows
    if not st["use_history"]:
        # `_ball_traj[ids, :F] = new_traj` on the reference's rolled tensor: frames F..99 of the current window stay
        old = np.concatenate([A("ball_traj", dt).reshape(n, TRAJ_FRAMES, 3), np.zeros((n, TRAJ_FRAMES, 3), dt)], 1)
        cur = np.clip(A("traj_cursor", np.int64), 0, TRAJ_FRAMES)
        window = old[np.arange(n)[:, None], cur[:, None] + np.arange(TRAJ_FRAMES)[None]]
        new = A("ball_traj", dt).reshape(n, TRAJ_FRAMES, 3)
        new[ids] = window[ids]
        new[ids, :F] = traj
        cursor = A("traj_cursor", np.int32)
        cursor[ids] = 0
        o.update(ball_traj=new, traj_cursor=cursor)
    ball[ids] = s_in
    ball[contact] = s_out  # (where both react, out wins)
    has_bounce, bounce_pos, contact_flag, prev_vy = A("has_bounce").astype(bool), A("bounce_pos", dt), A("has_racket_contact").astype(bool), A("prev_ball_vy", dt)
    has_bounce[ids], bounce_pos[ids], contact_flag[ids] = False, 0, False
    prev_vy[ids] = ball[ids, 8]
    tar_action, tar_time, count, bounce_in = A("tar_action", np.int64), A("tar_time", np.int64), A("num_reset_reaction", np.int64), A("bounce_in").astype(bool)
    tar_action[rec_ids], has_bounce[rec_ids], bounce_pos[rec_ids] = 0, False, 0
    tar_time[ids], tar_action[ids], bounce_in[ids] = 0, 1, False
    count[ids] += 1
    o.update(ball_state=ball, has_bounce=has_bounce, bounce_pos=bounce_pos, has_racket_contact=contact_flag, prev_ball_vy=prev_vy, tar_action=tar_action,
             tar_time=tar_time, num_reset_reaction=count, bounce_in=bounce_in)
    after = dict(s, **{k: v for k, v in o.items() if k != "table_rows"})
    if s.get("ball_obs") is not None:
        hist = A("ball_obs", dt).reshape(n, st["L"], 3)
        if st["use_history"]:
            hist[ids] = ball[ids, None, 0:3]
        after["ball_obs"] = hist
    if st["use_target"]:
        u = np.asarray(s["target_draw"], dtype=_f)[ids]
        target = A("target_bounce_pos", dt)
        target[ids] = np.stack([np.where(u < _f(0.33), -3.0, np.where(u > _f(0.67), 3.0, 0.0)), np.full(len(ids), 10.0), np.zeros(len(ids))], -1)
        o["target_bounce_pos"] = after["target_bounce_pos"] = target
    if st["reward_type"] == "return_w_estimate":
        est, est_time, est_in, est_peak = A("est_bounce_pos", dt), A("est_bounce_time", dt), A("est_bounce_in").astype(bool), A("est_max_height", dt)
        est[ids], est_time[ids], est_in[ids], est_peak[ids] = 0, 0, False, 0
        o.update(est_bounce_pos=est, est_bounce_time=est_time, est_bounce_in=est_in, est_max_height=est_peak)
    # `_compute_observations(reset_reaction_env_ids)`
    obs, rpos, rnorm = A("obs", dt), A("racket_pos", dt), A("racket_normal", dt)
    hist_out = after.get("ball_obs")
    for side, (rows_obs, hist, rp, rn) in enumerate(_by_parity(st, lambda one: tc.observation_reference(one, after, ids))):
        sel = ids % 2 == side
        obs[ids[sel]], rpos[ids[sel]], rnorm[ids[sel]] = rows_obs[sel], rp[sel], rn[sel]
        if hist is not None:
            hist_out = hist_out.copy() if side == 0 else hist_out
            hist_out[ids[sel]] = hist[sel]
    o.update(obs=obs, racket_pos=rpos, racket_normal=rnorm)
    if hist_out is not None:
        o["ball_obs"] = hist_out
    return o


# ------------------------------------------------------------------------------------------------------------------ pairs by flags
def _receiver_side(serve_from):
    if serve_from not in _lib.SERVE_FROM:
        raise ValueError("serve_from %r is neither 'near' nor 'far'" % (serve_from,))
    return _lib.SERVE_FROM[serve_from]  # 'near': the even env of a pair receives and the odd env serves (:31-36)


def pair_flags_reference(flags):
    """(mask made whole [n] int64, pair flagged [n] bool): a pair (2k, 2k+1) is flagged when either word is not 0; its zero word becomes
    1, a non-zero word keeps its value."""
    f = np.array(flags, dtype=np.int64).reshape(-1, 2)
    up = (f != 0).any(1)
    return np.where(up[:, None] & (f == 0), 1, f).reshape(-1), np.repeat(up, 2)


def pair_reset_begin_reference(s, flags, serve_from="near"):
    """`v2p_ctl_pair_reset_begin` on arrays (names of _lib.CTL_RESET_BUFFER_NAMES): returns (the seven arrays after, the flags after)."""
    whole, up = pair_flags_reference(flags)
    receives = np.arange(len(whole)) % 2 == _receiver_side(serve_from)
    o = {k: np.array(v) for k, v in s.items()}
    for k in ("progress", "terminate", "num_reset_reaction", "distance"):
        o[k][up] = 0
    o["num_reset"][up] += 1
    o["reset_reaction"] = np.where(up, receives, o["reset_reaction"].astype(bool))
    o["reset_recovery"] = np.where(up, ~receives, o["reset_recovery"].astype(bool))
    return o, whole


def serve_flagged_reference(flags, serve_from, racket_pos, ball_state, draws):
    """`v2p_tennis_dual_serve_flagged` on arrays: `_reset_balls` (humanoid_smpl_im_mvae_dual.py:56-63) for the servers of the flagged
    pairs.  draws [n/2,3]: a row per PAIR (the caller's table, or `device_rng.uniform` of the words `serve_vel_reference` reads)."""
    from ..device_rng import SERVE_VEL_OFFSET, SERVE_VEL_SCALE

    _, up = pair_flags_reference(flags)
    n = len(up)
    servers = np.flatnonzero(up & (np.arange(n) % 2 != _receiver_side(serve_from)))
    ball = np.array(ball_state, dtype=_f)
    ball[servers, 0:3] = np.asarray(racket_pos, dtype=_f)[servers]
    ball[servers, 10:13] = np.array([-40.0, 0.0, 0.0], _f)
    ball[servers, 7:10] = np.asarray(draws, dtype=_f).reshape(-1, 3)[servers >> 1] * np.array(SERVE_VEL_SCALE, _f) + np.array(SERVE_VEL_OFFSET, _f)
    return ball


def pair_reset_end_reference(flags):
    """`v2p_ctl_pair_reset_end` on arrays: the mask, cleared."""
    return np.zeros_like(np.asarray(flags, dtype=np.int64))


def _stream(t):
    return _lib.current_stream(t.device)


def _need(t, shape, dtype, what):
    """a kernel indexes `t` by env or by pair: anything but a contiguous GPU tensor of that shape is refused here"""
    if not torch.is_tensor(t) or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or (dtype is not None and t.dtype != dtype):
        raise RuntimeError("%s must be a contiguous %sGPU tensor %s" % (what, "" if dtype is None else str(dtype).replace("torch.", "") + " ", list(shape)))


def launch_pair_reset_begin(n, flags, tensors, serve_from="near"):
    """v2p_ctl_pair_reset_begin on a dict of device tensors (names of _lib.CTL_RESET_BUFFER_NAMES; None = NULL)."""
    _need(flags, (n,), torch.int64, "v2p_ctl_pair_reset_begin: flags")
    for k, v in tensors.items():
        if v is not None:
            _need(v, (n,), None, "v2p_ctl_pair_reset_begin: " + k)
    b = _lib.CtlResetBuffers(**{k: v.data_ptr() for k, v in tensors.items() if v is not None})
    with torch.cuda.device(flags.device):
        _lib.check(_lib.load().v2p_ctl_pair_reset_begin(int(n), _lib.ptr(flags), C.byref(b), _receiver_side(serve_from), _stream(flags)), "v2p_ctl_pair_reset_begin")


def launch_serve_flagged(n, flags, serve_from, racket_pos, ball_state, draws=None, seed=0, call=0):
    """v2p_tennis_dual_serve_flagged; draws [n/2,3] (None: the kernel draws under (seed, call, server))."""
    who = "v2p_tennis_dual_serve_flagged: "
    _need(flags, (n,), torch.int64, who + "flags")
    _need(racket_pos, (n, 3), torch.float32, who + "racket_pos")
    _need(ball_state, (n, 13), torch.float32, who + "ball_state")
    if draws is not None:
        _need(draws, (n // 2, 3), torch.float32, who + "draws")
    rule = None if draws is not None else _lib.ServeRule(seed=int(seed) & (2 ** 64 - 1), call=int(call) & (2 ** 64 - 1))
    with torch.cuda.device(flags.device):
        _lib.check(_lib.load().v2p_tennis_dual_serve_flagged(int(n), _lib.ptr(flags), _receiver_side(serve_from), _lib.ptr(racket_pos), _lib.ptr(ball_state), _lib.ptr(draws),
                                                             None if rule is None else C.byref(rule), _stream(flags)), "v2p_tennis_dual_serve_flagged")


def launch_pair_reset_end(n, flags):
    _need(flags, (n,), torch.int64, "v2p_ctl_pair_reset_end: flags")
    with torch.cuda.device(flags.device):
        _lib.check(_lib.load().v2p_ctl_pair_reset_end(int(n), _lib.ptr(flags), _stream(flags)), "v2p_ctl_pair_reset_end")


# ------------------------------------------------------------------------------------------------------------------ the task
class DualTennisControllerTask(tc.TennisControllerTask):
    """`PhysicsMVAEControllerDual` on top of a racket + ball batch: cfg v2p `dual_mode: True` over a single-player task (both sides of a
    pair are the same player) or `dual_mode: 'different'` over a two-player one (env i is player i % 2, its own wrist link and, with a
    `grip` list, its own grip).  On top of `TennisControllerTask`'s cfg: `ball_traj_in_file` (a file name or an array [B,F,2]),
    `serve_from` (see `reset`); `traj_in_params`: the in-estimator's grids.  Both task
    flags start at zero (:16-17).  `post_physics_step()` is `v2p_tennis_dual_step`; `reset([])` is `v2p_tennis_dual_handover` alone - the
    rally path, no synchronisation; `reset(ids)` with whole sorted pairs resets their actors first; `reset_pairs_by_flags()` does the same
    for the pairs whose `reset_buf` is up, without a list and without a host read.  `_reset_root_xy` [N,2] and `_reset_serve_draws`
    [N/2,3] (both default None: drawn) stand in for the draws of either."""

    def __init__(self, task, cfg, params=traj_out_params, traj_in_params=traj_in_params, seed=None):
        super().__init__(task, cfg, params, seed=seed)
        v2p, dev, n = self.cfg_v2p, self.device, self.num_envs
        if "ball_traj_in_file" not in v2p:
            raise ValueError("DualTennisControllerTask: cfg v2p.ball_traj_in_file (the in-estimator's table, a file name or an array) is required")
        t = v2p["ball_traj_in_file"]
        self._ball_traj_in = torch.from_numpy(np.ascontiguousarray(np.load(t) if isinstance(t, str) else t, dtype=np.float32)).to(dev).contiguous()
        if self._ball_traj_in.dim() != 3 or self._ball_traj_in.shape[2] != 2 or not 1 <= self._ball_traj_in.shape[1] <= TRAJ_FRAMES:
            raise ValueError("the in-estimator's table must be [B,F,2] with F <= %d" % TRAJ_FRAMES)
        self.settings = dict(self.settings, **{k: v for k, v in dual_settings(grip=v2p.get("grip", "eastern"), in_grids=in_grids_of(traj_in_params)).items()
                                               if k in ("grip_normals", "in_grids")})
        self._reset_reaction_buf[:] = False
        self._reset_recovery_buf[:] = False
        self._target_draw = torch.zeros(n, dtype=torch.float32, device=dev)
        # [N/2,3]: a uniform draw per PAIR that stands in for the serve's, in `reset_pairs_by_flags()`; `match.MatchPlayer` hands
        # `reset(ids)` its rows.  Without it the serve kernel draws under (seed, the count of such launches, the server's env id)
        self._reset_serve_draws = None
        self._serve_calls = 0

    def _check_mode(self, task, v2p):
        mode, players = v2p.get("dual_mode"), getattr(task, "racket_players", None)
        if mode is True and players is None or mode == "different" and players is not None:
            if task.num_envs % 2:
                raise ValueError("DualTennisControllerTask: envs 2k and 2k+1 are opponents - num_envs must be even, got %d" % task.num_envs)
            return
        raise ValueError("DualTennisControllerTask: cfg v2p.dual_mode True goes with a single-player racket + ball task, 'different' with a "
                         "two-player one; got dual_mode %r over %s" % (mode, "a two-player task" if players is not None else "a single-player task"))

    def reset_by_flags(self):
        raise NotImplementedError("DualTennisControllerTask.reset_by_flags: resetting finished pairs by mask is not built (the single-player controller's is)")

    def attach_motion_generator(self, player):
        """As `TennisControllerTask.attach_motion_generator`; the player's mode is the task's: one generator for both sides under
        `dual_mode: True`, a weight set per side under 'different'."""
        if bool(getattr(player, "_is_dual", False)) != (self.cfg_v2p.get("dual_mode") == "different"):
            raise ValueError("attach_motion_generator: cfg v2p.dual_mode %r and the player's (%r) disagree" % (self.cfg_v2p.get("dual_mode"), player.cfg.get("dual_mode")))
        super().attach_motion_generator(player)

    def _grip(self, v2p):
        """The grip of the base settings: the even side's (cfg v2p.grip is a list of two names under `dual_mode: different`, one name
        otherwise); both sides' grips are `settings["grip_normals"]`."""
        grip = v2p.get("grip", "eastern")
        if v2p.get("dual_mode") == "different":
            if isinstance(grip, str) or len(grip) != 2 or not all(isinstance(g, str) for g in grip):
                raise ValueError("DualTennisControllerTask: with dual_mode 'different' cfg v2p.grip is a list of two names (one per player), got %r" % (grip,))
            return grip[0]
        return grip

    def _load_tables(self, v2p, load):
        self._ball_traj_out_x = self._ball_traj_out_y = None  # (no out-estimator under dual_mode, physics_mvae_controller.py:73)

    def _tensors(self):
        t = {k: v for k, v in super()._tensors().items() if k not in UNUSED_BUFFERS}
        t.update(traj_in=self._ball_traj_in, target_draw=self._target_draw, num_reset_reaction=self._num_reset_reaction)
        return t

    def _launch_step(self):
        return launch_dual_step(self.settings, self._tensors(), self.num_envs)

    def handover(self):
        """Launch 2 for all pairs, from the flags as they stand."""
        if self.settings["use_target"]:
            self._target_draw.uniform_()
        launch_handover(self.settings, self._tensors(), self.num_envs)
        self._has_init = True

    def reset(self, env_ids=None, root_xy=None, serve_vel_draws=None):
        """`reset` / `_reset_envs` (:22-66).  None after initialisation returns; an empty list is the hand-over alone.  env_ids - whole
        pairs, ascending - get the reference's actor reset first: of every pair the player on `serve_from`'s side ('near': the odd env,
        :31-36) starts from the serve frame and its opponent from the ready frame (`MotionVAEPlayer.reset_dual`, root_xy as there), the
        physics task takes the pose (`ImitationTarget.reset`), the ball goes to the server's racket head with spin (-40, 0, 0) and the
        velocity of `_reset_balls:61-63` from serve_vel_draws [pairs,3] (uniform draws in [0,1), drawn here when left out), the receiver
        gets `reset_reaction` and the server `reset_recovery` (:37-38) - and then the hand-over serves."""
        if env_ids is None:
            if self._has_init:
                return
            env_ids = torch.arange(self.num_envs, device=self.device, dtype=torch.long)
        ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long).reshape(-1)
        if ids.numel():
            if ids.numel() % 2 or not bool(((ids[::2] % 2 == 0) & (ids[1::2] == ids[::2] + 1)).all()) or not bool((ids[2::2] > ids[:-2:2]).all()):
                raise ValueError("DualTennisControllerTask.reset: env_ids must be whole pairs (2k, 2k+1) in ascending order")
            receivers = ids[::2] if self.cfg_v2p.get("serve_from", "near") == "near" else ids[1::2]
            servers = receivers ^ 1
            if self._mvae_player is not None:
                self._mvae_player.reset_dual(receivers, servers, root_xy)
                if self._imitation_target is not None:
                    self._imitation_target.reset(ids)
            self._reset_env_tensors(ids)
            self._num_reset[ids] += 1
            if self._mvae_player is not None:
                ball = self.task._ball_root_states
                u = torch.rand((servers.numel(), 3), device=self.device) if serve_vel_draws is None else torch.as_tensor(serve_vel_draws, dtype=torch.float32, device=self.device)
                ball[servers, 0:3] = self._mvae_player._racket_pos[servers]
                ball[servers, 10:13] = torch.tensor([-40.0, 0.0, 0.0], device=self.device)
                ball[servers, 7:10] = u.reshape(-1, 3) * torch.tensor([4.0, 4.0, 3.0], device=self.device) + torch.tensor([-2.0, 28.0, 5.0], device=self.device)
            self._reset_reaction_buf[receivers] = True
            self._reset_recovery_buf[servers] = True
        self.handover()

    def reset_pairs_by_flags(self):
        """`reset(ids of the done pairs)` for the pairs whose `reset_buf` is up (either word of a pair), without knowing them on the
        host: ONE fixed sequence of launches over all envs, the same whether 0 or N/2 pairs are done - `v2p_ctl_pair_reset_begin` (the
        mask made whole, the bookkeeping, the pair's reaction / recovery flags), the generator's flagged reset
        (`MotionVAEPlayer.reset_dual_flagged`), `v2p_mvae_target_reset_flagged` and `v2p_env_push_state_flagged`,
        `v2p_tennis_dual_serve_flagged`, the hand-over (with its `_target_draw.uniform_()` under use_random_ball_target),
        `v2p_ctl_pair_reset_end` (the mask).  No host read of a device result, no id list, no allocation.  `_reset_root_xy` [N,2] and
        `_reset_serve_draws` [N/2,3] stand in for the generator's and the serve's draw; without them the kernels draw.  Without a motion
        generator the generator, target and serve launches are left out, as in `reset(ids)`."""
        who, flags, n = "DualTennisControllerTask.reset_pairs_by_flags", self.reset_buf, self.num_envs
        serve_from = self.cfg_v2p.get("serve_from", "near")
        _receiver_side(serve_from)
        _need(flags, (n,), torch.int64, who + ": reset_buf")
        t = dict(progress=self.progress_buf, terminate=self._terminate_buf, num_reset_reaction=self._num_reset_reaction, num_reset=self._num_reset,
                 distance=self._distance, reset_reaction=self._reset_reaction_buf, reset_recovery=self._reset_recovery_buf)
        for k, v in t.items():
            _need(v, (n,), None, who + ": " + k)
        player, draws = self._mvae_player, self._reset_serve_draws
        if player is not None:
            if player._is_dual and len(player._joint_pos_bind_rel) > 1:
                raise NotImplementedError("%s: the attached generator has %d rows of joint_pos_bind_rel; a row per pair is read by list position, which is not built "
                                          "by flags (reset(ids) is)" % (who, len(player._joint_pos_bind_rel)))
            ball = self.task._ball_root_states
            _need(ball, (n, 13), torch.float32, who + ": the task's _ball_root_states")
            if draws is not None:
                _need(draws, (n // 2, 3), torch.float32, who + ": _reset_serve_draws")
        launch_pair_reset_begin(n, flags, t, serve_from)
        if player is not None:
            player.reset_dual_flagged(flags, self._reset_root_xy, serve_from)
            if self._imitation_target is not None:
                self._imitation_target.reset_flagged(flags)
            launch_serve_flagged(n, flags, serve_from, player._racket_pos, ball, draws, self.seed, self._serve_calls)
            if draws is None:
                self._serve_calls += 1
        self.handover()
        launch_pair_reset_end(n, flags)

    def _reset_envs(self, env_ids):
        self.reset(env_ids)
