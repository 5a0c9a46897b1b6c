"""Golden data of the tennis controller's task step, recorded from the reference itself: tests/golden/tennis_controller.npz.

`PhysicsMVAEController` (vid2player/env/tasks/physics_mvae_controller.py) is imported on the CPU through oracle/ref_shim, with inert
stand-ins for the modules it cannot have here (the MVAE player, the player builder, the viewer, the progress bar).  An object made with
`__new__` gets its attributes set by hand - synthetic player and ball tensors for N = 80 envs - and for T consecutive steps the
reference's OWN methods run on it: `_update_state`, `_compute_reward`, `_compute_observations`, `_compute_reset`, the two lines of
`physics_step`'s roll, then `_reset_env_tensors` / `_reset_recovery_tasks` / `_reset_reaction_tasks` / `_compute_observations(ids)` for
the envs the flags name.  The task-side half of the state update (`HumanoidSMPLIMMVAE._update_state_from_sim`,
humanoid_smpl_im_mvae.py:799-849: the velocity rule of the racket hit, the racket normal) is the reference's own method too, run on a
stand-in task object.  Inputs, state before and after every step are recorded under the names of v2p_tennis_buffers.

Kept small: the players' poses are static over the steps (the actor block of the observation is recorded once, and asserted to be the
same bits in every step of every variant; the root velocity columns are an input), the ball trajectories are rows of a small pool.

The generator asserts that its inputs reach every branch, and that every float32 quantity compared with a threshold - or rounded to an
index - stays 1e-3 away from it, so that flags and indices must match exactly whatever the contraction of the arithmetic.
Only arrays are stored.  Run where the reference exists:
    python tools/gen_golden_tennis_controller.py
"""
import math
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True  # never leave __pycache__ in the read-only reference mount

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)

from ref_shim.install import REFERENCE_ROOT, _Sink, install  # noqa: E402

install()
for absent in ("players", "players.mvae_player", "env.utils.player_builder", "smpl_visualizer", "smpl_visualizer.vis_sport", "tqdm"):
    try:
        __import__(absent)
    except Exception:
        sys.modules[absent] = _Sink(absent)
sys.path.insert(0, os.path.join(REFERENCE_ROOT, "vid2player"))

import torch  # noqa: E402

torch.set_num_threads(1)
torch.Tensor.get_device = lambda self: self.device

import env.tasks.humanoid_smpl_im_mvae as ref_task  # noqa: E402
import env.tasks.physics_mvae_controller as ref_ctl  # noqa: E402
import utils.tennis_ball_out_estimator as ref_out  # noqa: E402

# (`_compute_observations` drops into the debugger when it sees a NaN, :321-328: two envs carry one on purpose)
ref_ctl.pdb = types.SimpleNamespace(set_trace=lambda *a, **k: None)

OUT = os.path.join(REPO, "tests", "golden", "tennis_controller.npz")
N, T, MARGIN = 80, 10, 1e-3
COURT_MIN, COURT_MAX = [-5.0, -16.0], [5.0, -1.0]
SCALES = {"pos": 4.0, "phase": 8.0, "bounce_pos": 0.04, "bounce_time": 0.2}
WEIGHTS = {"pos": 0.7, "ball_pos": 1.3}
MAX_EPISODE_LENGTH, REACTION_NFRAMES = 9, 6
BOUNCE_COURT = (-4.11, 4.11, 0.0, 11.89)


class OutGrid:  # small grids, as tools/gen_golden_ball_estimators.py
    VEL_X_RANGE = (10, 14, 1.0)
    VEL_Y_RANGE = (-2, 2, 1.0)
    VSPIN_RANGE = (-2, 2, 1.0)
    TRAJ_X_RANGE = (0, 10, 0.5)
    TRAJ_Y_RANGE = (0, 3, 0.1)


GRIDS = np.array([OutGrid.VEL_X_RANGE, OutGrid.VEL_Y_RANGE, OutGrid.VSPIN_RANGE, OutGrid.TRAJ_X_RANGE, OutGrid.TRAJ_Y_RANGE], dtype=np.float64)

VARIANTS = {  # every value of every switch appears once
    "A": dict(reward_type="return_w_estimate", history=False, target=False, early=True, velocity=True, L=10, steps=T, grip="eastern"),
    "B": dict(reward_type="reach", history=True, target=True, early=False, velocity=False, L=10, steps=T, grip="semi_western"),
    "C": dict(reward_type="return", history=False, target="continuous", early=True, velocity=False, L=10, steps=T, grip="eastern"),
    "D": dict(reward_type="return_w_estimate", history=False, target=True, early=False, velocity=True, L=100, steps=3, grip="semi_western"),
}


def cells(r):
    return int((r[1] - r[0]) / r[2])


def away(v, thresholds, margin=10 * MARGIN):
    return all(abs(v - t) > margin for t in thresholds)


def index_ok(v, r):
    """the value rounded to an index stays away from every k + 0.5 (in units of the value: MARGIN)"""
    u = (min(max(v, r[0]), r[1] - r[2]) - r[0]) / r[2]
    return abs(u - math.floor(u) - 0.5) * r[2] > 10 * MARGIN


def hit_ok(b, tx, ty):
    """margins of everything `TennisBallOutEstimator.estimate` compares or rounds for ball state b (float64 restatement, used ONLY to
    reject draws that sit on a threshold)"""
    VX, VY, VS, TX, TY = GRIDS
    if not (away(b[8], [VX[0], 0.0]) and away(b[9], [VY[0], VY[1]]) and away(b[2], [TY[1]])):
        return False
    x_net = b[0] + b[7] * abs(b[1] / b[8])
    if not away(x_net, [-4.0, 4.0]):
        return False
    vel_x = math.hypot(b[7], b[8])
    vspin = float(np.linalg.norm(b[10:13])) / (2 * math.pi)
    net_dist = -b[1] / b[8] * vel_x
    if not (away(vel_x, [VX[1]]) and index_ok(vel_x, VX) and index_ok(b[9], VY) and index_ok(vspin, VS) and index_ok(b[2], TY) and index_ok(net_dist, TX)):
        return False
    idx = lambda v, r: int(round((min(max(v, r[0]), r[1] - r[2]) - r[0]) / r[2]))
    ti = idx(vel_x, VX) * cells(VY) * cells(VS) + idx(b[9], VY) * cells(VS) + idx(vspin, VS)
    bx, by = b[0] + ty[ti, idx(b[2], TY), 0] * b[7] / vel_x, b[1] + ty[ti, idx(b[2], TY), 0] * b[8] / vel_x
    return away(tx[ti, idx(net_dist, TX)] + b[2], [1.07]) and away(bx, BOUNCE_COURT[:2]) and away(by, BOUNCE_COURT[2:])


def make_script(rng, tx, ty):
    """Static player tensors and T steps of scripted ball / flag / motion-generator inputs, shared by the variants."""
    s = {}
    pos = np.zeros((N, 25, 3), np.float32)
    pos[:, 0] = np.stack([rng.uniform(-3, 3, N), rng.uniform(-14, -10, N), rng.uniform(0.8, 1.0, N)], -1)
    pos[:, 1:] = pos[:, :1] + rng.uniform(-0.8, 0.8, (N, 24, 3))
    pos[0, 0, 0], pos[1, 0, 1], pos[2, 0, 0], pos[5, 0, 1] = 6.0, -17.0, -5.5, -0.5  # out of court, one per side
    rot = rng.normal(0, 1, (N, 25, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True) * rng.uniform(0.98, 1.02, (N, 25, 1))  # (not exactly unit: the conversion normalises)
    pos[3, 7, 1] = np.nan   # a NaN in a body position ...
    rot[4, 5, 2] = np.nan   # ... and one in a body rotation (neither the root, the wrist nor the racket)
    s["pos25"], s["rot25"] = pos, rot.astype(np.float32)
    root = pos[:, 0]
    ball = np.zeros((T, N, 13), np.float32)
    ball[:, :, 6] = 1
    hit_step = np.where(rng.uniform(size=N) < 0.45, rng.integers(0, 9, N), 99)
    hit_step[[6, 7]] = 99
    for t in range(T):
        for e in range(N):
            out = t >= hit_step[e]
            for _ in range(1000):
                b = np.zeros(13)
                b[0:3] = [rng.uniform(-3, 3), root[e, 1] + rng.uniform(-2.5, 6.0), rng.choice([rng.uniform(0.3, 2.9), rng.uniform(3.1, 3.4)], p=[0.9, 0.1])]
                b[7:10] = [rng.uniform(-3, 3), rng.uniform(8, 16) if out else rng.uniform(-25, -15), rng.uniform(-2.6, 2.6)]
                b[10:13] = rng.normal(0, 6.0, 3)
                if e in (6, 7):  # the near miss of the velocity rule: vy turns positive, by less than 10 m/s
                    b[8] = -3.0 if t < 4 else 6.9
                b = b.astype(np.float32).astype(np.float64)
                if away(b[1] - (root[e, 1] - 1.0), [0.0]) and (t != hit_step[e] or hit_ok(b, tx, ty)):
                    break
            else:
                raise AssertionError("no draw with margins for env %d step %d" % (e, t))
            ball[t, e, [0, 1, 2, 7, 8, 9, 10, 11, 12]] = b[[0, 1, 2, 7, 8, 9, 10, 11, 12]]
    s["ball_state"], s["hit_step"] = ball, hit_step
    s["root_vel"] = rng.normal(0, 1.5, (T, N, 3)).astype(np.float32)
    s["has_bounce_now"] = rng.uniform(size=(T, N)) < 0.15
    s["has_bounce"] = np.cumsum(s["has_bounce_now"], 0) > 0
    bp = np.stack([rng.uniform(-6, 6, (T, N)), rng.uniform(-3, 15, (T, N)), np.full((T, N), 0.1)], -1)
    for k, lines in ((0, BOUNCE_COURT[:2]), (1, BOUNCE_COURT[2:])):
        for line in lines:
            bp[..., k] = np.where(np.abs(bp[..., k] - line) < 0.02, bp[..., k] + 0.05, bp[..., k])
    s["bounce_pos"] = (bp * s["has_bounce"][..., None]).astype(np.float32)
    s["flag_contact_now"] = np.arange(T)[:, None] == hit_step[None]
    s["flag_contact"] = np.arange(T)[:, None] >= hit_step[None]
    s["phase_pred"] = rng.uniform(2.0, 4.2, (T, N)).astype(np.float32)
    s["swing_type"] = rng.integers(-1, 4, (T, N)).astype(np.int64)
    s["swing_type_cycle"] = rng.integers(-1, 4, (T, N)).astype(np.int64)
    s["pool"] = np.cumsum(rng.normal(0, 0.3, (6, 100, 3)), 1).astype(np.float32) + np.array([0, -11, 1], np.float32)
    s["progress0"] = rng.integers(0, 6, N).astype(np.int64)
    return s


STATE = ("tar_time", "tar_time_total", "tar_action", "progress", "target_bounce_pos", "bounce_in", "est_bounce_pos", "est_bounce_time", "est_max_height", "est_bounce_in",
         "distance", "prev_ball_vy", "traj_cursor", "traj_row", "has_racket_contact", "has_racket_contact_now", "ball_obs")


def run_variant(name, v, s, est, rng):
    L, steps = v["L"], v["steps"]
    width = 225 + 3 * L + (2 if v["target"] else 0)
    F = torch.from_numpy
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    # ---- the stand-in task object `_update_state_from_sim` and the controller read
    task = types.SimpleNamespace(cfg={"sim": {"substeps": 6 if v["velocity"] else 2}}, cfg_v2p={"grip": v["grip"]}, _is_train=True, num_envs=N, device="cpu", viewer=None,
                                 _has_racket_ball_contact=z(N, dtype=torch.bool), _has_racket_ball_contact_now=z(N, dtype=torch.bool), _ball_root_states=z(N, 13),
                                 _ball_pos=z(N, 3), _ball_vel=z(N, 3), _ball_vspin=z(N), _root_pos=z(N, 3), _root_vel=z(N, 3), _humanoid_root_states=z(N, 13),
                                 _rigid_body_pos=F(s["pos25"].copy()), _rigid_body_rot=F(s["rot25"].copy()), _rigid_body_vel=z(N, 25, 3), _racket_body_id=24,
                                 _racket_pos=z(N, 3), _racket_vel=z(N, 3), _racket_normal=z(N, 3), _lefthand=None, _racket_wrist_body_id=22,
                                 _has_bounce=z(N, dtype=torch.bool), _has_bounce_now=z(N, dtype=torch.bool), _bounce_pos=z(N, 3))
    task._humanoid_root_states[:, 0:3] = task._rigid_body_pos[:, 0]
    task._ball_vel[:, 1] = F(s["ball_state"][0, :, 8]) - 1.0  # (the ball's velocity of the step before the first)
    mvae = types.SimpleNamespace(_phase_pred=z(N), _swing_type=z(N, dtype=torch.int64), _swing_type_cycle=z(N, dtype=torch.int64))
    c = ref_ctl.PhysicsMVAEController.__new__(ref_ctl.PhysicsMVAEController)
    c.cfg = {"env": {"episodeLength": MAX_EPISODE_LENGTH, "enableEarlyTermination": v["early"]}}
    c.cfg_v2p = {"reward_type": v["reward_type"], "reward_weights": dict(WEIGHTS), "obs_ball_traj_length": L, "use_history_ball_obs": v["history"],
                 "use_random_ball_target": v["target"], "reset_reaction_nframes": REACTION_NFRAMES}
    c._max_episode_length, c._enable_early_termination, c._is_train, c.device, c.num_envs, c.headless = MAX_EPISODE_LENGTH, v["early"], True, "cpu", N, True
    c._physics_player, c._mvae_player, c._ball_out_estimator = types.SimpleNamespace(task=task), mvae, est
    c.obs_buf, c.rew_buf, c.extras = z(N, width), z(N), {}
    c.reset_buf, c.progress_buf, c._terminate_buf = torch.ones(N, dtype=torch.long), z(N, dtype=torch.long), torch.ones(N, dtype=torch.long)
    c._reward_scales = dict(SCALES)
    c._obs_ball_traj_length = L
    c._num_humanoid_bodies, c._racket_body_id, c._head_body_id = 24, 24, 13
    c._ball_traj, c._ball_obs = z(N, 100, 3), z(N, L, 3)
    c._bounce_in, c._est_bounce_pos, c._est_bounce_time, c._est_bounce_in, c._est_max_height = z(N, dtype=torch.bool), z(N, 3), z(N), z(N, dtype=torch.bool), z(N)
    c._court_min, c._court_max = torch.FloatTensor(COURT_MIN), torch.FloatTensor(COURT_MAX)
    c._tar_time, c._tar_time_total, c._tar_action = z(N, dtype=torch.long), z(N, dtype=torch.long), z(N, dtype=torch.long)
    c._target_bounce_pos = z(N, 3)
    c._target_bounce_pos[:] = torch.FloatTensor([0, 10, 0])
    c._target_bounce_min, c._target_bounce_max = torch.FloatTensor([-3, 9, 0]), torch.FloatTensor([3, 11, 0])
    c._reset_reaction_buf, c._reset_recovery_buf = torch.ones(N, dtype=torch.bool), z(N, dtype=torch.bool)
    c._num_reset_reaction, c._num_reset, c._distance = z(N, dtype=torch.long), z(N, dtype=torch.long), z(N)
    c._ball_pos = task._ball_pos
    traj_row, cursor = np.zeros(N, np.int64), np.zeros(N, np.int32)
    pool = F(s["pool"])
    rec = {k: [] for k in ("pre/" + x for x in STATE)}
    rec.update({k: [] for k in ("post/" + x for x in STATE[:-1] + ("ball_obs", "rew", "sub_rewards", "task_obs", "reset", "terminate", "reset_reaction", "reset_recovery", "vel_x_overflow"))})
    rec.update({"reset/ids": [], "reset/task_obs": [], "reset/ball_obs_in": []})
    cover = dict(hits=0, valid=0, net=0, out_of_court=0, nan=0, episode_end=0, reaction_due=0, missed=0, bounce_in=0, bounce_out=0, swing_a=0, swing_b=0, vel_hit=0,
                 vel_near_miss=0, overflow=0)
    actor = None

    def set_inputs(t):
        task._ball_root_states[:] = F(s["ball_state"][t])
        task._humanoid_root_states[:, 7:10] = F(s["root_vel"][t])
        task._has_bounce[:], task._has_bounce_now[:], task._bounce_pos[:] = F(s["has_bounce"][t]), F(s["has_bounce_now"][t]), F(s["bounce_pos"][t])
        if not v["velocity"]:
            task._has_racket_ball_contact[:], task._has_racket_ball_contact_now[:] = F(s["flag_contact"][t]), F(s["flag_contact_now"][t])
        mvae._phase_pred[:], mvae._swing_type[:], mvae._swing_type_cycle[:] = F(s["phase_pred"][t]), F(s["swing_type"][t]), F(s["swing_type_cycle"][t])

    def window():
        pad = torch.cat([pool[traj_row], torch.zeros(N, 100, 3)], 1)
        return pad[torch.arange(N)[:, None], torch.from_numpy(cursor.astype(np.int64))[:, None] + torch.arange(100)[None]]

    def state():
        return dict(tar_time=c._tar_time, tar_time_total=c._tar_time_total, tar_action=c._tar_action, progress=c.progress_buf, target_bounce_pos=c._target_bounce_pos,
                    bounce_in=c._bounce_in, est_bounce_pos=c._est_bounce_pos, est_bounce_time=c._est_bounce_time, est_max_height=c._est_max_height,
                    est_bounce_in=c._est_bounce_in, distance=c._distance, prev_ball_vy=task._ball_vel[:, 1], traj_cursor=torch.from_numpy(cursor),
                    traj_row=torch.from_numpy(traj_row), has_racket_contact=task._has_racket_ball_contact, has_racket_contact_now=task._has_racket_ball_contact_now,
                    ball_obs=c._ball_obs)

    def record(prefix, extra=None):
        for k, t in dict(state(), **(extra or {})).items():
            if prefix + k in rec:
                rec[prefix + k].append(t.detach().clone().numpy())

    def resets(ids, first=False):
        """`_reset_envs` (:173-201) without the MVAE player and the physics task's actor reset"""
        reaction, recovery = c._reset_reaction_buf.nonzero().flatten(), c._reset_recovery_buf.nonzero().flatten()
        everyone = (c._reset_reaction_buf + c._reset_recovery_buf).nonzero().flatten()
        if len(ids):
            c._reset_env_tensors(ids)
            c._num_reset[ids] += 1
        if len(reaction):
            rows = rng.integers(0, len(pool), len(reaction))
            traj_row[reaction.numpy()], cursor[reaction.numpy()] = rows, 0
            if not v["history"]:
                c._ball_traj[reaction] = pool[rows]
            task._has_racket_ball_contact[reaction] = 0  # (`_reset_balls`, humanoid_smpl_im_mvae.py:520)
        if len(ids):
            c._update_state()
        if len(recovery):
            c._reset_recovery_tasks(recovery)
        if len(reaction):
            c._reset_reaction_tasks(reaction, ids)
        mask = np.zeros(N, bool)
        mask[everyone.numpy()] = True
        if not first:
            rec["reset/ids"].append(mask)
            rec["reset/ball_obs_in"].append(c._ball_obs.clone().numpy())
        if len(everyone):
            c._compute_observations(everyone)
        if not first:
            rec["reset/task_obs"].append(c.obs_buf[:, 225:].numpy() * mask[:, None])

    # ---- the first reset of all envs, then episodes that end at different steps
    set_inputs(0)
    ref_task.HumanoidSMPLIMMVAE._update_state_from_sim(task)
    task._ball_vel[:, 1] = F(s["ball_state"][0, :, 8]) - 1.0
    resets(torch.arange(N), first=True)
    c.progress_buf[:] = F(s["progress0"])
    for t in range(steps):
        set_inputs(t)
        record("pre/")
        if not v["history"]:
            assert torch.equal(c._ball_traj, window()), "cursor + pool row do not restate the rolled _ball_traj"
        prev_vy, had_hit = task._ball_vel[:, 1].clone(), task._has_racket_ball_contact.clone()
        ref_task.HumanoidSMPLIMMVAE._update_state_from_sim(task)
        c._tar_time += 1
        c.progress_buf += 1
        overflow_before = 0
        c._update_state()
        c._compute_reward(None)
        c._compute_observations()
        c._compute_reset()
        c._ball_traj = c._ball_traj.roll(-1, dims=1)
        c._ball_traj[:, -1] = 0
        cursor[:] = np.minimum(cursor + 1, 100)
        # ---- what this step exercised
        now = task._has_racket_ball_contact_now
        b = task._ball_root_states
        valid, bpos, btime, _ = est.estimate(b[now]) if int(now.sum()) else (torch.zeros(0, dtype=torch.bool), None, None, None)
        vel_x = b[now][valid][:, 7:9].norm(dim=-1) if int(valid.sum()) else torch.zeros(0)
        n_over = int((vel_x >= OutGrid.VEL_X_RANGE[1]).sum())
        cover["hits"] += int(now.sum()); cover["valid"] += int(valid.sum()); cover["net"] += 0 if btime is None else int((btime == 0).sum()); cover["overflow"] += n_over
        root = task._root_pos
        cover["out_of_court"] += int(ref_ctl.check_out_of_court(root, c._court_min, c._court_max).sum())
        cover["nan"] += int(torch.isnan(c.obs_buf).any(dim=1).sum())
        cover["episode_end"] += int((c.progress_buf >= MAX_EPISODE_LENGTH - 1).sum())
        cover["reaction_due"] += int((c._tar_time == c._tar_time_total).sum())
        cover["missed"] += int(((c._tar_action == 1) & (b[:, 1] < root[:, 1] - 1)).sum())
        upd = (c._tar_action == 0) & task._has_bounce_now
        cover["bounce_in"] += int((upd & c._bounce_in).sum()); cover["bounce_out"] += int((upd & ~c._bounce_in).sum())
        sw = mvae._swing_type_cycle if v["reward_type"] == "return_w_estimate" else mvae._swing_type
        early = (sw == -1) if v["reward_type"] == "reach" else (sw >= 2)
        cover["swing_a"] += int(early.sum()); cover["swing_b"] += int((~early).sum())
        if v["velocity"]:
            dv = b[:, 8] - prev_vy
            assert float(((dv - 10).abs()).min()) > MARGIN and float(b[:, 8].abs().min()) > MARGIN
            cover["vel_hit"] += int(now.sum()); cover["vel_near_miss"] += int((~had_hit & (b[:, 8] > 0) & (dv > 9) & (dv < 10)).sum())
        # ---- margins of the comparisons of this step that the script could not settle in advance
        for k in range(2):
            assert float((root[:, k] - c._court_min[k]).abs().min()) > MARGIN and float((root[:, k] - c._court_max[k]).abs().min()) > MARGIN
        assert float((b[:, 1] - (root[:, 1] - 1)).abs().min()) > MARGIN
        for k, lines in ((0, BOUNCE_COURT[:2]), (1, BOUNCE_COURT[2:])):
            for line in lines:
                for val in (c._est_bounce_pos[:, k], task._bounce_pos[:, k]):  # (exact zeros - nothing estimated, no bounce - are exact everywhere)
                    assert not int((val != 0).sum()) or float((val[val != 0] - line).abs().min()) > MARGIN
        a = c.obs_buf[:, :225].clone().numpy()
        assert np.array_equal(a[:, 3:6], s["root_vel"][t])
        a[:, 3:6] = 0
        actor = a if actor is None else actor
        assert np.array_equal(a, actor, equal_nan=True), "the actor block moved although the poses are static"
        record("post/", dict(rew=c.rew_buf, sub_rewards=c._sub_rewards, task_obs=c.obs_buf[:, 225:], reset=c.reset_buf, terminate=c._terminate_buf,
                             reset_reaction=c._reset_reaction_buf, reset_recovery=c._reset_recovery_buf, vel_x_overflow=torch.tensor(n_over)))
        resets(c.reset_buf.nonzero().flatten())
    out = {"%s/%s" % (name, k): np.stack(x) for k, x in rec.items() if len(x) and (v["history"] or "ball_obs" not in k)}
    if v["history"]:
        out["%s/ball_obs_final" % name] = c._ball_obs.numpy().copy()
    out["%s/sub_rewards_names" % name] = np.frombuffer(c._sub_rewards_names.encode(), dtype=np.uint8).copy()
    out["%s/settings" % name] = np.array([["reach", "return", "return_w_estimate"].index(v["reward_type"]), L, int(v["history"]), int(bool(v["target"])), int(v["velocity"]),
                                          int(v["early"]), steps, ["eastern", "semi_western"].index(v["grip"])], dtype=np.int64)
    print("variant %s: %s" % (name, cover))
    return out, cover, actor, task._racket_pos.numpy().copy(), task._racket_normal.numpy().copy()


def main():
    rng = np.random.default_rng(2027)
    torch.manual_seed(2027)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        nb = cells(OutGrid.VEL_X_RANGE) * cells(OutGrid.VEL_Y_RANGE) * cells(OutGrid.VSPIN_RANGE)
        tx = rng.uniform(-1.5, 2.5, (nb, cells(OutGrid.TRAJ_X_RANGE))).astype(np.float32)
        ty = np.stack([rng.uniform(0, 25, (nb, cells(OutGrid.TRAJ_Y_RANGE))), rng.uniform(0, 2, (nb, cells(OutGrid.TRAJ_Y_RANGE)))], -1).astype(np.float32)
        fx, fy = os.path.join(d, "x.npy"), os.path.join(d, "y.npy")
        np.save(fx, tx); np.save(fy, ty)
        est = ref_out.TennisBallOutEstimator(fx, fy)
        est.params = OutGrid
        s = make_script(rng, tx, ty)
        total, actor0 = {}, None
        for name, v in VARIANTS.items():
            o, cover, actor, rpos, rnorm = run_variant(name, v, s, est, rng)
            out.update(o)
            out["%s/racket_normal" % name] = rnorm
            actor[:, 222:225] = 0  # (the racket normal follows the variant's grip: recorded per variant)
            actor0 = actor if actor0 is None else actor0
            assert np.array_equal(actor, actor0, equal_nan=True)
            for k, n in cover.items():
                total[k] = total.get(k, 0) + n
            if name == "A":
                assert cover["hits"] >= 8 and cover["valid"] >= 4 and cover["net"] >= 2 and cover["vel_hit"] >= 1 and cover["vel_near_miss"] >= 1, cover
        assert total["out_of_court"] >= 3 and total["nan"] >= 2 and total["episode_end"] >= 2 and total["reaction_due"] >= 3 and total["missed"] >= 3, total
        assert total["bounce_in"] >= 1 and total["bounce_out"] >= 1 and total["swing_a"] >= 1 and total["swing_b"] >= 1, total
    rb = np.zeros((N, 24, 13), np.float32)
    rb[:, :, 0:3], rb[:, :, 3:7] = s["pos25"][:, :24], s["rot25"][:, :24]
    rk = np.zeros((N, 13), np.float32)
    rk[:, 0:3], rk[:, 3:7] = s["pos25"][:, 24], s["rot25"][:, 24]
    out.update({"rb_state": rb, "racket_state": rk, "actor_obs": actor0, "racket_pos": rpos, "traj_out_x": tx, "traj_out_y": ty, "grids": GRIDS, "pool": s["pool"],
                "court": np.array([COURT_MIN, COURT_MAX], np.float64), "scales": np.array([SCALES[k] for k in ("pos", "phase", "bounce_pos", "bounce_time")]),
                "weights": np.array([WEIGHTS["pos"], WEIGHTS["ball_pos"]]), "max_episode_length": np.int64(MAX_EPISODE_LENGTH)})
    for k in ("ball_state", "root_vel", "has_bounce", "has_bounce_now", "bounce_pos", "flag_contact", "flag_contact_now", "phase_pred", "swing_type", "swing_type_cycle"):
        out["script/" + k] = s[k]
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.relpath(OUT, REPO), "%.2f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
