"""Golden data of the tennis controller's evaluation step, recorded from the reference itself: tests/golden/tennis_eval.npz.

`MVAEControllerVis` (vid2player/env/tasks/mvae_controller_vis.py, what `run.py --test` runs) is imported on the CPU with the shim and
the inert stand-ins of tools/gen_golden_tennis_controller.py (that module is imported for them, for its small estimator grids and for
the margins of an estimator hit).  An object made with `__new__` gets its attributes set by hand - scripted player, ball and motion
generator tensors for N = 80 envs - and for T consecutive steps the reference's OWN methods run on it:
`HumanoidSMPLIMMVAE._update_state_from_sim` with `_is_train` false (the velocity rule of the racket hit, the racket normal,
`_joint_rot`), `PhysicsMVAEController._update_state`, `_compute_reward`, `_compute_observations`, `MVAEControllerVis._compute_reset`
with its `_compute_stats`, the roll of `physics_step`, `MVAEControllerVis.render_vis` (cfg env.record: the record lines :140-146; at the
last step with select_best, whose candidate list is caught from `render_one_result`), then `_reset_env_tensors` /
`_reset_recovery_tasks` / `_reset_reaction_tasks` / `_compute_observations(ids)` for the envs the flags name.

Two variants share the script: V reads the racket hit from the ball's velocity (6 substeps) under `return_w_estimate` with a random
target, F takes the contact flags under `reach` with the history window.  The poses are static except for eight envs whose whole body
walks (the distance `select_best` sorts by); the DoF positions change every step.

Float results that are new in this step - the meters' sum / avg / max and joint 0 of `_joint_rot` - are stored with their
float32-float64 scatter: the reference's `_compute_stats` and `quaternion_to_angle_axis` run a second time on float64 copies of what
they read.  The generator asserts that every float compared with a threshold stays MARGIN away from it and that every case of the
census at the end of `run_variant` occurs.  Only arrays are stored.  Run where the reference exists:
    python tools/gen_golden_tennis_eval.py
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import gen_golden_tennis_controller as base  # noqa: E402  (installs the shim and the stand-ins, imports the reference's controller)
from gen_golden_tennis_controller import MARGIN, OutGrid, _Sink, away, cells, hit_ok, ref_ctl, ref_out, ref_task, torch  # noqa: E402

for absent in ("smpl_visualizer.vis_scenepic", "smpl_visualizer.vis"):
    try:
        __import__(absent)
    except Exception:
        sys.modules[absent] = _Sink(absent)

import env.tasks.mvae_controller_vis as ref_vis  # noqa: E402
from utils.common import AverageMeterUnSync  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "tennis_eval.npz")
N, T = 80, 12
EPISODE_LENGTH, REACTION_NFRAMES = 7, 3
COURT_MIN, COURT_MAX = base.COURT_MIN, base.COURT_MAX  # the training court: env 0 stands outside it and is not terminated
SCALES, WEIGHTS = base.SCALES, base.WEIGHTS
WALKERS = np.arange(8, 16)   # their bodies move: candidates of select_best (8..11), forehand only (12, 13), as it comes (14, 15)
BEHIND = np.arange(16, 24)   # the ball stays behind them, never hit: the recovery flag by `ball_y < root_y - 1` alone, again and again
SLOW = np.arange(24, 32)     # a slow ball in front of them, never hit: the recovery flag by `|ball_vy| < 2` alone
TWICE = np.arange(32, 48)    # two hits
METERS = ("hit_rate", "fh_ratio", "bounce_in_rate", "bounce_in_pos_error")
VARIANTS = {
    "V": dict(reward_type="return_w_estimate", history=False, target=True, velocity=True, L=10, grip="eastern"),
    "F": dict(reward_type="reach", history=True, target=False, velocity=False, L=10, grip="eastern"),
}


def make_script(rng, est, tx, ty):
    s = {}
    pos = np.zeros((N, 25, 3), np.float32)
    pos[:, 0] = np.stack([rng.uniform(-3, 3, N), rng.uniform(-14, -10, N), rng.uniform(0.8, 1.0, N)], -1)
    pos[:, 1:] = pos[:, :1] + rng.uniform(-0.8, 0.8, (N, 24, 3))
    pos[0, :, 0] += np.float32(6.0) - pos[0, 0, 0]  # root x = 6: outside the training court
    rot = rng.normal(0, 1, (N, 25, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True) * rng.uniform(0.98, 1.02, (N, 25, 1))
    rot[1, 0] = np.float32([0.0, 0.0, 0.0, 1.0])   # the identity as a root rotation (x^2 + y^2 + z^2 = 0) ...
    rot[2, 0, 3] = -abs(rot[2, 0, 3])              # ... and one with w < 0
    pos[3, 7, 1] = np.nan                          # a NaN in a body position: the observation row carries it, nothing ends
    offset = np.zeros((T, N, 3), np.float32)
    offset[:, WALKERS, 0:2] = np.cumsum(rng.normal(0, 1, (T, len(WALKERS), 2)) * np.linspace(0.02, 0.3, len(WALKERS))[None, :, None], 0)
    s["pos25"], s["rot25"], s["offset"] = pos, rot.astype(np.float32), offset
    root = pos[None, :, 0] + offset  # [T,N,3] float32, as the steps form it
    s["dof_pos"] = (rng.integers(-64, 65, (T, N, 69)) / 64.0).astype(np.float32)
    t1 = np.where(rng.uniform(size=N) < 0.5, rng.integers(0, 9, N), 99)
    t1[WALKERS], t1[BEHIND], t1[SLOW], t1[[0, 3]] = rng.integers(1, 5, len(WALKERS)), 99, 99, (2, 3)
    t1[TWICE] = rng.integers(0, 3, len(TWICE))
    t2 = np.full(N, 99)
    t2[TWICE] = t1[TWICE] + rng.integers(4, 7, len(TWICE))
    # the ball flies out (and, for variant F, the contact flag stands) for two steps after a hit of a TWICE env or a walker, for good after the others'
    out = lambda t, e: (t1[e] <= t < t1[e] + 2) or (t2[e] <= t < t2[e] + 2) if e in TWICE or e in WALKERS else t >= t1[e]
    ball = np.zeros((T, N, 13), np.float32)
    ball[:, :, 6] = 1
    for t in range(T):
        for e in range(N):
            now = t in (t1[e], t2[e])
            for _ in range(4000):
                b = np.zeros(13)
                y = rng.uniform(-3.5, -1.3) if e in BEHIND else (rng.uniform(-0.7, 6.0) if e in SLOW or e in WALKERS or e in TWICE else rng.uniform(-2.5, 6.0))
                b[0:3] = [rng.uniform(-3, 3), root[t, e, 1] + y, rng.choice([rng.uniform(0.3, 2.9), rng.uniform(3.1, 3.4)], p=[0.9, 0.1])]
                b[7:10] = [rng.uniform(-3, 3), rng.uniform(8, 16) if out(t, e) else rng.uniform(-25, -15), rng.uniform(-2.6, 2.6)]
                if e in SLOW:
                    b[8] = rng.choice([-1, 1]) * rng.uniform(0.2, 1.8)
                b[10:13] = rng.normal(0, 6.0, 3)
                b = b.astype(np.float32).astype(np.float64)
                if not away(b[1] - (float(root[t, e, 1]) - 1.0), [0.0]) or (now and not hit_ok(b, tx, ty)):
                    continue
                if now and e in WALKERS:  # their hit must land in the court, by the reference's own estimator
                    ok, bp, _, _ = est.estimate(torch.from_numpy(b[None].astype(np.float32)))
                    if not bool(ok[0]) or not (-4.11 < float(bp[0, 0]) < 4.11 and 0 < float(bp[0, 1]) < 11.89):
                        continue
                break
            else:
                raise AssertionError("no draw with margins for env %d step %d" % (e, t))
            ball[t, e, [0, 1, 2, 7, 8, 9, 10, 11, 12]] = b[[0, 1, 2, 7, 8, 9, 10, 11, 12]]
    s["ball_state"], s["t1"], s["t2"] = ball, t1, t2
    s["root_vel"] = rng.normal(0, 1.5, (T, N, 3)).astype(np.float32)
    s["has_bounce_now"] = rng.uniform(size=(T, N)) < 0.15
    s["has_bounce"] = np.cumsum(s["has_bounce_now"], 0) > 0
    bp = np.stack([rng.uniform(-6, 6, (T, N)), rng.uniform(-3, 15, (T, N)), np.full((T, N), 0.1)], -1)
    for k, lines in ((0, base.BOUNCE_COURT[:2]), (1, base.BOUNCE_COURT[2:])):
        for line in lines:
            bp[..., k] = np.where(np.abs(bp[..., k] - line) < 0.02, bp[..., k] + 0.05, bp[..., k])
    s["bounce_pos"] = (bp * s["has_bounce"][..., None]).astype(np.float32)
    steps = np.arange(T)[:, None]
    s["flag_contact_now"] = (steps == t1[None]) | (steps == t2[None])
    s["flag_contact"] = np.array([[bool(out(t, e)) for e in range(N)] for t in range(T)])
    s["phase_pred"] = rng.uniform(2.0, 4.2, (T, N)).astype(np.float32)
    s["swing_type"] = rng.integers(-1, 4, (T, N)).astype(np.int64)
    cycle = rng.integers(-1, 3, (T, N)).astype(np.int64)
    cycle[:, WALKERS[:4]], cycle[:, WALKERS[4:6]], cycle[:, WALKERS[6]] = 2, 1, -1
    # a standing env travels no distance: none may become a candidate, or select_best's order would hang on how a sort breaks ties.
    # Its bounce-in rate stays 1 only if every update is a hit, so every hit of a standing env is a forehand
    for e in np.setdiff1d(np.arange(N), WALKERS):
        for t in (t1[e], t2[e]):
            if t < T:
                cycle[t, e] = 1
    s["swing_type_cycle"] = cycle
    s["pool"] = np.cumsum(rng.normal(0, 0.3, (6, 100, 3)), 1).astype(np.float32) + np.array([0, -11, 1], np.float32)
    s["progress0"] = rng.integers(0, 6, N).astype(np.int64)
    return s


STATE = base.STATE


def run_variant(name, v, s, est, rng):
    L = v["L"]
    width = 225 + 3 * L + (2 if v["target"] else 0)
    F = torch.from_numpy
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    task = types.SimpleNamespace(cfg={"sim": {"substeps": 6 if v["velocity"] else 2}}, cfg_v2p={"grip": v["grip"]}, _is_train=False, num_envs=N, device="cpu", viewer=None,
                                 _has_racket_ball_contact=z(N, dtype=torch.bool), _has_racket_ball_contact_now=z(N, dtype=torch.bool), _ball_root_states=z(N, 13),
                                 _ball_pos=z(N, 3), _ball_vel=z(N, 3), _ball_vspin=z(N), _root_pos=z(N, 3), _root_vel=z(N, 3), _humanoid_root_states=z(N, 13),
                                 _rigid_body_pos=F(s["pos25"].copy()), _rigid_body_rot=F(s["rot25"].copy()), _rigid_body_vel=z(N, 25, 3), _racket_body_id=24,
                                 _racket_pos=z(N, 3), _racket_vel=z(N, 3), _racket_normal=z(N, 3), _lefthand=None, _racket_wrist_body_id=22,
                                 _has_bounce=z(N, dtype=torch.bool), _has_bounce_now=z(N, dtype=torch.bool), _bounce_pos=z(N, 3), _dof_pos=z(N, 69), _joint_rot=z(N, 24, 3))
    ref_task.HumanoidSMPLIMMVAE._build_mujoco_smpl_transform(task)
    task._ball_vel[:, 1] = F(s["ball_state"][0, :, 8]) - 1.0
    mvae = types.SimpleNamespace(_phase_pred=z(N), _swing_type=z(N, dtype=torch.int64), _swing_type_cycle=z(N, dtype=torch.int64))
    c = ref_vis.MVAEControllerVis.__new__(ref_vis.MVAEControllerVis)
    c.cfg = {"env": {"episodeLength": EPISODE_LENGTH, "enableEarlyTermination": False, "record": True, "num_rec_frames": 10 ** 9}}
    c.cfg_v2p = {"reward_type": v["reward_type"], "reward_weights": dict(WEIGHTS), "obs_ball_traj_length": L, "use_history_ball_obs": v["history"],
                 "use_random_ball_target": v["target"], "reset_reaction_nframes": REACTION_NFRAMES}
    c._max_episode_length, c._enable_early_termination, c._is_train, c.device, c.num_envs, c.headless = EPISODE_LENGTH, False, False, "cpu", N, True
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
    c.frame_index = 0
    for k in ("joint_rot_all", "root_pos_all", "ball_pos_all", "target_pos_all", "phase_all", "swing_type_all"):
        setattr(c, k, None)
    # the float64 shadow of `_compute_stats`: the same method on float64 meters and float64 copies of the two positions it subtracts
    sh = types.SimpleNamespace(_physics_player=c._physics_player, _mvae_player=mvae)
    for who in (c, sh):
        for m in METERS:
            setattr(who, m, AverageMeterUnSync(dim=N))
    for m in METERS:
        meter = getattr(sh, m)
        meter.sum, meter.avg, meter.max = meter.sum.double(), meter.avg.double(), meter.max.double()
    meters = lambda who, dt: {f: np.stack([getattr(getattr(who, m), f).numpy().astype(dt if f != "count" else np.int64) for m in METERS]) for f in ("sum", "count", "avg", "max")}
    traj_row, cursor = np.zeros(N, np.int64), np.zeros(N, np.int32)
    pool = F(s["pool"])
    post_keys = STATE[:-1] + ("ball_obs", "rew", "sub_rewards", "task_obs", "reset", "terminate", "reset_reaction", "reset_recovery", "vel_x_overflow")
    rec = {k: [] for k in ["pre/" + x for x in STATE] + ["post/" + x for x in post_keys]}
    rec.update({k: [] for k in ("pre/meter_sum", "pre/meter_count", "pre/meter_avg", "pre/meter_max", "post/meter_sum", "post/meter_count", "post/meter_avg", "post/meter_max",
                                "post/meter_sum64", "post/meter_avg64", "post/meter_max64", "post/root_rot64", "post/actor_walk", "post/racket_pos_walk")})
    cover = dict(react_hit_bounced=0, react_hit_no_bounce=0, react_miss=0, recover_hit=0, recover_behind=0, recover_slow=0, reset_over_recovery=0, reset_over_reaction=0,
                 at_length=0, past_length=0, error_skipped=0, max_rises=0, max_stays=0, fh_types=set(), nan_kept=0, out_kept=0, hits=0, valid=0)
    actor = None

    def set_inputs(t):
        task._rigid_body_pos[:] = F(s["pos25"]) + F(s["offset"][t])[:, None]
        task._humanoid_root_states[:, 0:3] = task._rigid_body_pos[:, 0]
        task._dof_pos[:] = F(s["dof_pos"][t])
        task._ball_root_states[:] = F(s["ball_state"][t])
        task._humanoid_root_states[:, 7:10] = F(s["root_vel"][t])
        task._has_bounce[:], task._has_bounce_now[:], task._bounce_pos[:] = F(s["has_bounce"][t]), F(s["has_bounce_now"][t]), F(s["bounce_pos"][t])
        if not v["velocity"]:
            task._has_racket_ball_contact[:], task._has_racket_ball_contact_now[:] = F(s["flag_contact"][t]), F(s["flag_contact_now"][t])
        mvae._phase_pred[:], mvae._swing_type[:], mvae._swing_type_cycle[:] = F(s["phase_pred"][t]), F(s["swing_type"][t]), F(s["swing_type_cycle"][t])

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
        for f, a in meters(c, np.float32).items():
            rec[prefix + "meter_" + f].append(a)

    def resets(ids):
        """`_reset_envs` (physics_mvae_controller.py:173-201) without the MVAE player and the physics task's actor reset"""
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
        if len(everyone):
            c._compute_observations(everyone)

    set_inputs(0)
    ref_task.HumanoidSMPLIMMVAE._update_state_from_sim(task)
    task._ball_vel[:, 1] = F(s["ball_state"][0, :, 8]) - 1.0
    resets(torch.arange(N))
    c.progress_buf[:] = F(s["progress0"])
    best = None
    for t in range(T):
        set_inputs(t)
        record("pre/")
        prev_vy, max_before = task._ball_vel[:, 1].clone(), meters(c, np.float32)["max"]
        count_before = meters(c, np.float32)["count"]
        ref_task.HumanoidSMPLIMMVAE._update_state_from_sim(task)
        c._tar_time += 1
        c.progress_buf += 1
        c._update_state()
        c._compute_reward(None)
        c._compute_observations()
        c._compute_reset()
        # the float64 shadow: the flags and the estimate are this step's
        sh._reset_recovery_buf, sh._est_bounce_in = c._reset_recovery_buf, c._est_bounce_in
        sh._est_bounce_pos, sh._target_bounce_pos = c._est_bounce_pos.double(), c._target_bounce_pos.double()
        ref_vis.MVAEControllerVis._compute_stats(sh)
        root_rot64 = ref_task.quaternion_to_angle_axis(task._rigid_body_rot[:, 0][..., [3, 0, 1, 2]].double())
        c._ball_traj = c._ball_traj.roll(-1, dims=1)
        c._ball_traj[:, -1] = 0
        cursor[:] = np.minimum(cursor + 1, 100)
        if t == T - 1:  # the last frame closes the record: select_best's own lines, the candidate list caught from the calls it makes
            c.cfg["env"].update(num_rec_frames=T, select_best=True, num_eg=N + 1, start_eg_id=0)
            best = []
            c.render_one_result = lambda env_id, eg_id: best.append(int(env_id))
            try:
                ref_vis.MVAEControllerVis.render_vis(c)
            except IndexError:  # (the list of candidates is shorter than num_eg)
                pass
        else:
            ref_vis.MVAEControllerVis.render_vis(c)
        if t == 0:  # (on the CPU `.cpu()` copies nothing: the first frame of each list would alias the live tensor and follow it)
            for k in ("joint_rot_all", "root_pos_all", "ball_pos_all", "target_pos_all", "phase_all", "swing_type_all"):
                setattr(c, k, getattr(c, k).clone())
        # ---- what this step exercised, and the margins of its comparisons
        b, root = task._ball_root_states, task._root_pos
        hit, now, act0 = task._has_racket_ball_contact, task._has_racket_ball_contact_now, c._tar_action == 0
        in_time, bounced = c._tar_time >= c._tar_time_total, task._has_bounce
        behind, slow = b[:, 1] < root[:, 1] - 1, b[:, 8].abs() < 2
        done = c.reset_buf > 0
        assert torch.equal(done, c.progress_buf > EPISODE_LENGTH) and torch.equal(c._terminate_buf, c.reset_buf)
        cover["react_hit_bounced"] += int((hit & act0 & bounced & in_time & ~done).sum())
        cover["react_hit_no_bounce"] += int((hit & act0 & ~bounced & in_time & ~done & ~c._reset_reaction_buf).sum())
        cover["react_miss"] += int((~hit & in_time & ~done).sum())
        swing = ~act0 & ~done
        cover["recover_hit"] += int((swing & hit & ~behind & ~slow).sum())
        cover["recover_behind"] += int((swing & ~hit & behind & ~slow).sum())
        cover["recover_slow"] += int((swing & ~hit & ~behind & slow).sum())
        cover["reset_over_recovery"] += int((done & ~act0 & (hit | behind | slow)).sum())
        cover["reset_over_reaction"] += int((done & ~((hit & act0 & bounced & in_time) | (~hit & in_time))).sum())
        assert not bool((done & c._reset_recovery_buf).any()) and bool(c._reset_reaction_buf[done].all())
        cover["at_length"] += int((c.progress_buf == EPISODE_LENGTH).sum())
        cover["past_length"] += int((c.progress_buf == EPISODE_LENGTH + 1).sum())
        upd = c._reset_recovery_buf
        cover["error_skipped"] += int((upd & ~c._est_bounce_in).sum())
        after = meters(c, np.float32)
        grew = after["max"] > max_before
        cover["max_rises"] += int(grew.sum())
        cover["max_stays"] += int(((after["count"] > count_before) & ~grew & (max_before > 0)).sum())
        cover["fh_types"] |= set(int(x) for x in mvae._swing_type_cycle[upd])
        cover["nan_kept"] += int((torch.isnan(c.obs_buf).any(dim=1) & ~done).sum())
        cover["out_kept"] += int((ref_ctl.check_out_of_court(root, c._court_min, c._court_max) & ~done).sum())
        cover["hits"] += int(now.sum())
        cover["valid"] += int(est.estimate(b[now])[0].sum()) if int(now.sum()) else 0
        assert float((b[:, 8].abs() - 2).abs().min()) > MARGIN and float((b[:, 1] - (root[:, 1] - 1)).abs().min()) > MARGIN
        if v["velocity"]:
            dv = b[:, 8] - prev_vy
            assert float(((dv - 10).abs()).min()) > MARGIN and float(b[:, 8].abs().min()) > MARGIN
        for k, lines in ((0, base.BOUNCE_COURT[:2]), (1, base.BOUNCE_COURT[2:])):
            for line in lines:
                for val in (c._est_bounce_pos[:, k], task._bounce_pos[:, k]):
                    assert not int((val != 0).sum()) or float((val[val != 0] - line).abs().min()) > MARGIN
        for k in (0, 1):  # the meters are exact in the 0 / 1 valued rows, and their float32 and float64 forms agree on the counts
            assert np.array_equal(after["sum"][k], np.round(after["sum"][k])) and np.array_equal(after["count"], meters(sh, np.float64)["count"])
        # ---- the actor block: static but for the root velocity and the walkers' rows
        a = c.obs_buf[:, :225].clone().numpy()
        assert np.array_equal(a[:, 3:6], s["root_vel"][t])
        a[:, 3:6] = 0
        rec["post/actor_walk"].append(a[WALKERS].copy())
        rec["post/racket_pos_walk"].append(task._racket_pos[WALKERS].numpy().copy())
        a[WALKERS] = 0
        actor = a if actor is None else actor
        assert np.array_equal(a, actor, equal_nan=True), "the actor block of a standing env moved"
        record("post/", dict(rew=c.rew_buf, sub_rewards=c._sub_rewards, task_obs=c.obs_buf[:, 225:], reset=c.reset_buf, terminate=c._terminate_buf,
                             reset_reaction=c._reset_reaction_buf, reset_recovery=c._reset_recovery_buf,
                             vel_x_overflow=torch.tensor(int((b[now][est.estimate(b[now])[0]][:, 7:9].norm(dim=-1) >= OutGrid.VEL_X_RANGE[1]).sum()) if int(now.sum()) else 0)))
        for f, arr in meters(sh, np.float64).items():
            if f != "count":
                rec["post/meter_%s64" % f].append(arr)
        rec["post/root_rot64"].append(root_rot64.numpy().copy())
        resets(c.reset_buf.nonzero().flatten())
    out = {"%s/%s" % (name, k): np.stack(x) for k, x in rec.items() if len(x) and (v["history"] or "ball_obs" not in k)}
    # ---- the record, frame-major, and select_best
    frames = {"joint_rot": c.joint_rot_all, "root_pos": c.root_pos_all, "ball_pos": c.ball_pos_all, "target_pos": c.target_pos_all, "phase": c.phase_all,
              "swing_type_cycle": c.swing_type_all}
    for k, x in frames.items():
        assert x.shape[:2] == (N, T)
        out["%s/rec/%s" % (name, k)] = np.ascontiguousarray(np.swapaxes(x.numpy(), 0, 1))
    dist = (c.root_pos_all[:, 1:] - c.root_pos_all[:, :-1]).norm(dim=-1).sum(dim=-1).numpy()
    in_rate, fh = c.bounce_in_rate.avg.numpy(), c.fh_ratio.avg.numpy()
    assert float(np.abs(in_rate - 0.95).min()) > MARGIN and float(np.abs(fh - 0.6).min()) > MARGIN
    gaps = np.diff(np.sort(dist[best]))
    assert len(best) >= 2 and float(gaps.min()) > MARGIN, "candidates of select_best need distances apart"
    assert int(((in_rate <= 0.95) & (fh < 0.6)).sum()) >= 1 and int(((in_rate > 0.95) & (fh >= 0.6)).sum()) >= 1
    out["%s/best/ids" % name], out["%s/best/dist" % name] = np.array(best, np.int64), dist.astype(np.float32)
    out["%s/sub_rewards_names" % name] = np.frombuffer(c._sub_rewards_names.encode(), dtype=np.uint8).copy()
    out["%s/settings" % name] = np.array([["reach", "return", "return_w_estimate"].index(v["reward_type"]), L, int(v["history"]), int(bool(v["target"])), int(v["velocity"]),
                                          ["eastern", "semi_western"].index(v["grip"])], dtype=np.int64)
    for f in ("sum", "avg", "max"):
        a32, a64 = out["%s/post/meter_%s" % (name, f)], out.pop("%s/post/meter_%s64" % (name, f))
        out["%s/post/meter_%s/scatter" % (name, f)] = np.abs(a32.astype(np.float64) - a64).reshape(T, 4, N).max(axis=(0, 2))  # per meter
    root_rot64 = out.pop("%s/post/root_rot64" % name)
    out["%s/rec/joint_rot/scatter" % name] = np.array(np.abs(out["%s/rec/joint_rot" % name][:, :, 0].astype(np.float64) - root_rot64).max())
    counts = out["%s/post/meter_count" % name][-1]
    assert (counts[0] == 0).any() and (counts[0] == 1).any() and (counts[0] >= 3).any(), "a meter updated 0, 1 and >= 3 times"
    print("variant %s: %s; select_best %s" % (name, cover, best))
    return out, cover, actor, task._racket_pos.numpy().copy(), task._racket_normal.numpy().copy(), np.array(task._mujoco_2_smpl, np.int32)


def main():
    rng = np.random.default_rng(2031)
    torch.manual_seed(2031)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        nb = cells(OutGrid.VEL_X_RANGE) * cells(OutGrid.VEL_Y_RANGE) * cells(OutGrid.VSPIN_RANGE)
        tx = rng.uniform(-1.5, 2.5, (nb, cells(OutGrid.TRAJ_X_RANGE))).astype(np.float32)
        ty = np.stack([rng.uniform(0, 25, (nb, cells(OutGrid.TRAJ_Y_RANGE))), rng.uniform(0, 2, (nb, cells(OutGrid.TRAJ_Y_RANGE)))], -1).astype(np.float32)
        fx, fy = os.path.join(d, "x.npy"), os.path.join(d, "y.npy")
        np.save(fx, tx); np.save(fy, ty)
        est = ref_out.TennisBallOutEstimator(fx, fy)
        est.params = OutGrid
        s = make_script(rng, est, tx, ty)
        actor0 = joints0 = None
        for name, v in VARIANTS.items():
            o, cover, actor, rpos, rnorm, body_of_smpl = run_variant(name, v, s, est, rng)
            jr = o.pop("%s/rec/joint_rot" % name)  # (the poses and the DoFs are the script's: one copy serves both variants)
            joints0 = jr if joints0 is None else joints0
            assert np.array_equal(jr, joints0)
            out.update(o)
            actor0 = actor if actor0 is None else actor0
            assert np.array_equal(actor, actor0, equal_nan=True)
            for k in ("react_hit_bounced", "react_hit_no_bounce", "react_miss", "recover_hit", "recover_behind", "recover_slow", "reset_over_recovery", "reset_over_reaction",
                      "at_length", "past_length", "error_skipped", "max_rises", "max_stays", "nan_kept", "out_kept", "valid"):
                assert cover[k] >= 1, (name, k, cover)
            assert {-1, 1, 2} <= cover["fh_types"], cover
    rb = np.zeros((N, 24, 13), np.float32)
    rb[:, :, 0:3], rb[:, :, 3:7] = s["pos25"][:, :24], s["rot25"][:, :24]
    rk = np.zeros((N, 13), np.float32)
    rk[:, 0:3], rk[:, 3:7] = s["pos25"][:, 24], s["rot25"][:, 24]
    out.update({"rb_state": rb, "racket_state": rk, "actor_obs": actor0, "racket_pos": rpos, "racket_normal": rnorm, "rec/joint_rot": joints0, "body_of_smpl": body_of_smpl,
                "walkers": WALKERS.astype(np.int64), "traj_out_x": tx, "traj_out_y": ty, "grids": base.GRIDS, "pool": s["pool"],
                "court": np.array([COURT_MIN, COURT_MAX], np.float64), "scales": np.array([SCALES[k] for k in ("pos", "phase", "bounce_pos", "bounce_time")]),
                "weights": np.array([WEIGHTS["pos"], WEIGHTS["ball_pos"]]), "episode_length": np.int64(EPISODE_LENGTH)})
    for k in ("ball_state", "root_vel", "has_bounce", "has_bounce_now", "bounce_pos", "flag_contact", "flag_contact_now", "phase_pred", "swing_type", "swing_type_cycle",
              "dof_pos", "offset"):
        out["script/" + k] = s[k]
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.relpath(OUT, REPO), "%.2f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
