"""Readers of tests/golden/tennis_eval.npz (tools/gen_golden_tennis_eval.py) shared by the CPU and the GPU tests of the controller's
evaluation step: settings, inputs and the reference's recorded outputs of step t of a variant under the names of v2p_tennis_buffers, the
meters as [4,N] arrays in the order of `tennis_controller.METER_NAMES`, the record's frame, and the comparison both tests hold their
subject to: flags, counters and integer state exact, the step's own floats within the bounds of tests/tennis_fixture.py, the floats this
step adds (the meters, joint 0 of the record) within 8 x their recorded float32-float64 scatter and exact where that is 0 (DESIGN.md
item 14).  (Against the numpy statements the GPU tests ask for the bits; this is the rule against the reference's recorded values.)"""
import os

import numpy as np

from tests import tennis_fixture as TF
from vid2player3d_amd.tasks import tennis_controller as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tennis_eval.npz")
VARIANTS = ("V", "F")
STEP_KEYS = ("tar_time", "progress", "has_racket_contact", "has_racket_contact_now", "bounce_in", "est_bounce_in", "reset", "terminate", "reset_reaction", "reset_recovery",
             "prev_ball_vy", "est_bounce_pos", "est_bounce_time", "est_max_height", "distance", "rew", "sub_rewards")
_cache = {}


def golden():
    if "d" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["d"] = {k: z[k] for k in z.files}
    return _cache["d"]


def steps():
    return len(golden()["script/ball_state"])


def settings(name):
    """(task_settings, eval_settings) of a variant"""
    d = golden()
    rt, L, hist, target, vel, grip = [int(x) for x in d[name + "/settings"]]
    sc, w = d["scales"], d["weights"]
    st = tc.task_settings(reward_type=("reach", "return", "return_w_estimate")[rt], obs_ball_traj_length=L, use_history_ball_obs=hist, use_random_ball_target=target,
                          contact_by_velocity=vel, enable_early_termination=False, max_episode_length=int(d["episode_length"]), grip=("eastern", "semi_western")[grip],
                          court_min=d["court"][0], court_max=d["court"][1], reward_scales=dict(zip(("pos", "phase", "bounce_pos", "bounce_time"), sc)),
                          reward_weights={"pos": w[0], "ball_pos": w[1]}, grids=d["grids"])
    return st, tc.eval_settings(int(d["episode_length"]), d["body_of_smpl"])


def _player(d, t):
    n = len(d["rb_state"])
    off = d["script/offset"][t]  # (float32 sums, as the generator forms the step's positions)
    rb, rk = d["rb_state"].copy(), d["racket_state"].copy()
    rb[:, :, 0:3] = rb[:, :, 0:3] + off[:, None]
    rk[:, 0:3] = rk[:, 0:3] + off
    root_states = np.zeros((n, 13), np.float32)
    root_states[:, 0:3], root_states[:, 7:10] = rb[:, 0, 0:3], d["script/root_vel"][t]
    return dict(rb_state=rb, root_states=root_states, racket_state=rk, ball_state=d["script/ball_state"][t], wrist_link=np.full(n, 22, np.int64))


def step_inputs(name, t):
    """Every array v2p_tennis_eval_step reads at step t of a variant: the state before the step, the meters [4,N] and `dof_pos` [N,69]."""
    d, (st, _) = golden(), settings(name)
    s = _player(d, t)
    for k in ("has_bounce", "has_bounce_now", "bounce_pos", "phase_pred", "swing_type", "swing_type_cycle", "dof_pos"):
        s[k] = d["script/" + k][t]
    for k in ("tar_time", "tar_time_total", "tar_action", "progress", "target_bounce_pos", "bounce_in", "est_bounce_pos", "est_bounce_time", "est_max_height", "est_bounce_in",
              "distance", "prev_ball_vy", "traj_cursor", "has_racket_contact", "has_racket_contact_now") + tc.METER_FIELDS:
        s[k] = d["%s/pre/%s" % (name, k)][t]
    s["traj_out_x"], s["traj_out_y"] = d["traj_out_x"], d["traj_out_y"]
    s["ball_traj"] = d["pool"][d[name + "/pre/traj_row"][t]]
    s["ball_obs"] = d[name + "/pre/ball_obs"][t] if st["use_history"] else None
    s["vel_x_overflow"] = np.zeros(1, np.int64)
    return s


def step_expected(name, t):
    """What the reference recorded after step t: the step's outputs, the meters, and the record's frame (dict `record`)."""
    d, (st, _) = golden(), settings(name)
    o = {k: d["%s/post/%s" % (name, k)][t] for k in STEP_KEYS + tc.METER_FIELDS}
    o["vel_x_overflow"] = d[name + "/post/vel_x_overflow"][t]
    walk = d["walkers"]
    actor, rpos = d["actor_obs"].copy(), d["racket_pos"].copy()
    actor[walk], rpos[walk] = d[name + "/post/actor_walk"][t], d[name + "/post/racket_pos_walk"][t]
    actor[:, 3:6] = d["script/root_vel"][t]
    o["racket_pos"], o["racket_normal"] = rpos, d["racket_normal"]
    o["obs"] = np.concatenate([actor, d[name + "/post/task_obs"][t]], 1)
    if st["use_history"]:
        o["ball_obs"] = d[name + "/post/ball_obs"][t]
    else:
        o["traj_cursor"] = d[name + "/post/traj_cursor"][t]
    o["record"] = dict({k: d["%s/rec/%s" % (name, k)][t] for k in tc.RECORD_NAMES[1:]}, joint_rot=d["rec/joint_rot"][t])
    return o


def within_scatter(got, want, scatter, what):
    """|got - want| <= 8 x scatter, bit-equal where the scatter is 0"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if scatter == 0:
        assert np.array_equal(got, want), "%s: differs where the recorded scatter is 0 (first at %s)" % (what, np.argwhere(got != want)[:1])
        return
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    assert err <= 8 * scatter, "%s: %.3e > 8 x scatter %.3e" % (what, err, scatter)


def compare(name, got, want, what):
    """`got`: the arrays a subject produced for a step (and `record`: its frame, or absent), `want`: step_expected(...)."""
    d = golden()
    TF.compare(got, {k: v for k, v in want.items() if k in TF.EXACT or k in TF.FLOATS}, what)
    assert np.array_equal(np.asarray(got["meter_count"]), want["meter_count"]), what + ": meter counts"
    for f in ("meter_sum", "meter_avg", "meter_max"):
        for m, meter in enumerate(tc.METER_NAMES):
            within_scatter(np.asarray(got[f])[m], want[f][m], float(d["%s/post/%s/scatter" % (name, f)][m]), "%s: %s of %s" % (what, f, meter))
    if got.get("record") is not None:
        g, w = got["record"], want["record"]
        for k in tc.RECORD_NAMES[1:]:
            assert np.array_equal(np.asarray(g[k]), w[k], equal_nan=True), "%s: record %s" % (what, k)
        jr = np.asarray(g["joint_rot"])
        within_scatter(jr[:, 0], w["joint_rot"][:, 0], float(d[name + "/rec/joint_rot/scatter"]), what + ": joint 0 of the record")
        assert np.array_equal(jr[:, 1:], w["joint_rot"][:, 1:]), what + ": joints 1..23 of the record are copies of the DoF positions"


# ------------------------------------------------------------------------------------------------------------------ the controller (GPU tests, tools)
DEV = "cuda:0"
EPISODE_LENGTH = 5


def near_pool():
    """`flag_reset_fixture.make_pool` with the launch points two metres in front of the players instead of across the net: at 25 m/s the
    ball is behind a player within a handful of steps, so a short run raises recovery flags (and fills the meters) without a hit"""
    from tests import flag_reset_fixture as FF

    pool = FF.make_pool()
    pool[:, 1] -= 23.5  # launch y 12 .. 13 -> -11.5 .. -10.5; the players stand around y = -13
    return pool


def eval_controller(n, episode_length=EPISODE_LENGTH, units=None, pool=None):
    """(ctl, task, player, target, policy): a `TennisControllerEval` built like `flag_reset_fixture.controller` - a racket + ball batch
    over an offline pool, cfg v2p `task_reset: 'device'`, `_reset_root_xy` set - with the generator in test mode (is_train false), the
    imitation target, a random low-level policy and a random `ControllerPolicy` attached.  units: the tools' network widths; pool: the
    ball pool, default `flag_reset_fixture.make_pool()`."""
    import torch

    from tests import flag_reset_fixture as FF
    from tests import mvae_fixture as MF
    from tests import mvae_target_fixture as FX
    from tests import policies_fixture as PF
    from vid2player3d_amd import ball_traj, mvae
    from vid2player3d_amd import mvae_target as mt
    from vid2player3d_amd import policies as P
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall

    torch.manual_seed(7)
    tg, g = TF.golden(), FX.golden()
    gen = ball_traj.TennisBallGeneratorOffline(FF.make_pool() if pool is None else pool, sample_random=True, device=DEV, seed=3)
    cfg = PF._sim_cfg(n, {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                          "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                          "reset_reaction_nframes": 6, "ball_traj_out_x_file": tg["traj_out_x"], "ball_traj_out_y_file": tg["traj_out_y"], "add_residual_dof": "euler",
                          "add_residual_root": True, "residual_root_scale": 0.02, "fix_head_orientation": True, "task_reset": "device"})
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in tg["grids"]]

    ctl = tc.TennisControllerEval(task, {"env": {"episodeLength": int(episode_length)}, "v2p": cfg["v2p"]}, params=SmallGrid, seed=FF.SEED)
    w, avg, std = MF.weights()
    rot = g["H/in/joint_rotmat"][0][np.arange(n) % 12]
    init = np.tile(avg, (n, 1)).astype(np.float32)
    init[:, 2] = 0.92
    init[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(n, 144)
    bind = g["H/joint_pos_bind"][0]
    player = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler", "seed": FF.SEED}, n, w, avg, std, init, bind - bind[:1], False, DEV)
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)
    ctl._reset_root_xy = torch.as_tensor(FF.root_xy_table(n), device=DEV).contiguous()
    kw = {} if units is None else {"units": units}
    ctl.attach_low_level_policy(P.LowLevelPolicy(target, PF.random_actors(1, 734, 75, **kw)[0], PF.random_norms(1, 734)[0], 5.0, 1.0))
    task.reset()
    ctl.reset()
    dim, act = int(ctl.obs_buf.shape[1]), ctl.get_action_size()
    policy = P.ControllerPolicy(ctl, PF.random_actors(1, dim, act, seed=51, **kw)[0], PF.random_norms(1, dim, ("mean_var", "mean_var"), seed=61)[0], 5.0, 1.0)
    return ctl, task, player, target, policy
