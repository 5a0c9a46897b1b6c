"""Readers of tests/golden/tennis_controller.npz (tools/gen_golden_tennis_controller.py) shared by the CPU and the GPU tests of the tennis
controller's task step: settings, inputs and expected outputs of step t of a variant under the names of v2p_tennis_buffers, and the
comparison both tests hold their subject to."""
import os

import numpy as np

from tests.gpu_util import close
from vid2player3d_amd.tasks import tennis_controller as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tennis_controller.npz")
VARIANTS = ("A", "B", "C", "D")
OBS_TOL, REW_TOL = 5e-6, 5e-5  # the tolerances of test_gpu_task_ops.py for observations / rewards
EXACT = ("tar_time", "progress", "has_racket_contact", "has_racket_contact_now", "bounce_in", "est_bounce_in", "traj_cursor", "reset", "terminate", "reset_reaction",
         "reset_recovery", "vel_x_overflow")
FLOATS = {"prev_ball_vy": OBS_TOL, "est_bounce_pos": OBS_TOL, "est_bounce_time": OBS_TOL, "est_max_height": OBS_TOL, "distance": OBS_TOL, "racket_pos": OBS_TOL,
          "racket_normal": OBS_TOL, "obs": OBS_TOL, "ball_obs": OBS_TOL, "rew": REW_TOL, "sub_rewards": REW_TOL}
_cache = {}


def golden():
    if "d" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["d"] = {k: z[k] for k in z.files}
    return _cache["d"]


def settings(name):
    d = golden()
    rt, L, hist, target, vel, early, steps, grip = [int(x) for x in d[name + "/settings"]]
    sc, w = d["scales"], d["weights"]
    st = tc.task_settings(reward_type=("reach", "return", "return_w_estimate")[rt], obs_ball_traj_length=L, use_history_ball_obs=hist, use_random_ball_target=target,
                          contact_by_velocity=vel, enable_early_termination=early, max_episode_length=int(d["max_episode_length"]), grip=("eastern", "semi_western")[grip],
                          court_min=d["court"][0], court_max=d["court"][1], reward_scales=dict(zip(("pos", "phase", "bounce_pos", "bounce_time"), sc)),
                          reward_weights={"pos": w[0], "ball_pos": w[1]}, grids=d["grids"])
    return st, steps


def _player(d, t):
    n = len(d["rb_state"])
    root_states = np.zeros((n, 13), np.float32)
    root_states[:, 0:3], root_states[:, 7:10] = d["rb_state"][:, 0, 0:3], d["script/root_vel"][t]
    return dict(rb_state=d["rb_state"], root_states=root_states, racket_state=d["racket_state"], ball_state=d["script/ball_state"][t], wrist_link=np.full(n, 22, np.int64))


def step_inputs(name, t):
    """Every array v2p_tennis_task_step reads at step t of a variant (state before the step included)."""
    d, (st, _) = golden(), settings(name)
    s = _player(d, t)
    for k in ("has_bounce", "has_bounce_now", "bounce_pos", "phase_pred", "swing_type", "swing_type_cycle"):
        s[k] = d["script/" + k][t]
    for k in ("tar_time", "tar_time_total", "tar_action", "progress", "target_bounce_pos", "bounce_in", "est_bounce_pos", "est_bounce_time", "est_max_height", "est_bounce_in",
              "distance", "prev_ball_vy", "traj_cursor", "has_racket_contact", "has_racket_contact_now"):
        s[k] = d["%s/pre/%s" % (name, k)][t]
    s["traj_out_x"], s["traj_out_y"] = d["traj_out_x"], d["traj_out_y"]
    s["ball_traj"] = d["pool"][d[name + "/pre/traj_row"][t]]
    s["ball_obs"] = d[name + "/pre/ball_obs"][t] if st["use_history"] else None
    s["vel_x_overflow"] = np.zeros(1, np.int64)
    return s


def _obs_rows(d, name, t, task_obs):
    actor = d["actor_obs"].copy()
    actor[:, 3:6], actor[:, 222:225] = d["script/root_vel"][t], d[name + "/racket_normal"]
    return np.concatenate([actor, task_obs], 1)


def step_expected(name, t):
    d, (st, _) = golden(), settings(name)
    o = {k: d["%s/post/%s" % (name, k)][t] for k in ("tar_time", "progress", "has_racket_contact", "has_racket_contact_now", "bounce_in", "est_bounce_in", "reset", "terminate",
                                                      "reset_reaction", "reset_recovery", "prev_ball_vy", "est_bounce_pos", "est_bounce_time", "est_max_height", "distance", "rew",
                                                      "sub_rewards")}
    o["vel_x_overflow"] = d[name + "/post/vel_x_overflow"][t]
    o["racket_pos"], o["racket_normal"] = d["racket_pos"], d[name + "/racket_normal"]
    o["obs"] = _obs_rows(d, name, t, d[name + "/post/task_obs"][t])
    if st["use_history"]:
        o["ball_obs"] = d[name + "/post/ball_obs"][t]
    else:
        o["traj_cursor"] = d[name + "/post/traj_cursor"][t]
    return o


def reset_obs_case(name, t):
    """`_compute_observations(ids)` after the resets that follow step t (t < steps - 1): inputs, env ids, expected rows / history."""
    d, (st, _) = golden(), settings(name)
    s = _player(d, t)
    s["target_bounce_pos"] = d[name + "/pre/target_bounce_pos"][t + 1]
    s["ball_traj"], s["traj_cursor"] = d["pool"][d[name + "/pre/traj_row"][t + 1]], d[name + "/pre/traj_cursor"][t + 1]
    s["ball_obs"] = d[name + "/reset/ball_obs_in"][t] if st["use_history"] else None
    ids = np.nonzero(d[name + "/reset/ids"][t])[0].astype(np.int64)
    want = dict(obs=_obs_rows(d, name, t, d[name + "/reset/task_obs"][t])[ids], racket_pos=d["racket_pos"][ids], racket_normal=d[name + "/racket_normal"][ids])
    if st["use_history"]:
        want["ball_obs"] = d[name + "/pre/ball_obs"][t + 1][ids]
    return s, ids, want


def close_nan(a, b, tol, what):
    """`close` refuses non-finite values: the NaN rows are compared for their NaN positions first, then for the rest."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN positions differ"
    close(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b), tol, what)


def compare(got, want, what):
    """Flags, counters and integer state exact; floats within the tolerance of their kind."""
    for k, w in want.items():
        g = np.asarray(got[k])
        if k in EXACT:
            assert np.array_equal(g.reshape(-1).astype(np.int64), np.asarray(w).reshape(-1).astype(np.int64)), "%s: %s differs at %s" % (
                what, k, np.nonzero(g.reshape(-1).astype(np.int64) != np.asarray(w).reshape(-1).astype(np.int64))[0][:8])
        else:
            close_nan(g.reshape(np.asarray(w).shape), w, FLOATS[k], "%s: %s" % (what, k))
