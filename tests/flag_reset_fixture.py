"""What the tests of the controller's reset by flags share: a single-player racket + ball controller built like
`policies_fixture.single_controller` - the seeded generator and the imitation target attached - but over a `TennisBallGeneratorOffline`
with a small synthetic pool (shaped like `make_pool` of tests/test_gpu_tennis_reset.py), with cfg v2p `task_reset: 'device'` and
`episodeLength: 5`: `ctl.progress_buf = arange(n) % 5` then makes different envs done at different steps, deterministically.  And the
flag patterns of the kernel-level tests."""
import numpy as np

DEV = "cuda:0"
SEED = 11
POOL_ROWS, POOL_FRAMES = 64, 100
EPISODE_LENGTH = 5


def make_pool(rows=POOL_ROWS, frames=POOL_FRAMES, seed=1):
    """rows [pos3 vel3 vspin1 traj 3 x frames] sorted by launch x over [-4, 4], as the reference's pool files are"""
    rng = np.random.default_rng(seed + rows)
    pool = rng.normal(0, 1, (rows, 7 + 3 * frames)).astype(np.float32)
    pool[:, 0] = np.sort(rng.uniform(-4, 4, rows))
    pool[:, 1], pool[:, 2] = rng.uniform(12, 13, rows), rng.uniform(1, 1.5, rows)
    pool[:, 3:6] = rng.normal(0, 1, (rows, 3)) * (3, 3, 2) + (0, -25, 4)
    pool[:, 6] = rng.uniform(5, 10, rows)
    return pool


def root_xy_table(n, seed=5):
    """a start per env near the baseline's centre: the table both reset paths are given, so that they can be compared bit for bit"""
    rng = np.random.default_rng(seed)
    return ((rng.uniform(0, 1, (n, 2)) - 0.5) * (2.0, 1.5) + (0.0, -13.0)).astype(np.float32)


def flag_patterns(n):
    """{name: flags [n] int64}: none, all, alternating, only the last env, exactly one env of an 8-env workgroup (and of a 4-env one),
    exactly one half of one wave (the target's kernel gives 32 lanes to an env: one env of a pair), the values 2 and -1."""
    p = {"none": np.zeros(n, np.int64), "all": np.ones(n, np.int64), "alternating": (np.arange(n) % 2 == 0).astype(np.int64), "last": np.zeros(n, np.int64)}
    p["last"][n - 1] = 1
    one = np.zeros(n, np.int64)
    one[np.arange(min(3, n - 1), n, 8)] = 1       # one env of every 8-env workgroup (env 3 of it, or the batch's last)
    p["one_of_a_workgroup"] = one
    half = np.zeros(n, np.int64)
    half[min(1, n - 1)] = 1                        # the upper half of the first wave alone
    if n > 10:
        half[10] = 1                               # the lower half of a wave in the second workgroup alone
    p["half_a_wave"] = half
    values = np.zeros(n, np.int64)
    values[0::3], values[1::3] = 2, -1
    p["values_2_and_minus_1"] = values
    return p


def controller(n, env=None, episode_length=EPISODE_LENGTH):
    """Returns (ctl, task, player, target, gen).  episode_length: the tools measure at another share of done envs per step."""
    import torch

    from tests import mvae_fixture as MF
    from tests import mvae_target_fixture as FX
    from tests import policies_fixture as PF
    from tests import tennis_fixture as F
    from vid2player3d_amd import ball_traj, mvae
    from vid2player3d_amd import mvae_target as mt
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall
    from vid2player3d_amd.tasks import tennis_controller as tc

    torch.manual_seed(7)
    tg, g = F.golden(), FX.golden()
    gen = ball_traj.TennisBallGeneratorOffline(make_pool(), sample_random=True, device=DEV, seed=3)
    cfg = PF._sim_cfg(n, {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                          "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                          "reset_reaction_nframes": 6, "ball_traj_out_x_file": tg["traj_out_x"], "ball_traj_out_y_file": tg["traj_out_y"], "add_residual_dof": "euler",
                          "add_residual_root": True, "residual_root_scale": 0.02, "fix_head_orientation": True, "task_reset": "device"})
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in tg["grids"]]

    ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": int(episode_length), "enableEarlyTermination": True}, "v2p": cfg["v2p"]}, params=SmallGrid, seed=SEED)
    w, avg, std = MF.weights()
    rot = g["H/in/joint_rotmat"][0][np.arange(n) % 12]
    init = np.tile(avg, (n, 1)).astype(np.float32)
    init[:, 2] = 0.92
    init[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(n, 144)
    bind = g["H/joint_pos_bind"][0]
    player = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler", "seed": SEED}, n, w, avg, std, init, bind - bind[:1], True, DEV)
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": dict(env or {"no_scale_action": True})})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)
    ctl._reset_root_xy = torch.as_tensor(root_xy_table(n), device=DEV).contiguous()
    task.reset()
    ctl.reset()
    return ctl, task, player, target, gen
