"""What tools/gen_golden_policies.py and the policy tests share: the variants of tests/golden/policies.npz, the synthetic checkpoints
(weights and statistics from a seed - numpy's RandomState, stable across versions - so the fixture stores results, not weights) and the
builders of the controllers the GPU tests and tools/ll_policy_bench.py close the control step on."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "policies.npz")
N, UNITS = 12, (64, 48, 32)
LL_DIM, LL_ACT, CTL_DIM, CTL_ACT, CTL_CKPT_DIM = 734, 75, 40, 35, 33
INF = math.inf
PREFIX = "a2c_network."

# kind: ll (the imitation policy, 734 -> 75, PD targets recorded) or ctl (the controller's actor, 40 -> 35).
# stats, one per network: where the checkpoint keeps its input statistics -
#   norm_n0 / norm   `running_obs.n / mean / var / std` of a RunningNorm in the model dict (n == 0 / n > 0)
#   rms              the checkpoint's `running_mean_std` (rl_games), read by load_dual_cp into the network's RunningNorm
#   rms_model        `running_obs.running_mean / running_var / count` in the model dict, read by load_dual_cp likewise
#   input            the checkpoint's `running_mean_std`, loaded into the player's own RunningMeanStd (normalize_input)
#   rl_game          `running_obs.running_mean / ...` loaded into a RunningMeanStd INSIDE the network (running_obs_type rl_game)
# ckpt_dim: columns of the checkpoint's first layer and statistics (narrower than the observation: zero-padded)
VARIANTS = {
    "ll_one_running": dict(kind="ll", stats=["norm"], clip_obs=3.0, clip_actions=0.5, base="target_pos", no_scale=False),
    "ll_one_none": dict(kind="ll", stats=["norm_n0"], clip_obs=INF, clip_actions=INF, base="current_pos", no_scale=True),
    "ll_two_dual_cp": dict(kind="ll", stats=["rms", "rms_model"], clip_obs=3.0, clip_actions=0.5, base="none", no_scale=False),
    "ll_two_mixed": dict(kind="ll", stats=["norm_n0", "norm"], clip_obs=INF, clip_actions=INF, base="target_pos", no_scale=True),
    "ctl_one_input": dict(kind="ctl", stats=["input"], ckpt_dim=[CTL_CKPT_DIM], clip_obs=INF, clip_actions=INF),
    "ctl_one_rl_game": dict(kind="ctl", stats=["rl_game"], ckpt_dim=[CTL_DIM], clip_obs=4.0, clip_actions=1.0),
    "ctl_two_dual_cp": dict(kind="ctl", stats=["rms", "rms_model"], ckpt_dim=[CTL_CKPT_DIM, CTL_DIM], clip_obs=4.0, clip_actions=1.0),
}
NORM_KIND = {"norm": "running", "norm_n0": "none", "rms": "running", "rms_model": "running", "input": "mean_var", "rl_game": "mean_var"}


def sides(v):
    return len(VARIANTS[v]["stats"])


def dims(v):
    return (LL_DIM, LL_ACT) if VARIANTS[v]["kind"] == "ll" else (CTL_DIM, CTL_ACT)


def seed_of(v, side):
    return 7000 + 10 * sorted(VARIANTS).index(v) + side


def _exact_variances(r, width, eps):
    """Variances var (exact in float32) with sqrt(var + eps) exact in float32: the root has 11 significant bits.  The reference takes
    these roots with torch's CPU sqrt, a vectorised library call that is faithful but not correctly rounded; on an exact root both agree,
    so the recorded bits do not depend on the library."""
    out = np.zeros(width, np.float64)
    todo = np.ones(width, bool)
    while todo.any():
        m, e = np.frexp(r.uniform(0.05, 1.5, int(todo.sum())))
        root = np.ldexp(np.round(m * 2048) / 2048, e).astype(np.float32)
        square = root * root  # (22 bits: exact)
        var = (square - eps).astype(np.float32)
        ok = ((var + eps).astype(np.float32) == square) & (np.sqrt(square) == root)
        idx = np.nonzero(todo)[0]
        out[idx[ok]] = var[ok]
        todo[idx[ok]] = False
    return out


def checkpoint_arrays(v, side):
    """The synthetic checkpoint of one network as numpy arrays: {"model": {...}, "running_mean_std": {...}?}.  Critic layers are there
    because the reference's loaders read them."""
    spec = VARIANTS[v]
    dim, act = dims(v)
    width = spec.get("ckpt_dim", [dim] * 2)[side]
    r = np.random.RandomState(seed_of(v, side))
    model, d = {}, width
    for i, u in enumerate(UNITS):
        for net in ("actor_mlp", "critic_mlp"):
            model["%s%s.%d.weight" % (PREFIX, net, 2 * i)] = (r.standard_normal((u, d)) / np.sqrt(d)).astype(np.float32)
            model["%s%s.%d.bias" % (PREFIX, net, 2 * i)] = (0.1 * r.standard_normal(u)).astype(np.float32)
        d = u
    model[PREFIX + "mu.weight"] = (0.3 * r.standard_normal((act, d)) / np.sqrt(d)).astype(np.float32)
    model[PREFIX + "mu.bias"] = (0.05 * r.standard_normal(act)).astype(np.float32)
    model[PREFIX + "value.weight"] = (r.standard_normal((1, d)) / np.sqrt(d)).astype(np.float32)
    model[PREFIX + "value.bias"] = np.zeros(1, np.float32)
    model[PREFIX + "sigma"] = np.full(act, -1.756, np.float32)
    mean = r.uniform(-0.5, 0.5, width)
    kind = spec["stats"][side]
    var = _exact_variances(r, width, np.float32(1e-5) if NORM_KIND[kind] == "mean_var" else np.float32(0))
    if NORM_KIND[kind] != "mean_var":
        var[3] = 0.0  # (a column that never moved: std = 0)
    ck = {"model": model}
    if kind in ("norm", "norm_n0"):
        model[PREFIX + "running_obs.n"] = np.array(0 if kind == "norm_n0" else 1000, np.int64)
        model[PREFIX + "running_obs.mean"] = mean.astype(np.float32)
        model[PREFIX + "running_obs.var"] = var.astype(np.float32)
        model[PREFIX + "running_obs.std"] = np.sqrt(var.astype(np.float32))
    elif kind in ("rms", "input"):  # (rl_games keeps float64 statistics)
        ck["running_mean_std"] = {"running_mean": mean.astype(np.float64), "running_var": var.astype(np.float64), "count": np.array(4096.0, np.float64)}
    else:
        model[PREFIX + "running_obs.running_mean"] = mean.astype(np.float64)
        model[PREFIX + "running_obs.running_var"] = var.astype(np.float64)
        model[PREFIX + "running_obs.count"] = np.array(4096.0, np.float64)
    return ck


def checkpoint_tensors(v, side):
    """The same as torch tensors: what `torch.load` of the saved file returns."""
    import torch

    conv = lambda d: {k: (conv(x) if isinstance(x, dict) else torch.from_numpy(np.array(x))) for k, x in d.items()}
    return conv(checkpoint_arrays(v, side))


def observations(v):
    """obs [N,dim] in env order, of mixed scales so that clip_obs and the normaliser's +-5 both bind on some elements and not on others
    (the generator asserts it)."""
    dim, _ = dims(v)
    r = np.random.RandomState(seed_of(v, 5))
    obs = r.standard_normal((N, dim)) * r.choice([0.3, 1.0, 3.0, 9.0], (N, dim))
    if VARIANTS[v]["clip_obs"] == INF:  # (nothing bounds what an unnormalised side's network sees: keep its mu inside the PD clamp)
        obs *= 0.15
    return obs.astype(np.float32)


_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(PATH))
    return _cache["g"]


def loaded(v):
    """(actors, norms) of variant v through the product's loaders, from the synthetic checkpoints."""
    from vid2player3d_amd import policies as P

    dim, _ = dims(v)
    actors, norms = [], []
    for s, kind in enumerate(VARIANTS[v]["stats"]):
        ck = checkpoint_tensors(v, s)
        actors.append(P.ActorMLP.from_state_dict(ck["model"], obs_dim=dim))
        norms.append(P.input_norm(ck, dim) if kind == "input" else P.network_norm(ck, dim) if kind != "rl_game" else rl_game_norm(ck, dim))
    return actors, norms


def rl_game_norm(ck, dim):
    """A RunningMeanStd INSIDE the network (running_obs_type rl_game): the model dict's `running_obs.running_mean / running_var`, eval form."""
    from vid2player3d_amd import policies as P

    m = ck["model"]
    return P.input_norm({"running_mean_std": {"running_mean": m[PREFIX + "running_obs.running_mean"], "running_var": m[PREFIX + "running_obs.running_var"]}}, dim)


# ------------------------------------------------------------------------------------------------------------------ GPU: the controllers
DEV = "cuda:0"


def _sim_cfg(n, v2p, clips=8, frames=(10, 14)):
    from tests.gpu_util import synth_tables
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import default_cfg

    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=clips, min_frames=frames[0], max_frames=frames[1]), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = v2p
    return cfg


def single_controller(n, env=None):
    """A racket + ball controller of n envs with the seeded generator and the imitation target attached (as tests/test_gpu_mvae_target.py
    builds it).  Returns (ctl, task, player, target); env: the target's cfg env (pd_target_base, no_scale_action, ...)."""
    import torch

    from tests import mvae_fixture as MF
    from tests import mvae_target_fixture as FX
    from tests import tennis_fixture as F
    from vid2player3d_amd import ball_traj, mvae
    from vid2player3d_amd import mvae_target as mt
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall
    from vid2player3d_amd.tasks import tennis_controller as tc

    torch.manual_seed(7)
    tg, g = F.golden(), FX.golden()
    gen = ball_traj.TennisBallGenerator({"num_samples": 500}, device=DEV, seed=3)
    cfg = _sim_cfg(n, {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                       "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                       "reset_reaction_nframes": 6, "ball_traj_out_x_file": tg["traj_out_x"], "ball_traj_out_y_file": tg["traj_out_y"], "add_residual_dof": "euler",
                       "add_residual_root": True, "residual_root_scale": 0.02, "fix_head_orientation": True})
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in tg["grids"]]

    ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": 300, "enableEarlyTermination": True}, "v2p": cfg["v2p"]}, params=SmallGrid)
    w, avg, std = MF.weights()
    rot = g["H/in/joint_rotmat"][0][np.arange(n) % 12]
    init = np.tile(avg, (n, 1)).astype(np.float32)
    init[:, 2] = 0.92
    init[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(n, 144)
    bind = g["H/joint_pos_bind"][0]
    player = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, n, w, avg, std, init, bind - bind[:1], True, DEV)
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": dict(env or {"no_scale_action": True})})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)
    task.reset()
    ctl.reset()
    return ctl, task, player, target


def two_player_controller(n, env=None):
    """The two-player controller (`dual_mode: different`) of n envs with the two-player generator and the target attached (as
    tests/test_gpu_mvae_dual.py builds it).  Returns (ctl, task, player, target)."""
    import torch

    from tests import mvae_dual_fixture as DX
    from tests import mvae_target_fixture as TX
    from tests import tennis_dual_fixture as F
    from vid2player3d_amd import mvae
    from vid2player3d_amd import mvae_target as mt
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall
    from vid2player3d_amd.tasks import tennis_controller_dual as td

    torch.manual_seed(19)
    d, tg = F.golden(), TX.golden()
    betas = [[0.1 * (k + 1) for k in range(10)], [-0.05 * (k + 1) for k in range(10)]]
    cfg = _sim_cfg(n, {"dual_mode": "different", "player": ["nadal", "federer"], "righthand": [False, True], "grip": ["semi_western", "eastern"], "serve_from": "near",
                       "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate", "reward_weights": {"pos": 0.5, "ball_pos": 0.5},
                       "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10, "reset_reaction_nframes": 6, "ball_traj_in_file": d["traj_in"],
                       "add_residual_dof": "euler", "vae_action_scale": 0.7, "residual_dof_scale": 0.3, "smpl_beta": betas}, frames=(60, 120))
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class InGrid:
        HEIGHT_RANGE, VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE = [tuple(r) for r in d["in_grids"]]

    ctl = td.DualTennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"]}, traj_in_params=InGrid)
    w, avg, std = DX.weights()
    rot = tg["H/in/joint_rotmat"][0][:4]
    frames = np.stack([avg[0], avg[1], avg[0], avg[1]]).astype(np.float32)
    frames[:, 2] = 0.92
    frames[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(4, 144)
    bind = np.stack([tg["H/joint_pos_bind"][0], tg["H/joint_pos_bind"][0] * np.float32(1.06)])
    player = mvae.MotionVAEPlayer(cfg["v2p"], n, w, avg, std, None, bind[0] - bind[0, :1], True, DEV, init_data_ready=[frames[0:1], frames[1:2]],
                                  init_data_serve=[frames[2:3], frames[3:4]])
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": dict(env or {"no_scale_action": True})})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)
    task.reset()
    ctl.reset(None, serve_vel_draws=np.random.default_rng(3).uniform(0, 1, (n // 2, 3)).astype(np.float32))
    return ctl, task, player, target


def random_actors(sides, obs_dim, num_actions, units=UNITS, seed=31):
    """ActorMLPs with seeded weights of a size that keeps mu moderate."""
    import torch

    from vid2player3d_amd import policies as P

    out = []
    for s in range(sides):
        r = np.random.RandomState(seed + s)
        a = P.ActorMLP(obs_dim, units, num_actions)
        with torch.no_grad():
            for p in a.parameters():
                scale = (0.3 if p is a.mu.weight else 1.0) / np.sqrt(p.shape[-1]) if p.dim() == 2 else 0.05
                p.copy_(torch.from_numpy((scale * r.standard_normal(tuple(p.shape))).astype(np.float32)))
        out.append(a)
    return out


def random_norms(sides, dim, kinds=("running", "running"), seed=41):
    from vid2player3d_amd import policies as P

    out = []
    for s in range(sides):
        r = np.random.RandomState(seed + s)
        mean, spread = r.uniform(-0.3, 0.3, dim).astype(np.float32), r.uniform(0.05, 1.5, dim).astype(np.float32)
        spread[3] = 0.0
        out.append(P.Normaliser(kinds[s], mean, spread) if kinds[s] != "none" else P.Normaliser("none"))
    return out
