"""Golden data of policy inference, recorded from the reference itself: tests/golden/policies.npz.

The reference's OWN classes run on the CPU through oracle/ref_shim (imported, not modified): `ImitatorBuilder.Network.eval_actor`
(vid2player/models/im_network_builder.py:53-81), `ImitatorBuilderDual.Network.eval_actor` (models/im_network_builder_dual.py:37-45),
`V2PBuilder.Network.eval_actor`, `V2PBuilderDual.Network.eval_actor`, `RunningNorm.forward` (models/running_norm.py:31-42), and the
loaders `ImitatorPlayer.load_dual_cp` (players/im_player.py:54-91), `V2PPlayer.load_dual_cp` and `V2PPlayer.restore`
(players/v2p_player.py:17-109) on synthetic checkpoints saved to a temporary directory.  Objects are made with `__new__` and their
attributes set by hand (rl_games' A2CBuilder, which would build them, is absent here); rl_games' `RunningMeanStd` is the restatement of
oracle/ref_shim/rl_games_restated.py.  The PD targets of the low-level variants are `HumanoidSMPLIMMVAE._action_to_pd_targets`
(env/tasks/humanoid_smpl_im_mvae.py:693-709) of the clamped mu, its clamp asserted inactive.

The checkpoints - weights and statistics - come from a seed (tests/policies_fixture.py), so the file stores what the reference made of
them, not the weights: per variant the clamped and normalised network input `x` (side-major order, tests/policies_fixture
documents the variants), `mu`, the clamped action, the PD targets, and the state the loaders left (statistics, padded first layers, row
sums of the wide ones).  Every float32 result comes with max |fp32 - fp64| of the reference against itself (the dense layers re-run in
double on the same float32 input).  The generator asserts that clip_obs, the normaliser's +-5 and clip_actions each bind on some
elements and not on others where they are finite.  Only arrays are stored.  Run where the reference exists:
    python tools/gen_golden_policies.py
"""
import copy
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

from ref_shim import rl_games_restated  # noqa: E402
from ref_shim.install import REFERENCE_ROOT, _Sink, install  # noqa: E402

install()
rl_games_restated.register()
for absent in ("players.mvae_player", "env.utils.player_builder", "smpl_visualizer", "smpl_visualizer.vis_sport", "tqdm"):
    sys.modules.setdefault(absent, _Sink(absent))
sys.path.insert(0, os.path.join(REFERENCE_ROOT, "vid2player"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

torch.set_num_threads(1)

import env.tasks.humanoid_smpl_im_mvae as ref_task  # noqa: E402
import models.im_network_builder as ref_im  # noqa: E402
import models.im_network_builder_dual as ref_im_dual  # noqa: E402
import models.v2p_network_builder as ref_v2p  # noqa: E402
import models.v2p_network_builder_dual as ref_v2p_dual  # noqa: E402
import players.im_player as ref_im_player  # noqa: E402
import players.v2p_player as ref_v2p_player  # noqa: E402
from models.running_norm import RunningNorm  # noqa: E402

from tests import policies_fixture as PF  # noqa: E402

RunningMeanStd = rl_games_restated.RunningMeanStd
# (`V2PPlayer.restore` reads its file through rl_games' helper, absent here: torch.load stands in)
ref_v2p_player.torch_ext = types.SimpleNamespace(load_checkpoint=lambda path: torch.load(path, map_location="cpu"))
OUT = PF.PATH


def mlp(inp, units):
    layers, d = [], inp
    for u in units:
        layers += [nn.Linear(d, u), nn.ReLU()]
        d = u
    return nn.Sequential(*layers)


def make_network(cls, dim, act, running_obs):
    """One `*.Network` of the reference with the attributes its __init__ would set for the shipped configs; running_obs: a module or None."""
    net = cls.__new__(cls)
    nn.Module.__init__(net)
    net.use_running_obs, net.running_obs_type = running_obs is not None, "rl_game" if isinstance(running_obs, RunningMeanStd) else "ours"
    if running_obs is not None:
        net.running_obs = running_obs
    net.is_continuous, net.is_discrete, net.is_multi_discrete = True, False, False
    net.space_config = {"fixed_sigma": True, "learn_sigma": False}
    net.actor_cnn, net.critic_cnn = nn.Sequential(), nn.Sequential()
    net.actor_mlp, net.critic_mlp = mlp(dim, PF.UNITS), mlp(dim, PF.UNITS)
    net.mu, net.value = nn.Linear(PF.UNITS[-1], act), nn.Linear(PF.UNITS[-1], 1)
    net.mu_act, net.sigma_act, net.value_act = nn.Identity(), nn.Identity(), nn.Identity()
    net.sigma = nn.Parameter(torch.zeros(act), requires_grad=False)
    return net.eval()


def make_dual(cls, nets):
    net = cls.__new__(cls)
    nn.Module.__init__(net)
    net.network1, net.network2 = nets
    return net.eval()


def save_checkpoints(v, tmp):
    paths = []
    for s in range(PF.sides(v)):
        paths.append(os.path.join(tmp, "%s_%d.pth" % (v, s)))
        torch.save(PF.checkpoint_tensors(v, s), paths[-1])
    return paths


def load_variant(v, tmp):
    """(network, outer normaliser or None) of variant v, loaded by the reference's own loaders."""
    spec, (dim, act) = PF.VARIANTS[v], PF.dims(v)
    paths = save_checkpoints(v, tmp)
    if spec["kind"] == "ll":
        nets = [make_network(ref_im.ImitatorBuilder.Network, dim, act, RunningNorm(dim)) for _ in paths]
        player = ref_im_player.ImitatorPlayer.__new__(ref_im_player.ImitatorPlayer)
        nn.Module.__init__(player) if isinstance(player, nn.Module) else None  # (the stand-in base class of the absent rl_games is a Module)
        player.device, player.config, player.normalize_input = "cpu", {}, False
        if len(nets) == 2:
            net = make_dual(ref_im_dual.ImitatorBuilderDual.Network, nets)
            player.model = rl_games_restated.ModelA2CContinuousLogStd.Network(net)
            player.load_dual_cp(paths)
        else:  # (`restore`, :44-52: the file name is made of network_path, the config's name and the checkpoint's)
            net = nets[0]
            player.model = rl_games_restated.ModelA2CContinuousLogStd.Network(net)
            player.network_path, player.config = tmp, {"name": v}
            player.restore("0")
        return net, None
    kinds = spec["stats"]
    player = ref_v2p_player.V2PPlayer.__new__(ref_v2p_player.V2PPlayer)
    nn.Module.__init__(player) if isinstance(player, nn.Module) else None
    player.device = "cpu"
    if len(kinds) == 2:
        nets = [make_network(ref_v2p.V2PBuilder.Network, dim, act, RunningNorm(dim)) for _ in paths]
        net = make_dual(ref_v2p_dual.V2PBuilderDual.Network, nets)
        player.model, player.config = rl_games_restated.ModelA2CContinuousLogStd.Network(net), {}
        player.load_dual_cp(paths)
        return net, None
    inside = RunningMeanStd((dim,)) if kinds[0] == "rl_game" else None
    net = make_network(ref_v2p.V2PBuilder.Network, dim, act, inside)
    player.model = rl_games_restated.ModelA2CContinuousLogStd.Network(net)
    player.network_path, player.config = tmp, {"name": v}
    player.normalize_input = kinds[0] == "input"
    player.running_mean_std = RunningMeanStd((dim,)).eval() if player.normalize_input else None
    player.restore("0")
    return net, player.running_mean_std


def networks_of(net):
    return [net.network1, net.network2] if hasattr(net, "network1") else [net]


def binds(x, c, what):
    a = np.abs(x[np.isfinite(x)])
    assert (a >= c).any() and (a < c).any(), "%s: the clip %g binds on %d of %d elements" % (what, c, int((a >= c).sum()), a.size)


def record(v, tmp, out):
    spec, (dim, act), sides = PF.VARIANTS[v], PF.dims(v), PF.sides(v)
    net, outer = load_variant(v, tmp)
    nets = networks_of(net)
    obs = torch.from_numpy(PF.observations(v))
    clip_obs, clip_actions = spec["clip_obs"], spec["clip_actions"]
    with torch.no_grad():
        clamped = torch.clamp(obs, -clip_obs, clip_obs)  # (im_player.py:189)
        pre = outer(clamped) if outer is not None else clamped  # (`_preproc_obs`: the player's RunningMeanStd in eval mode)
        mu = net.eval_actor({"obs": pre})[0]
        # the networks' input as the reference's normalisers make it, side by side (side-major order)
        x = torch.cat([(n.running_obs(pre[s::sides]) if n.use_running_obs else pre[s::sides]) for s, n in enumerate(nets)], 0)
        # the dense layers in double on the same input
        mu64 = []
        for s, n in enumerate(nets):
            d = copy.deepcopy(n).double()
            d.use_running_obs = False
            mu64.append(d.eval_actor({"obs": x[s * (PF.N // sides):(s + 1) * (PF.N // sides)].double()})[0])
        mu64 = torch.stack(mu64, 1).reshape(PF.N, act) if sides == 2 else mu64[0]
        action = torch.clamp(mu, -clip_actions, clip_actions)  # (im_player.py:196)
    if np.isfinite(clip_obs):
        binds(obs.numpy(), clip_obs, v + " clip_obs")
    for s, n in enumerate(nets):
        kind = PF.NORM_KIND[spec["stats"][s]]
        if kind != "none":
            binds(x.numpy()[s * (PF.N // sides):(s + 1) * (PF.N // sides)], 5.0 * (1 - 1e-7), "%s side %d normaliser" % (v, s))
    if np.isfinite(clip_actions):
        binds(mu.numpy(), clip_actions, v + " clip_actions")
    out[v + "/x"], out[v + "/mu"], out[v + "/action"] = x.numpy(), mu.numpy(), action.numpy()  # (the observation is the seed's: PF.observations)
    out[v + "/mu_scatter"] = np.float64(np.abs(mu.numpy().astype(np.float64) - mu64.numpy()).max())
    assert out[v + "/mu_scatter"] > 0 and np.isfinite(mu.numpy()).all()
    # ---- the state the loaders left
    for s, n in enumerate(nets):
        p = "%s/loaded/%d/" % (v, s)
        w0 = n.actor_mlp[0].weight.detach().numpy()
        if dim <= 64:
            out[p + "actor_mlp.0.weight"] = w0
        out[p + "actor_mlp.0.weight_row_sums"] = w0.astype(np.float64).sum(1)
        out[p + "mu.bias"] = n.mu.bias.detach().numpy()
        if n.use_running_obs and isinstance(n.running_obs, RunningNorm):
            out[p + "n"], out[p + "mean"], out[p + "std"] = np.int64(n.running_obs.n), n.running_obs.mean.numpy(), n.running_obs.std.numpy()
        elif n.use_running_obs:
            out[p + "mean"], out[p + "var"] = n.running_obs.running_mean.float().numpy(), n.running_obs.running_var.float().numpy()
        if outer is not None:
            out[p + "mean"], out[p + "var"] = outer.running_mean.float().numpy(), outer.running_var.float().numpy()
    if spec["kind"] != "ll":
        return
    # ---- `_action_to_pd_targets` of the clamped action
    r = np.random.RandomState(PF.seed_of(v, 9))
    scale, offset = r.uniform(0.4, 1.0, 69).astype(np.float32), r.uniform(-0.2, 0.2, 69).astype(np.float32)
    tdof = r.uniform(-0.6, 0.6, (PF.N, 69)).astype(np.float32)
    cur = (tdof + r.uniform(-0.05, 0.05, (PF.N, 69))).astype(np.float32)
    res = {}
    for dtype in (torch.float32, torch.float64):
        o = ref_task.HumanoidSMPLIMMVAE.__new__(ref_task.HumanoidSMPLIMMVAE)
        o.cfg, o.no_scale_action = {"env": {"pd_target_base": spec["base"]}}, spec["no_scale"]
        c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        o._target_dof_pos, o._dof_pos, o._pd_action_offset, o._pd_action_scale = c(tdof), c(cur), c(offset), c(scale)
        if spec["base"] == "none":  # (the clamp is around `_dof_pos`: the object of this base sits at the offsets)
            o._dof_pos = c(np.broadcast_to(offset, (PF.N, 69)) + 0.0)
        pd = o._action_to_pd_targets(action[:, :69].to(dtype))
        assert ((pd > o._dof_pos - np.pi / 2 + 1e-3) & (pd < o._dof_pos + np.pi / 2 - 1e-3)).all(), v + ": the clamp of _action_to_pd_targets is active"
        res[dtype] = pd.numpy().copy()
    out[v + "/pd_action_scale"], out[v + "/pd_action_offset"], out[v + "/target_dof_pos"], out[v + "/dof_pos"] = scale, offset, tdof, cur
    out[v + "/pd"] = res[torch.float32]
    out[v + "/pd_scatter"] = np.float64(np.abs(res[torch.float32].astype(np.float64) - res[torch.float64]).max())


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for v in PF.VARIANTS:
            record(v, tmp, out)
            print("%-18s mu scatter %.3g" % (v, out[v + "/mu_scatter"]))
    np.savez_compressed(OUT, **{k: (x if np.ndim(x) == 0 else np.ascontiguousarray(x)) for k, x in out.items()})
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
