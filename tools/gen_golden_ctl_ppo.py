"""tests/golden/ctl_ppo.npz: one epoch of the reference's controller agent, recorded by RUNNING THE REFERENCE'S OWN METHODS on the CPU
through oracle/ref_shim (imported, not modified), as unbound methods on a hand-made `self`:

  vid2player/agents/v2p_agent.py        V2PAgent.play_steps, _eval_critic, calc_gradients, load_pretrained, set_network_weights, set_stats_weights
  vid2player/learning/common_agent.py   CommonAgent.discount_values, bound_loss, _actor_loss, _critic_loss, prepare_dataset, _calc_advs
  vid2player/models/v2p_models.py       V2PModel.Network.forward
  vid2player/models/v2p_network_builder.py   V2PBuilder.Network (forward, eval_actor, eval_critic; built as tools/gen_golden_policies.py builds it)
  vid2player/env/tasks/physics_mvae_controller.py   PhysicsMVAEController.get_aux_losses
  vid2player/learning/amp_datasets.py   AMPDataset._get_item / _shuffle_idx_buf

What rl_games would supply and the shim lacks is stated below in a few labelled lines each.  The "environment" is the scripted one of
tests/ctl_ppo_fixture.py (6 envs, 8 steps, obs 21, actions 35, 3 sub-rewards, units 32 / 16, minibatches of 16 frames, 2 mini-epochs).
Every float32 result is stored with its fp32-fp64 scatter: the same methods run on float64 copies, max |difference| (key + "/scatter").
`Normal.sample` draws from torch's generator; the fixture stores noise = (a - mu) / sigma recomputed in float64, and mu + sigma * noise
reproduces the sampled action only to rounding: actions are compared within the scatter rule, not bit for bit.
    PYTORCH_JIT=0 python tools/gen_golden_ctl_ppo.py        -> tests/golden/ctl_ppo.npz
"""
import copy
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)
os.environ.setdefault("PYTORCH_JIT", "0")
sys.dont_write_bytecode = True

from ref_shim import rl_games_restated as RG  # noqa: E402
from ref_shim.install import REFERENCE_ROOT, _Sink, install  # noqa: E402

install()
RG.register()
for absent in ("players.mvae_player", "env.utils.player_builder", "smpl_visualizer", "smpl_visualizer.vis_sport", "tqdm"):
    sys.modules.setdefault(absent, _Sink(absent))
sys.path.insert(0, os.path.join(REFERENCE_ROOT, "vid2player"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

torch.set_num_threads(1)

import agents.v2p_agent as ref_agent  # noqa: E402
import env.tasks.physics_mvae_controller as ref_ctl  # noqa: E402
import learning.amp_datasets as ref_data  # noqa: E402
import models.v2p_models as ref_models  # noqa: E402
import models.v2p_network_builder as ref_net  # noqa: E402
from utils.common import AverageMeter  # noqa: E402

from tests import ctl_ppo_fixture as FX  # noqa: E402

Agent = ref_agent.V2PAgent
# rl_games a2c_common.swap_and_flatten01 [restated]: [T, N, ...] -> [N * T, ...], env-major
ref_agent.a2c_common = types.SimpleNamespace(swap_and_flatten01=lambda t: t.transpose(0, 1).reshape(t.shape[0] * t.shape[1], *t.shape[2:]))
ref_agent.common_agent.a2c_common = ref_agent.a2c_common


def make_network(dtype):
    """`V2PBuilder.Network` with the attributes its __init__ would set for the shipped configs (tools/gen_golden_policies.py)"""
    cls = ref_net.V2PBuilder.Network
    net = cls.__new__(cls)
    nn.Module.__init__(net)
    net.use_running_obs, net.running_obs_type = False, "ours"
    net.is_continuous, net.is_discrete, net.is_multi_discrete = True, False, False
    net.space_config = {"fixed_sigma": True, "learn_sigma": False}
    net.actor_cnn, net.critic_cnn = nn.Sequential(), nn.Sequential()
    mlp = lambda: nn.Sequential(nn.Linear(FX.OBS_DIM, FX.UNITS[0]), nn.ReLU(), nn.Linear(FX.UNITS[0], FX.UNITS[1]), nn.ReLU())
    net.actor_mlp, net.critic_mlp = mlp(), mlp()
    net.mu, net.value = nn.Linear(FX.UNITS[-1], FX.A), nn.Linear(FX.UNITS[-1], 1)
    net.mu_act, net.sigma_act, net.value_act = nn.Identity(), nn.Identity(), nn.Identity()
    net.sigma = nn.Parameter(torch.zeros(FX.A), requires_grad=False)
    model = ref_models.V2PModel.Network(net)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in FX.initial_weights().items()})
    return model.to(dtype)


class Dataset(ref_data.AMPDataset):
    """rl_games PPODataset's base [restated]: the fields AMPDataset reads, update_values_dict, __len__, __getitem__"""

    def __init__(self, batch_size, minibatch_size, perms):
        self.batch_size, self.minibatch_size, self.length = batch_size, minibatch_size, batch_size // minibatch_size
        self.special_names = ["rnn_states"]
        self.perms = iter(perms)
        self._idx_buf = torch.as_tensor(next(self.perms)).long()

    def _shuffle_idx_buf(self):  # (the recorded permutations instead of torch.randperm: the order is an input of the fixture)
        self._idx_buf[:] = torch.as_tensor(next(self.perms)).long()

    def update_values_dict(self, values_dict):
        self.values_dict = values_dict

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        return self._get_item(idx)


def run(dtype, noise=None):
    torch.manual_seed(77)
    ctl = FX.ScriptedController(torch.device("cpu"), dtype=dtype)
    s = types.SimpleNamespace()
    cfg = FX.small_params()["config"]
    s.model = make_network(dtype)
    s.running_mean_std, s.value_mean_std = RG.RunningMeanStd((FX.OBS_DIM,)), RG.RunningMeanStd((1,))
    st = FX.initial_statistics()
    s.running_mean_std.running_mean[:], s.running_mean_std.running_var[:] = torch.from_numpy(st["obs_mean"]), torch.from_numpy(st["obs_var"])
    s.running_mean_std.count.fill_(st["obs_count"])
    s.value_mean_std.running_mean[:], s.value_mean_std.running_var[:] = st["value_mean"], st["value_var"]
    if dtype == torch.float64:  # (`current_var.float()` inside the normalisers would round the float64 run to float32)
        for m in (s.running_mean_std, s.value_mean_std):
            m.forward = types.MethodType(forward64, m)
    s.normalize_input = s.normalize_value = s.normalize_advantage = True
    s.horizon_length, s.gamma, s.tau, s.e_clip = FX.T, cfg["gamma"], cfg["tau"], cfg["e_clip"]
    s.critic_coef, s.entropy_coef, s.bounds_loss_coef, s.clip_value = cfg["critic_coef"], cfg["entropy_coef"], cfg["bounds_loss_coef"], cfg["clip_value"]
    s.truncate_grads, s.grad_norm, s.last_lr = cfg["truncate_grads"], cfg["grad_norm"], cfg["learning_rate"]
    s.is_rnn = s.use_action_masks = s.has_central_value = s.multi_gpu = s.mixed_precision = False
    s.num_agents, s.batch_size = 1, FX.N * FX.T
    s.update_list = ["actions", "neglogpacs", "values", "mus", "sigmas"]
    s.tensor_list = s.update_list + ["obses", "states", "dones"]
    z = lambda *sh: torch.zeros(sh, dtype=dtype)
    s.experience_buffer = RG.ExperienceBuffer({"obses": z(FX.T, FX.N, FX.OBS_DIM), "next_obses": z(FX.T, FX.N, FX.OBS_DIM), "rewards": z(FX.T, FX.N, 1),
                                               "dones": torch.zeros((FX.T, FX.N), dtype=torch.uint8), "values": z(FX.T, FX.N, 1), "next_values": z(FX.T, FX.N, 1),
                                               "actions": z(FX.T, FX.N, FX.A), "mus": z(FX.T, FX.N, FX.A), "sigmas": z(FX.T, FX.N, FX.A), "neglogpacs": z(FX.T, FX.N)})
    s.current_rewards, s.current_lengths = z(FX.N, 1), z(FX.N)
    s.optimizer = torch.optim.Adam(s.model.parameters(), float(s.last_lr), eps=1e-08, weight_decay=0.0)
    s.scaler = torch.cuda.amp.GradScaler(enabled=False)
    s.task = types.SimpleNamespace(cfg_v2p=ctl.cfg_v2p, _num_mvae_action=32, _num_res_dof_action=3, render_vis=lambda: None)
    s.task.get_aux_losses = types.MethodType(ref_ctl.PhysicsMVAEController.get_aux_losses, s.task)
    s.algo_observer = types.SimpleNamespace(process_infos=lambda infos, ids: None, after_steps=lambda: None)
    s.dataset = Dataset(s.batch_size, FX.MINIBATCH, FX.permutations())
    meters = {"game_rewards": [], "game_lengths": []}
    s.game_rewards = types.SimpleNamespace(update=lambda v: meters["game_rewards"].append(v.clone()))   # rl_games' windowed meters [restated: what they receive]
    s.game_lengths = types.SimpleNamespace(update=lambda v: meters["game_lengths"].append(v.clone()))
    clip_obs, clip_actions = FX.CLIP_OBS, FX.CLIP_ACTIONS
    sampled = []
    # rl_games A2CBase pieces [restated]: set_eval / set_train, _preproc_obs, get_action_values, the reward shaper (scale 1), env_reset / env_step
    # through the vec env wrapper's clamps (env/tasks/vec_task.py:103, 108)
    s.set_eval = lambda: (s.model.eval(), s.running_mean_std.eval(), s.value_mean_std.eval())
    s.set_train = lambda: (s.model.train(), s.running_mean_std.train(), s.value_mean_std.train())
    s._preproc_obs = lambda obs: s.running_mean_std(obs)
    s.rewards_shaper = lambda r: r

    def get_action_values(obs):
        s.model.eval()
        with torch.no_grad():
            if noise is not None:  # the float64 run replays the float32 run's draws
                ref_models.torch.distributions.Normal.sample = lambda d, k=len(sampled): d.loc + d.scale * noise[k].to(dtype)
            res = s.model({"is_train": False, "prev_actions": None, "obs": s._preproc_obs(obs["obs"])})
            sampled.append(((res["actions"].double() - res["mus"].double()) / res["sigmas"].double()).clone())
            if s.normalize_value:
                res["values"] = s.value_mean_std(res["values"], True)
        return res

    def env_reset(ids=None):
        ctl.reset(torch.as_tensor(ids if ids is not None and len(ids) else [], dtype=torch.long))
        return {"obs": torch.clamp(ctl.obs_buf, -clip_obs, clip_obs).clone()}

    def env_step(actions):
        ctl.step(torch.clamp(actions, -clip_actions, clip_actions))
        infos = {"terminate": ctl.extras["terminate"].clone(), "sub_rewards": ctl.extras["sub_rewards"].clone(), "sub_rewards_names": "a,b,c"}
        return {"obs": torch.clamp(ctl.obs_buf, -clip_obs, clip_obs).clone()}, ctl.rew_buf.clone().unsqueeze(1), ctl.reset_buf.clone().to(torch.uint8), infos

    s.get_action_values, s.env_reset, s.env_step = get_action_values, env_reset, env_step
    for name in ("play_steps", "_eval_critic", "calc_gradients"):
        setattr(s, name, types.MethodType(getattr(Agent, name), s))
    for name in ("discount_values", "bound_loss", "_actor_loss", "_critic_loss", "prepare_dataset", "_calc_advs"):
        setattr(s, name, types.MethodType(getattr(ref_agent.common_agent.CommonAgent, name), s))
    s.train_actor_critic = lambda d: (s.calc_gradients(d), s.train_result)[1]
    sides, actor_loss = [], s._actor_loss

    def watched_actor_loss(old_neglogp, neglogp, advantage, e_clip):
        """the reference's `_actor_loss`, with the number of frames whose ratio lies below / above the clip counted on the way"""
        ratio = torch.exp(old_neglogp - neglogp).detach()
        sides.append([int((ratio < 1.0 - e_clip).sum()), int((ratio > 1.0 + e_clip).sum())])
        return actor_loss(old_neglogp, neglogp, advantage, e_clip)

    s._actor_loss = watched_actor_loss
    out = {}
    with torch.no_grad():
        batch = s.play_steps()
    for k, v in s.experience_buffer.tensor_dict.items():
        out["buffer/" + k] = v.double().numpy().reshape(FX.T, FX.N, -1).squeeze(-1) if v.dim() < 3 or v.shape[-1] == 1 else v.double().numpy()
    out["noise"] = torch.stack(sampled).numpy()
    out["returns"] = batch["returns"].double().numpy().reshape(-1)
    out["meters/game_rewards"] = torch.cat([m.reshape(-1) for m in meters["game_rewards"]]).double().numpy()
    out["meters/game_lengths"] = torch.cat([m.reshape(-1) for m in meters["game_lengths"]]).double().numpy()
    out["meters/step_rewards"] = np.asarray(s.step_rewards.avg.double().numpy()).reshape(-1)
    out["meters/step_sub_rewards"] = s.step_sub_rewards.avg.double().numpy()
    s.set_train()
    batch.pop("played_frames")
    s.prepare_dataset(batch)
    for k in ("old_values", "old_logp_actions", "advantages", "returns"):
        out["dataset/" + k] = s.dataset.values_dict[k].double().numpy().reshape(-1)
    out["dataset/value_mean_var_count"] = np.array([s.value_mean_std.running_mean.item(), s.value_mean_std.running_var.item(), s.value_mean_std.count.item()])
    step = 0
    names = [k for k, _ in s.model.named_parameters()]
    for _ in range(FX.MINI_EPOCHS):
        for i in range(len(s.dataset)):
            r = s.train_actor_critic(s.dataset[i])
            out["step%d/stats" % step] = np.array([float(r[k]) for k in ("actor_loss", "critic_loss", "b_loss", "aux_dof_res_loss", "actor_clip_frac", "kl", "entropy")])
            out["step%d/clip_sides" % step] = np.array(sides[-1], dtype=np.int64)
            for k, p in zip(names, s.model.parameters()):
                out["step%d/param/%s" % (step, k)] = p.detach().double().numpy().copy()
            step += 1
    out["final/obs_mean"], out["final/obs_var"] = s.running_mean_std.running_mean.numpy().copy(), s.running_mean_std.running_var.numpy().copy()
    out["final/obs_count"] = np.array([s.running_mean_std.count.item()])
    return out, ctl


def run_loading():
    """`V2PAgent.load_pretrained` -> `set_network_weights` / `set_stats_weights` on the synthetic checkpoints of tests/ctl_ppo_fixture.py:
    the network's state dict and both normalisers afterwards, for every case of FX.LOAD_CASES."""
    out = {}
    for case, (w_obs, w_act, discard) in FX.LOAD_CASES.items():
        ck = FX.synthetic_checkpoint(w_obs, w_act)
        # rl_games torch_ext.load_checkpoint [restated]: the dict the file holds
        ref_agent.torch_ext.load_checkpoint = lambda path, ck=ck: copy.deepcopy(ck)
        s = types.SimpleNamespace(model=make_network(torch.float32), config={"discard_pretrained_sigma": discard}, normalize_input=True, normalize_value=True,
                                  has_central_value=False, mixed_precision=False, running_mean_std=RG.RunningMeanStd((FX.OBS_DIM,)), value_mean_std=RG.RunningMeanStd((1,)))
        for name in ("load_pretrained", "set_network_weights", "set_stats_weights"):
            setattr(s, name, types.MethodType(getattr(Agent, name), s))
        s.load_pretrained(case)
        for k, v in s.model.state_dict().items():
            out["load/%s/model/%s" % (case, k)] = v.detach().numpy().copy()
        for nm, m in (("obs", s.running_mean_std), ("value", s.value_mean_std)):
            out["load/%s/%s_mean" % (case, nm)], out["load/%s/%s_var" % (case, nm)] = m.running_mean.numpy().copy(), m.running_var.numpy().copy()
            out["load/%s/%s_count" % (case, nm)] = np.array([float(m.count)])
    return out


def forward64(self, input, unnorm=False):
    """RunningMeanStd.forward without the `.float()` casts, for the float64 run"""
    if self.training:
        self.running_mean, self.running_var, self.count = self._update_mean_var_count_from_moments(
            self.running_mean, self.running_var, self.count, input.mean(self.axis), input.var(self.axis), input.size()[0])
    if unnorm:
        return torch.sqrt(self.running_var + self.epsilon) * torch.clamp(input, min=-5.0, max=5.0) + self.running_mean
    return torch.clamp((input - self.running_mean) / torch.sqrt(self.running_var + self.epsilon), min=-5.0, max=5.0)


def main():
    f32, ctl = run(torch.float32)
    f64, _ = run(torch.float64, noise=torch.from_numpy(f32["noise"]))
    # the script must hold every case the tests lean on
    dones, term = f32["buffer/dones"], ctl.term_script[:FX.T].numpy()
    assert (dones.sum(1) == 0).any() and (dones.sum(0) == 2).any() and dones[FX.T - 1].any(), "no step without a done env / env done twice / done at the last step"
    assert ((dones > 0) & (term == 0)).any() and ((dones > 0) & (term == 1)).any(), "done envs with terminate 0 and with 1"
    assert (f32["buffer/rewards"] > 0).any() and (f32["buffer/rewards"] < 0).any(), "rewards of both signs"
    assert (f32["buffer/mus"] > 1).any() and (f32["buffer/mus"] < -1).any(), "a mu beyond +-1 on each side"
    sides = np.stack([f32["step%d/clip_sides" % k] for k in range(6)])
    assert sides[1:, 0].sum() > 0 and sides[1:, 1].sum() > 0 and sides.sum(1).min() < FX.MINIBATCH, "ratios that leave the clip on EACH side after the first minibatch: %s" % sides.tolist()
    out = {}
    for k, v in f32.items():
        if k == "noise" or k.endswith("/clip_sides"):
            out[k] = v
            continue
        out[k] = v.astype(np.float32) if not k.startswith(("final/", "dataset/value_mean")) else v
        out[k + "/scatter"] = np.array(np.abs(np.asarray(v, dtype=np.float64) - f64[k]).max())
    out.update(run_loading())
    path = os.path.join(REPO, "tests", "golden", "ctl_ppo.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
