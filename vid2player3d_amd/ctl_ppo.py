"""The PPO agent of the tennis controller: `V2PAgent` (vid2player/agents/v2p_agent.py) over `PhysicsMVAEController`, single player, method
for method:

    get_action_values / _eval_critic    rl_games' A2CBase.get_action_values; agents/v2p_agent.py:211-218
    play_steps                          agents/v2p_agent.py:220-297
    prepare_dataset / _calc_advs        learning/common_agent.py:283-313, 522-536
    calc_gradients                      agents/v2p_agent.py:299-414  (losses: learning/common_agent.py:442-450, 491-520;
                                        env/tasks/physics_mvae_controller.py:461-472 `get_aux_losses`)
    train_epoch / train                 learning/common_agent.py:146-216, agents/v2p_agent.py:98-209; minibatches learning/amp_datasets.py:16-33
    load_pretrained / set_network_weights / set_stats_weights    agents/v2p_agent.py:27-96

with the network of the six single-player yamls of vid2player/cfg/controller (`ControllerNetwork` = `V2PBuilder.Network`,
models/v2p_network_builder.py, behind `V2PModel.Network`, models/v2p_models.py; `normalize_input: True` puts rl_games' `RunningMeanStd`
in FRONT of it).  It is not `ppo.PPOAgent` with other sizes - the law differs:

  * done envs are reset INSIDE the rollout (:278-280), so `values[n + 1]` and `next_values[n]` of such an env are values of two different
    observations; there is no `alive` mask; the bootstrap is masked by `terminate` alone (:251-255),
  * the input normaliser is in training mode in every minibatch (`RunningMeanStd.forward`: the batch mean and unbiased variance are
    merged into the statistics before they are applied),
  * `bound_loss` and the task's `dof_res` loss join the total, minibatches are a permutation of FRAMES.

HOW it is done here, none of it a difference in WHAT:

  * the experience buffer is [T, N, ...] device tensors written in place; what stands around the dense layers of a rollout step is three
    launches of csrc/ctl_ppo.hip and policy_io.hip: `v2p_policy_input` (clamp + eval-mode normaliser, read by actor AND critic),
    `v2p_ctl_policy_head` (sample, neglogp, the buffer's rows, the clamped action the task steps on), `v2p_ctl_rollout_record` (the
    bookkeeping behind env_step, with float64 device accumulators for what the reference's meters receive), then `v2p_value_record`,
  * the critic runs ONCE per step on all envs, on the observation BEFORE the reset: that is `next_values[n]` (times 1 - terminated) and,
    for every env that is not reset, `values[n + 1]` as well - the reference evaluates the same eval-mode critic on the same row twice.
    The reset rewrites the observation of the done envs and of every env with a reaction or recovery flag up: the input launch then
    runs over all rows again (the actor of step n + 1 reads the new rows) and, where there is such an env, the critic once more
    (over all rows: a pass over a few rows is another GEMM shape and rounds differently in the last bit), which gives `values[n + 1]`;
    a step without such an env skips the second pass.  `reuse_next_values =
    False` runs the reference's two full passes; both fill `values` / `next_values` with the same numbers (tested),
  * the list of done envs is obtained as the reference obtains it, `dones.nonzero()`; it comes back with the flags of the rows the reset can rewrite in the ONE host read per rollout step that is kept
    (`reset_mode = 'ids'`, the default).  `reset_mode = 'flags'` resets the done envs by `reset_buf` on the device instead
    (`TennisControllerTask.reset_by_flags`: one fixed sequence of launches per step, no host read, no id list); the host then does not
    know whether a row changed, so the second critic pass runs at every step but the last - the same numbers, bit for bit (tested),
  * the epoch's action noise is one `torch.randn` draw from the agent's generator (`noise_fn` for tests), GAE is `v2p_gae`,
  * the loss head of calc_gradients is one kernel, forward and backward (`v2p_ppo_loss` behind a `torch.autograd.Function`): it reads the
    epoch's dataset THROUGH the minibatch's frame indices, so only the observation rows are gathered.  `fused_loss = False` runs the
    torch statement of the same head (`ppo_loss_torch`): what the kernel is tested and timed against,
  * the statistics of an epoch come back in one read.

`policy_head_reference`, `rollout_record_reference`, `ppo_loss_reference` (with analytic gradients) are the numpy statements of the three
kernels - the checkers of the tests; the product never calls them.  There is no CPU path: a CPU controller is a RuntimeError.
Pinned to vectors recorded from the reference's own methods: tools/gen_golden_ctl_ppo.py -> tests/golden/ctl_ppo.npz, tests/test_ctl_ppo.py,
tests/test_gpu_ctl_ppo.py.

Not built (each refused by name where a config asks for it): the two-player agent (`V2PBuilderDual`, `vid2player_dual_v2`, a sigma per
side), data parallel over ranks (`multi_gpu`), mixed precision, a learned sigma, `clip_value`, a learning-rate schedule, a network with an
inner normaliser (`use_running_obs`), a fused or reduced-precision MLP, `train()`'s `_best` checkpoint and its
`_latest` save every `save_best_after` epochs, the window of past episodes behind `eps_len` and the mean reward, the observer's logging.
"""
import ctypes as C
import datetime
import math
import os
import time

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .ppo import LOG_2PI, ValueMeanStd, _mlp, _mlp_forward, policy_kl

PREFIX = "a2c_network."
NUM_MVAE_ACTION = 32      # the latent part of the controller's action (physics_mvae_controller.py `_num_mvae_action`)
OBS_EPS = 1e-5            # rl_games RunningMeanStd(epsilon=1e-05)
OBS_NORM_CLIP = 5.0
STAT_NAMES = _lib.PPO_LOSS_STATS


# ------------------------------------------------------------------------------------------------------------------ numpy statements
def _clamp_np(v, lo, hi, dt):
    """torch.clamp on arrays: compare-and-select, so that a NaN stays a NaN and an infinite bound changes nothing."""
    v = np.where(v < dt(lo), dt(lo), v)
    return np.where(v > dt(hi), dt(hi), v).astype(dt)


def _wave_rows_sum(v, dt):
    """Row sums [n] of v [n,A], A <= 128, in the order of the kernels: lane k adds columns k and k + 64, then a butterfly over the 64
    lanes (offsets 32, 16, .., 1), lane 0's value."""
    n, A = v.shape
    p = np.zeros((n, 128), dt)
    p[:, :A] = v
    lanes = (p[:, :64] + p[:, 64:]).astype(dt)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, idx ^ o]).astype(dt)
    return lanes[:, 0]


def policy_head_reference(mu, logstd, sigma, noise, clip_actions=math.inf, dt=np.float32):
    """`v2p_ctl_policy_head` on arrays: (actions, mus, sigmas, neglogp, actions_clamped)."""
    mu, noise = np.asarray(mu, dtype=dt), np.asarray(noise, dtype=dt)
    logstd, sigma = np.asarray(logstd, dtype=dt), np.asarray(sigma, dtype=dt)
    n, A = mu.shape
    with np.errstate(all="ignore"):
        a = (mu + (sigma * noise).astype(dt)).astype(dt)
        t = ((a - mu).astype(dt) / sigma).astype(dt)
        q = _wave_rows_sum((t * t).astype(dt), dt)
        ls = _wave_rows_sum(np.tile(logstd, (n, 1)), dt)
        nlp = ((dt(0.5) * q).astype(dt) + dt(0.5 * LOG_2PI * A)).astype(dt) + ls
        return a, mu.copy(), np.tile(sigma, (n, 1)), nlp.astype(dt), _clamp_np(a, -clip_actions, clip_actions, dt)


def _record_tree_sum(v):
    """Sum of v [n] (float64) in the order of `v2p_ctl_rollout_record`: thread t adds envs t, t + 256, ... in rising order, the lanes of a
    wave combine by a butterfly, the four waves add as ((w0 + w1) + w2) + w3."""
    v = np.asarray(v, dtype=np.float64)
    pad = np.zeros((-len(v)) % 256)
    rows = np.concatenate([v, pad]).reshape(-1, 256)
    p = np.zeros(256)
    for row in rows:
        p = p + row
    lanes = p.reshape(4, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    w = lanes[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def rollout_record_reference(obs, rew, reset, terminate, sub_rewards, cur_rewards, cur_lengths, acc, sub_acc, clip_obs=math.inf):
    """`v2p_ctl_rollout_record` on arrays; returns a dict of every output (the in/out arrays as they are afterwards)."""
    f = np.float32
    obs, rew = np.asarray(obs, dtype=f), np.asarray(rew, dtype=f)
    reset, terminate = np.asarray(reset, dtype=np.int64), np.asarray(terminate, dtype=np.int64)
    n = len(rew)
    S = 0 if sub_rewards is None else np.asarray(sub_rewards).reshape(n, -1).shape[1]
    done = reset != 0
    d = reset.astype(f)
    with np.errstate(all="ignore"):
        cr = (np.asarray(cur_rewards, dtype=f) + rew).astype(f)
        cl = (np.asarray(cur_lengths, dtype=f) + f(1)).astype(f)
        acc = np.array(acc, dtype=np.float64)
        acc[0] += _record_tree_sum(np.where(done, 1.0, 0.0))
        acc[1] += _record_tree_sum(np.where(done, cr.astype(np.float64), 0.0))
        acc[2] += _record_tree_sum(np.where(done, cl.astype(np.float64), 0.0))
        acc[3] += _record_tree_sum(rew.astype(np.float64))
        sub_acc = np.array(sub_acc if S else [], dtype=np.float64)
        for k in range(S):
            sub_acc[k] += _record_tree_sum(np.asarray(sub_rewards, dtype=f).reshape(n, S)[:, k].astype(np.float64))
        nd = (f(1) - d).astype(f)
        return {"next_obs_row": _clamp_np(obs, -clip_obs, clip_obs, f), "rewards_row": rew.copy(), "dones_row": d, "terminated": terminate.astype(f),
                "cur_rewards": (cr * nd).astype(f), "cur_lengths": (cl * nd).astype(f), "acc": acc, "sub_acc": sub_acc}


def ppo_loss_reference(mu, value, data, idx=None, e_clip=0.2, critic_coef=5.0, entropy_coef=0.0, bounds_loss_coef=None, dof_res_weight=0.0, c0=0, c1=0,
                       dt=np.float64):
    """`v2p_ppo_loss` on arrays, elementwise in dt, sums in dt: (grad_mu [B,A], grad_value [B], stats [8] in the order of STAT_NAMES).
    data: old_neglogp, advantages, returns [rows], actions, old_mu [rows,A], old_sigma, logstd, sigma [A].  The gradients are analytic."""
    mu, value = np.asarray(mu, dtype=dt), np.asarray(value, dtype=dt).reshape(-1)
    B, A = mu.shape
    j = np.arange(B) if idx is None else np.asarray(idx, dtype=np.int64)
    g = lambda k: np.asarray(data[k], dtype=dt)
    act, old_mu, old_nlp, adv, ret = g("actions")[j], g("old_mu")[j], g("old_neglogp")[j], g("advantages")[j], g("returns")[j]
    sigma, old_sigma, logstd = g("sigma"), g("old_sigma"), g("logstd")
    one, half, two = dt(1), dt(0.5), dt(2)
    with np.errstate(all="ignore"):
        t = ((act - mu) / sigma).astype(dt)
        nlp = (half * (t * t).sum(-1, dtype=dt) + dt(0.5 * LOG_2PI * A) + logstd.sum(dtype=dt)).astype(dt)
        ratio = np.exp(old_nlp - nlp).astype(dt)
        lo, hi = dt(1.0 - e_clip), dt(1.0 + e_clip)
        x, y = -(adv * ratio), -(adv * _clamp_np(ratio, lo, hi, dt))
        a_loss = np.where(x > y, x, y)
        gx = np.where(x > y, one, np.where(x == y, half, dt(0)))
        inside = (ratio >= lo) & (ratio <= hi)
        d_ratio = gx * -adv + np.where(inside, (one - gx) * -adv, dt(0))
        d_nlp = d_ratio * -ratio
        c_loss = (ret - value) ** 2
        grad = d_nlp[:, None] * -(t / sigma)
        b_loss = np.zeros(B, dt)
        if bounds_loss_coef is not None:
            up, dn = np.where(mu - one < 0, dt(0), mu - one), np.where(mu + one > 0, dt(0), mu + one)
            b_loss = (dn * dn + up * up).sum(-1, dtype=dt)
            grad = grad + dt(bounds_loss_coef) * (two * (up + dn))
        res = mu[:, c0:c1]
        d_loss = (res * res).sum(-1, dtype=dt)
        grad[:, c0:c1] += dt(dof_res_weight) * (two * res)
        kl = (np.log(old_sigma / sigma + dt(1e-5)) + (sigma * sigma + (old_mu - mu) ** 2) / (two * (old_sigma * old_sigma + dt(1e-5))) - half).sum(-1, dtype=dt)
        ent = (dt(0.5 + 0.5 * LOG_2PI) + np.log(sigma)).sum(dtype=dt)
        clipped = (np.abs(ratio - one) > dt(e_clip)).astype(np.float64)
        means = [np.asarray(v, dtype=np.float64).sum() / B for v in (a_loss, c_loss, b_loss, d_loss, clipped, kl)]
        total = means[0] + float(dt(critic_coef)) * means[1] - float(dt(entropy_coef)) * float(ent) + (float(dt(bounds_loss_coef)) * means[2] if bounds_loss_coef is not None else 0.0) + \
            float(dt(dof_res_weight)) * means[3]
        grad_value = dt(critic_coef) * (two * (value - ret)) / dt(B)
        return (grad / dt(B)).astype(dt), grad_value.astype(dt), np.array(means + [float(ent), total], dtype=np.float64)


def ppo_loss_torch(mu, value, data, idx=None, e_clip=0.2, critic_coef=5.0, entropy_coef=0.0, bounds_loss_coef=None, dof_res_weight=0.0, c0=0, c1=0):
    """The loss head as the reference writes it in torch (v2p_agent.py:329-362, 395-397): (loss, stats [8] tensor in the order of
    STAT_NAMES).  What `fused_loss = False` runs, and what the kernel is tested and timed against."""
    g = (lambda k: data[k]) if idx is None else (lambda k: data[k][idx])
    sigma, logstd = data["sigma"], data["logstd"]
    A = mu.shape[-1]
    action_log_probs = 0.5 * (((g("actions") - mu) / sigma) ** 2).sum(dim=-1) + 0.5 * LOG_2PI * A + logstd.sum(dim=-1)
    advantage = g("advantages")
    ratio = torch.exp(g("old_neglogp") - action_log_probs)
    surr1 = advantage * ratio
    surr2 = advantage * torch.clamp(ratio, 1.0 - e_clip, 1.0 + e_clip)
    a_loss = torch.max(-surr1, -surr2).mean()
    c_loss = ((g("returns") - value.reshape(-1)) ** 2).mean()
    if bounds_loss_coef is not None:
        b_loss = (torch.clamp_max(mu + 1.0, 0.0) ** 2 + torch.clamp_min(mu - 1.0, 0.0) ** 2).sum(dim=-1).mean()
    else:
        b_loss = torch.zeros((), dtype=mu.dtype, device=mu.device)
    entropy = (0.5 + 0.5 * LOG_2PI + torch.log(sigma)).sum(dim=-1)
    dof_res_loss = (mu[:, c0:c1] ** 2).sum(dim=-1).mean()
    loss = a_loss + critic_coef * c_loss - entropy_coef * entropy + (bounds_loss_coef or 0.0) * b_loss + dof_res_weight * dof_res_loss
    with torch.no_grad():
        clip_frac = (torch.abs(ratio - 1.0) > e_clip).float().mean().to(mu.dtype)
        kl = policy_kl(mu.detach(), sigma.expand_as(mu), g("old_mu"), data["old_sigma"].expand_as(mu)).mean()
        stats = torch.stack([a_loss.detach(), c_loss.detach(), b_loss.detach(), dof_res_loss.detach(), clip_frac, kl, entropy.detach(), loss.detach()])
    return loss, stats


# ------------------------------------------------------------------------------------------------------------------ the network
class _A2C(nn.Module):
    def __init__(self, obs_dim, units, num_actions, sigma_init):
        super().__init__()
        self.actor_mlp, self.critic_mlp = _mlp(obs_dim, units), _mlp(obs_dim, units)
        self.mu, self.value = nn.Linear(units[-1], num_actions), nn.Linear(units[-1], 1)
        self.sigma = nn.Parameter(torch.full((num_actions,), float(sigma_init)), requires_grad=False)  # fixed_sigma, backprop_sigma False


class ControllerNetwork(nn.Module):
    """`V2PBuilder.Network` (models/v2p_network_builder.py:16-95) for the shipped option set: separate `actor_mlp` / `critic_mlp` (units,
    ReLU), `mu`, `value`, a fixed `sigma` parameter at sigma_init.val.  The state-dict keys are the reference's
    (`a2c_network.actor_mlp.0.weight`, ...): checkpoints go both ways with `policies.ActorMLP` / `ControllerPolicy`.  An inner
    normaliser (`use_running_obs`) is refused: a network with both an inner and an outer normaliser is not built."""

    def __init__(self, obs_dim, num_actions, units=(1024, 1024, 512), sigma_init=-2.9, use_running_obs=False, device=None):
        super().__init__()
        if use_running_obs:
            raise NotImplementedError("ControllerNetwork: use_running_obs (a normaliser inside the network) is not built; the single-player "
                                      "configs normalise in front of it (normalize_input: True)")
        if not 1 <= int(num_actions) <= _lib.CTL_MAX_ACTIONS:
            raise ValueError("ControllerNetwork: num_actions %r is outside [1, %d]" % (num_actions, _lib.CTL_MAX_ACTIONS))
        self.obs_dim, self.num_actions, self.units = int(obs_dim), int(num_actions), tuple(int(u) for u in units)
        self.a2c_network = _A2C(self.obs_dim, self.units, self.num_actions, sigma_init)
        self.to(device)

    def actor(self, x):
        """mu of normalised rows x (inference: bias + ReLU in the GEMM's epilogue, `ppo._mlp_forward`; under autograd: the plain layers)"""
        return self.a2c_network.mu(_mlp_forward(self.a2c_network.actor_mlp, x))

    def critic(self, x):
        return self.a2c_network.value(_mlp_forward(self.a2c_network.critic_mlp, x))

    @property
    def sigma(self):
        return self.a2c_network.sigma


class ObsMeanStd:
    """rl_games' `RunningMeanStd(obs_shape)` in front of the network (`normalize_input`, `_preproc_obs`), as oracle/ref_shim states it:
    float64 statistics, count from 1, a batch enters by its float32 mean and unbiased variance (`mean`, `var`), applied as
    clamp((x - mean.float()) / sqrt(var.float() + 1e-5), +-5) - by `v2p_policy_input`, which reads the float32 copies kept here."""

    def __init__(self, dim, device):
        self.running_mean = torch.zeros(dim, dtype=torch.float64, device=device)
        self.running_var = torch.ones(dim, dtype=torch.float64, device=device)
        self.count = torch.ones((), dtype=torch.float64, device=device)
        self.mean32, self.var32 = torch.zeros(dim, device=device), torch.ones(dim, device=device)
        self.training = False

    def sync(self):
        self.mean32.copy_(self.running_mean)
        self.var32.copy_(self.running_var)

    @torch.no_grad()
    def update(self, x):
        mean, var = x.mean(0), x.var(0)  # (the reference's two calls: var_mean's one-pass mean differs from `mean` in the last bit)
        m = float(x.shape[0])
        delta = mean - self.running_mean
        tot = self.count + m
        new_mean = self.running_mean + delta * m / tot
        M2 = self.running_var * self.count + var * m + delta ** 2 * self.count * m / tot
        self.running_mean, self.running_var, self.count = new_mean, M2 / tot, tot
        self.sync()

    def state_dict(self):
        return {"running_mean": self.running_mean.clone(), "running_var": self.running_var.clone(), "count": self.count.clone()}

    def load_state_dict(self, sd):
        dev = self.running_mean.device
        self.running_mean = torch.as_tensor(sd["running_mean"], dtype=torch.float64, device=dev).reshape(self.running_mean.shape).clone()
        self.running_var = torch.as_tensor(sd["running_var"], dtype=torch.float64, device=dev).reshape(self.running_var.shape).clone()
        self.count = torch.as_tensor(sd["count"], dtype=torch.float64, device=dev).reshape(()).clone()
        self.sync()


# ------------------------------------------------------------------------------------------------------------------ the loading rules
def set_network_weights(net, weights):
    """V2PAgent.set_network_weights (v2p_agent.py:46-76) on a `ControllerNetwork`: a checkpoint whose first layers read fewer columns
    fills the first columns of zeroed `actor_mlp.0` AND `critic_mlp.0`; one with fewer actions fills the first rows of a zeroed `mu`,
    and its sigma is dropped; everything else loads by name, non-strict.  `weights` (the checkpoint's `model` dict) is consumed."""
    a = net.a2c_network
    weights = {k: torch.as_tensor(v) for k, v in weights.items()}
    net_obs, w_obs = a.actor_mlp[0].weight.shape[-1], weights[PREFIX + "actor_mlp.0.weight"].shape[-1]
    net_act, w_act = a.mu.weight.shape[0], weights[PREFIX + "mu.weight"].shape[0]
    with torch.no_grad():
        if net_obs != w_obs:
            if net_obs < w_obs:
                raise ValueError("set_network_weights: the checkpoint's first layer reads %d columns, the observation has %d" % (w_obs, net_obs))
            for mlp, key in ((a.actor_mlp, "actor_mlp.0.weight"), (a.critic_mlp, "critic_mlp.0.weight")):
                mlp[0].weight.zero_()
                mlp[0].weight[:, :w_obs] = weights.pop(PREFIX + key).to(mlp[0].weight)
        if net_act != w_act:
            if net_act < w_act:
                raise ValueError("set_network_weights: the checkpoint has %d actions, the network %d" % (w_act, net_act))
            a.mu.weight.zero_()
            a.mu.weight[:w_act, :] = weights.pop(PREFIX + "mu.weight").to(a.mu.weight)
            a.mu.bias.zero_()
            a.mu.bias[:w_act] = weights.pop(PREFIX + "mu.bias").to(a.mu.bias)
            weights.pop(PREFIX + "sigma", None)
    return net.load_state_dict(weights, strict=False)


def set_stats_weights(obs_stats, value_stats, checkpoint, normalize_input=True, normalize_value=True):
    """V2PAgent.set_stats_weights (v2p_agent.py:78-92): a narrower `running_mean_std` is written into the first columns (count taken
    over), `reward_mean_std` is loaded into the value normaliser."""
    if normalize_input:
        if "running_mean_std" not in checkpoint:
            raise ValueError("set_stats_weights: the checkpoint has no running_mean_std")
        r = checkpoint["running_mean_std"]
        dev = obs_stats.running_mean.device
        w = torch.as_tensor(r["running_mean"]).shape[0]
        d = obs_stats.running_mean.shape[0]
        if w != d:
            if d < w:
                raise ValueError("set_stats_weights: the checkpoint's statistics have %d columns, the observation %d" % (w, d))
            obs_stats.count = torch.as_tensor(r["count"], dtype=torch.float64, device=dev).reshape(()).clone()
            obs_stats.running_mean[:w] = torch.as_tensor(r["running_mean"], dtype=torch.float64, device=dev)
            obs_stats.running_var[:w] = torch.as_tensor(r["running_var"], dtype=torch.float64, device=dev)
            obs_stats.sync()
        else:
            obs_stats.load_state_dict(r)
    if normalize_value:
        r = checkpoint["reward_mean_std"]
        dev = value_stats.running_mean.device
        value_stats.running_mean = torch.as_tensor(r["running_mean"], dtype=torch.float64, device=dev).reshape(1).clone()
        value_stats.running_var = torch.as_tensor(r["running_var"], dtype=torch.float64, device=dev).reshape(1).clone()
        value_stats.count = torch.as_tensor(r["count"], dtype=torch.float64, device=dev).reshape(()).clone()


def load_pretrained(net, obs_stats, value_stats, checkpoint, discard_pretrained_sigma=False, normalize_input=True, normalize_value=True):
    """V2PAgent.load_pretrained (v2p_agent.py:27-44) on a loaded checkpoint dict: the weights and the normalisers, not the optimizer."""
    model = dict(checkpoint["model"])
    if discard_pretrained_sigma:
        model = {k: v for k, v in model.items() if "sigma" not in k}
    set_network_weights(net, model)
    set_stats_weights(obs_stats, value_stats, checkpoint, normalize_input, normalize_value)


# ------------------------------------------------------------------------------------------------------------------ the loss head
class _PpoLossFn(torch.autograd.Function):
    """`v2p_ppo_loss`: forward computes the loss statistics AND d loss / d mu, d loss / d value in one launch; backward hands them out."""

    @staticmethod
    def forward(ctx, mu, value, agent, idx):
        grad_mu, grad_value = agent._launch_loss(mu.detach(), value.detach(), idx)
        ctx.save_for_backward(grad_mu, grad_value)
        ctx.value_shape = value.shape
        return agent._loss_stats[7].float()

    @staticmethod
    def backward(ctx, g):
        grad_mu, grad_value = ctx.saved_tensors
        return grad_mu * g, (grad_value * g).view(ctx.value_shape), None, None


class FrameSampler:
    """The minibatch order of `AMPDataset` (learning/amp_datasets.py:6-33): `_idx_buf` is a permutation of the N * T frames, minibatch i
    is `_idx_buf[i m : (i + 1) m]`, and taking the last one reshuffles.  perm_fn() (tests): the next permutation instead of a draw."""

    def __init__(self, batch_size, minibatch_size, device, generator=None):
        self.batch_size, self.minibatch_size, self.device, self.generator = int(batch_size), int(minibatch_size), device, generator
        self.idx_buf = torch.randperm(self.batch_size, generator=generator).to(device)

    def get(self, i, perm_fn=None):
        start, end = i * self.minibatch_size, (i + 1) * self.minibatch_size
        idx = self.idx_buf[start:end].clone()
        if end >= self.batch_size:
            perm = perm_fn() if perm_fn else torch.randperm(self.batch_size, generator=self.generator)
            self.idx_buf[:] = torch.as_tensor(perm, dtype=torch.long).to(self.device)
        return idx


# ------------------------------------------------------------------------------------------------------------------ the agent
def config_kwargs(params):
    """The agent's keyword arguments of a yaml's `params` block (vid2player/cfg/controller/*.yaml: `config` = what rl_games' A2CBase and
    CommonAgent read, `network` = what V2PBuilder reads).  Options this agent does not build are refused by name, not ignored."""
    cfg, net = dict(params.get("config") or {}), dict(params.get("network") or {})
    refuse = lambda what: NotImplementedError("ControllerPPOAgent: %s is not built" % what)
    if net.get("name", "vid2player") != "vid2player":
        raise refuse("network.name %r (the two-player networks vid2player_dual / vid2player_dual_v2)" % net.get("name"))
    if (params.get("model") or {}).get("name", "vid2player") != "vid2player":
        raise refuse("model.name %r" % params["model"]["name"])
    if net.get("use_running_obs", False):
        raise refuse("network.use_running_obs (a normaliser inside the network)")
    if not net.get("separate", True):
        raise refuse("network.separate False (a shared trunk)")
    for k in ("cnn", "rnn"):
        if net.get(k):
            raise refuse("a network.%s section" % k)
    mlp = dict(net.get("mlp") or {})
    if mlp.get("activation", "relu") != "relu":
        raise refuse("mlp.activation %r" % mlp.get("activation"))
    if mlp.get("d2rl", False):
        raise refuse("mlp.d2rl")
    space = dict(net.get("space") or {})
    if space and "continuous" not in space:
        raise refuse("a non-continuous action space")
    cont = dict(space.get("continuous") or {})
    if not cont.get("fixed_sigma", True) or cont.get("learn_sigma", False) or cont.get("backprop_sigma", False):
        raise refuse("a learned sigma (fixed_sigma False / learn_sigma / backprop_sigma)")
    for k in ("mu_activation", "sigma_activation"):
        if cont.get(k, "None") not in ("None", None):
            raise refuse("space.continuous.%s %r" % (k, cont.get(k)))
    if (cont.get("sigma_init") or {}).get("name", "const_initializer") != "const_initializer":
        raise refuse("sigma_init.name %r" % cont["sigma_init"]["name"])
    for key in ("multi_gpu", "mixed_precision", "clip_value", "use_action_masks", "central_value_config", "dual_mode", "dual_model_cp"):
        if cfg.get(key):
            raise refuse("config.%s" % key)
    if cfg.get("lr_schedule", "constant") not in ("constant", None):
        raise refuse("config.lr_schedule %r (only constant)" % cfg.get("lr_schedule"))
    if not cfg.get("ppo", True):
        raise refuse("config.ppo False")
    if not cfg.get("normalize_input", False):
        raise refuse("config.normalize_input False (the single-player configs normalise in front of the network)")
    if float((cfg.get("reward_shaper") or {}).get("scale_value", 1)) != 1.0 or (cfg.get("reward_shaper") or {}).get("shift_value", 0):
        raise refuse("a reward_shaper other than scale 1, shift 0")
    return dict(horizon_length=int(cfg.get("horizon_length", 32)), gamma=float(cfg.get("gamma", 0.99)), tau=float(cfg.get("tau", 0.95)),
                learning_rate=float(cfg.get("learning_rate", 1e-5)), e_clip=float(cfg.get("e_clip", 0.2)), critic_coef=float(cfg.get("critic_coef", 5.0)),
                mini_epochs=int(cfg.get("mini_epochs", 3)), minibatch_size=int(cfg.get("minibatch_size", 16384)), grad_norm=float(cfg.get("grad_norm", 50.0)),
                truncate_grads=bool(cfg.get("truncate_grads", True)), entropy_coef=float(cfg.get("entropy_coef", 0.0)),
                bounds_loss_coef=None if cfg.get("bounds_loss_coef") is None else float(cfg["bounds_loss_coef"]),
                normalize_value=bool(cfg.get("normalize_value", True)), normalize_advantage=bool(cfg.get("normalize_advantage", True)),
                clip_obs=float(cfg.get("clip_observations", math.inf)), clip_actions=float(cfg.get("clip_actions_val", math.inf)),
                units=tuple(mlp.get("units", (1024, 1024, 512))), sigma_init=float((cont.get("sigma_init") or {}).get("val", -2.9)),
                discard_pretrained_sigma=bool(cfg.get("discard_pretrained_sigma", False)), seed=int(params.get("seed", 0)))


class ControllerPPOAgent:
    def __init__(self, ctl, horizon_length=32, gamma=0.99, tau=0.95, learning_rate=1e-5, e_clip=0.2, critic_coef=5.0, mini_epochs=3, minibatch_size=16384,
                 grad_norm=50.0, truncate_grads=True, entropy_coef=0.0, bounds_loss_coef=10.0, normalize_value=True, normalize_advantage=True,
                 clip_obs=math.inf, clip_actions=math.inf, units=(1024, 1024, 512), sigma_init=-2.9, discard_pretrained_sigma=False, seed=0,
                 dof_res_weight=None, reuse_next_values=True, fused_loss=True, reset_mode="ids"):
        # reset_mode 'ids' (default): the done envs are read back once per step and reset from their id list; 'flags': the controller
        # resets them by `reset_buf` on the device (`reset_by_flags`), and the rollout step has no host read
        if reset_mode not in ("ids", "flags"):
            raise ValueError("ControllerPPOAgent: reset_mode %r is neither 'ids' nor 'flags'" % (reset_mode,))
        if reset_mode == "flags" and getattr(getattr(ctl, "task", None), "racket_players", None) is not None:
            raise NotImplementedError("ControllerPPOAgent: reset_mode 'flags' over a two-player controller is not built (resetting finished pairs by mask)")
        if reset_mode == "flags" and not callable(getattr(ctl, "reset_by_flags", None)):
            raise NotImplementedError("ControllerPPOAgent: reset_mode 'flags' needs a controller with reset_by_flags (TennisControllerTask with cfg v2p.task_reset "
                                      "'device'); %s has none" % type(ctl).__name__)
        dev = torch.device(ctl.device)
        if dev.type != "cuda":
            raise RuntimeError("ControllerPPOAgent: the controller must live on a GPU (no CPU fallback)")
        if getattr(getattr(ctl, "task", None), "racket_players", None) is not None:
            raise NotImplementedError("ControllerPPOAgent: the two-player agent is not built")
        self.reset_mode = reset_mode
        if entropy_coef != 0.0:
            raise NotImplementedError("ControllerPPOAgent: entropy_coef != 0 is not built (the entropy is a constant under the fixed sigma; all configs use 0)")
        self._lib = _lib.load()
        self.ctl, self.device = ctl, dev
        self.num_actors, self.obs_dim, self.num_actions = int(ctl.num_envs), int(ctl.obs_buf.shape[1]), int(ctl.get_action_size())
        self.horizon_length, self.gamma, self.tau = int(horizon_length), float(gamma), float(tau)
        self.e_clip, self.critic_coef, self.entropy_coef, self.mini_epochs = float(e_clip), float(critic_coef), float(entropy_coef), int(mini_epochs)
        self.bounds_loss_coef = None if bounds_loss_coef is None else float(bounds_loss_coef)
        self.grad_norm, self.truncate_grads = float(grad_norm), bool(truncate_grads)
        self.normalize_value, self.normalize_advantage, self.normalize_input = bool(normalize_value), bool(normalize_advantage), True
        self.clip_obs, self.clip_actions = float(clip_obs), float(clip_actions)
        self.discard_pretrained_sigma = bool(discard_pretrained_sigma)
        self.reuse_next_values, self.fused_loss = bool(reuse_next_values), bool(fused_loss)
        if not (self.clip_obs > 0 and self.clip_actions > 0 and self.e_clip > 0):
            raise ValueError("ControllerPPOAgent: clip_obs, clip_actions and e_clip must be > 0")
        # the task's aux loss (physics_mvae_controller.py:461-472): weight cfg v2p.aux_loss_specs.dof_res over the residual-DoF means
        if dof_res_weight is None:
            dof_res_weight = (getattr(ctl, "cfg_v2p", {}).get("aux_loss_specs") or {}).get("dof_res", 0)
        self.dof_res_weight = float(dof_res_weight)
        self.res_cols = (NUM_MVAE_ACTION, NUM_MVAE_ACTION + int(getattr(ctl, "_num_res_dof_action", 0)))
        self.batch_size = self.num_actors * self.horizon_length
        self.minibatch_size = int(minibatch_size)
        if self.minibatch_size < 1 or self.batch_size % self.minibatch_size != 0:  # (rl_games A2CBase: assert batch_size % minibatch_size == 0)
            raise ValueError("ControllerPPOAgent: num_envs * horizon_length = %d is no multiple of minibatch_size %d (frames)" % (self.batch_size, self.minibatch_size))
        self.num_minibatches = self.batch_size // self.minibatch_size
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            self.model = ControllerNetwork(self.obs_dim, self.num_actions, units, sigma_init, device=dev)
        self.model.eval()
        self.last_lr = float(learning_rate)
        self.optimizer = torch.optim.Adam(self.model.parameters(), self.last_lr, eps=1e-08, weight_decay=0.0)
        self.running_mean_std = ObsMeanStd(self.obs_dim, dev)
        self.value_mean_std = ValueMeanStd(dev)
        N, T, A, D = self.num_actors, self.horizon_length, self.num_actions, self.obs_dim
        f = dict(dtype=torch.float32, device=dev)
        self.S = int(ctl._sub_rewards.shape[1]) if getattr(ctl, "_sub_rewards", None) is not None else 0
        if self.S > _lib.CTL_MAX_SUB_REWARDS:
            raise NotImplementedError("ControllerPPOAgent: %d sub-rewards (at most %d)" % (self.S, _lib.CTL_MAX_SUB_REWARDS))
        self.tensor_dict = {"obses": torch.zeros((T, N, D), **f), "next_obses": torch.zeros((T, N, D), **f), "rewards": torch.zeros((T, N), **f),
                            "dones": torch.zeros((T, N), **f), "values": torch.zeros((T, N), **f), "next_values": torch.zeros((T, N), **f),
                            "actions": torch.zeros((T, N, A), **f), "mus": torch.zeros((T, N, A), **f), "sigmas": torch.zeros((T, N, A), **f),
                            "neglogpacs": torch.zeros((T, N), **f)}
        self.current_rewards, self.current_lengths = torch.zeros(N, **f), torch.zeros(N, **f)
        self.terminated = torch.zeros(N, **f)
        self.acc, self.sub_acc = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(max(self.S, 1), dtype=torch.float64, device=dev)
        self.x = torch.zeros((N, D), **f)                   # the eval-mode normalised observation actor and critic read
        self.actions_clamped = torch.zeros((N, A), **f)     # what the task steps on
        self.sigma_exp = torch.zeros(A, **f)                # exp(logstd), made once per rollout / minibatch on the host side of the launch
        self._input = _lib.PolicyInputCfg(sides=1, clip_obs=self.clip_obs)
        nm = self._input.norm[0]
        nm.kind, nm.eps, nm.clip = _lib.NORM_KINDS["mean_var"], OBS_EPS, OBS_NORM_CLIP
        nm.mean, nm.spread = self.running_mean_std.mean32.data_ptr(), self.running_mean_std.var32.data_ptr()
        self._loss_stats = torch.zeros(8, dtype=torch.float64, device=dev)
        self._loss_partials = torch.zeros(_lib.PPO_LOSS_PARTIALS, dtype=torch.float64, device=dev)
        self.action_gen = torch.Generator(device=dev)
        self.action_gen.manual_seed(seed)
        self.idx_gen = torch.Generator(device="cpu")
        self.idx_gen.manual_seed(seed)
        self.sampler = FrameSampler(self.batch_size, self.minibatch_size, dev, self.idx_gen)
        self.perm_fn = None    # tests: perm_fn() -> the next permutation of the frames (a recorded one)
        self.noise_fn = None   # tests: noise_fn(n) -> [N, A] standard-normal draws of step n
        self._done_ids = torch.zeros(0, dtype=torch.long, device=dev)
        self._has_obs = False
        self.dataset = None
        self.epoch_num, self.frame, self.max_epochs, self.save_freq, self.config_name = 0, 0, 10000, 0, "tennis_v1"
        self.last_mean_rewards = -100500

    # ------------------------------------------------------------------ configuration
    @classmethod
    def from_config(cls, ctl, params, **overrides):
        """`params`: the `params` block of a controller yaml.  `minibatch_size` counts FRAMES and must divide num_envs * horizon_length."""
        kw = config_kwargs(params)
        cfg = dict(params.get("config") or {})
        kw.update(overrides)
        agent = cls(ctl, **kw)
        agent.max_epochs, agent.save_freq = int(cfg.get("max_epochs", 10000)), int(cfg.get("save_frequency", 0))
        agent.config_name = cfg.get("name", "tennis_v1")
        return agent

    def set_eval(self):
        self.model.eval()
        self.running_mean_std.training = False
        self.value_mean_std.eval()

    def set_train(self):
        self.model.train()
        self.running_mean_std.training = True
        self.value_mean_std.train()

    # ------------------------------------------------------------------ launches
    def _stream(self):
        return _lib.current_stream(self.device)

    def _policy_input(self, obs, x):
        """`_preproc_obs` in eval mode (and the env wrapper's clamp in front of it): one launch"""
        _lib.check(self._lib.v2p_policy_input(C.byref(self._input), obs.shape[0], self.obs_dim, _lib.ptr(obs), _lib.ptr(x), self._stream()), "v2p_policy_input")
        return x

    def _value_record(self, raw, terminated, values_row, next_values_row):
        vms = self.value_mean_std
        _lib.check(self._lib.v2p_value_record(raw.shape[0], _lib.ptr(raw), _lib.ptr(vms.running_mean) if self.normalize_value else None,
                                              _lib.ptr(vms.running_var) if self.normalize_value else None, float(vms.epsilon), _lib.ptr(terminated),
                                              _lib.ptr(values_row), _lib.ptr(next_values_row), self._stream()), "v2p_value_record")

    def _policy_head(self, mu, noise, n):
        td = self.tensor_dict
        _lib.check(self._lib.v2p_ctl_policy_head(mu.shape[0], self.num_actions, _lib.ptr(mu), _lib.ptr(self.model.sigma), _lib.ptr(self.sigma_exp), _lib.ptr(noise),
                                                 self.clip_actions, _lib.ptr(td["actions"][n]), _lib.ptr(td["mus"][n]), _lib.ptr(td["sigmas"][n]),
                                                 _lib.ptr(td["neglogpacs"][n]), _lib.ptr(self.actions_clamped), self._stream()), "v2p_ctl_policy_head")

    def _rollout_record(self, n):
        ctl, td = self.ctl, self.tensor_dict
        sub = ctl.extras["sub_rewards"] if self.S else None
        for t, dt in ((ctl.obs_buf, torch.float32), (ctl.rew_buf, torch.float32), (ctl.reset_buf, torch.int64), (ctl.extras["terminate"], torch.int64)):
            if t.dtype != dt or not t.is_contiguous():
                raise RuntimeError("ControllerPPOAgent: the controller's obs / rew buffers must be contiguous float32, its reset / terminate flags int64")
        _lib.check(self._lib.v2p_ctl_rollout_record(self.num_actors, self.obs_dim, self.S, self.clip_obs, _lib.ptr(ctl.obs_buf), _lib.ptr(ctl.rew_buf),
                                                    _lib.ptr(ctl.reset_buf), _lib.ptr(ctl.extras["terminate"]), _lib.ptr(sub), _lib.ptr(td["next_obses"][n]),
                                                    _lib.ptr(td["rewards"][n]), _lib.ptr(td["dones"][n]), _lib.ptr(self.terminated), _lib.ptr(self.current_rewards),
                                                    _lib.ptr(self.current_lengths), _lib.ptr(self.acc), _lib.ptr(self.sub_acc) if self.S else None, self._stream()),
                   "v2p_ctl_rollout_record")

    def _launch_loss(self, mu, value, idx):
        d = self.dataset
        B, A = mu.shape
        mu, value = mu.contiguous(), value.contiguous()
        grad_mu, grad_value = torch.empty_like(mu), torch.empty(B, dtype=torch.float32, device=mu.device)
        c = _lib.PpoLossCfg(num_actions=A, has_bounds_loss=int(self.bounds_loss_coef is not None), c0=self.res_cols[0], c1=self.res_cols[1],
                            dataset_rows=d["old_neglogp"].shape[0], e_clip=self.e_clip, critic_coef=self.critic_coef, entropy_coef=self.entropy_coef,
                            bounds_loss_coef=self.bounds_loss_coef or 0.0, dof_res_weight=self.dof_res_weight)
        p = lambda t: None if t is None else t.data_ptr()
        b = _lib.PpoLossBuffers(mu=p(mu), value=p(value), idx=p(idx), old_neglogp=p(d["old_neglogp"]), advantages=p(d["advantages"]), returns=p(d["returns"]),
                                actions=p(d["actions"]), old_mu=p(d["old_mu"]), old_sigma=p(d["old_sigma"]), logstd=p(d["logstd"]), sigma=p(d["sigma"]),
                                grad_mu=p(grad_mu), grad_value=p(grad_value), stats=p(self._loss_stats), partials=p(self._loss_partials))
        _lib.check(self._lib.v2p_ppo_loss(C.byref(c), B, C.byref(b), self._stream()), "v2p_ppo_loss")
        return grad_mu, grad_value

    # ------------------------------------------------------------------ the network side of a step
    def _unnorm_value(self, raw):
        return self.value_mean_std(raw, True) if self.normalize_value else raw

    @torch.no_grad()
    def _eval_critic(self, obs):
        """v2p_agent.py:211-218: the un-normalised value [n,1] of observations obs [n,obs_dim] (eval mode)"""
        x = self._policy_input(obs.contiguous(), torch.empty_like(obs))
        return self._unnorm_value(self.model.critic(x))

    @torch.no_grad()
    def get_action_values(self, obs, noise=None):
        """rl_games' A2CBase.get_action_values over V2PModel.Network.forward(is_train = False) (models/v2p_models.py:41-52) on obs
        [n,obs_dim]: ONE `v2p_policy_input` launch gives the x actor and critic both read.  The torch statement of the head (the rollout
        goes through `v2p_ctl_policy_head`)."""
        x = self._policy_input(obs.contiguous(), torch.empty_like(obs))
        mu = self.model.actor(x)
        logstd = self.model.sigma
        sigma = torch.exp(logstd)
        if noise is None:
            noise = torch.randn(mu.shape, device=mu.device, generator=self.action_gen)
        actions = mu + sigma * noise
        nlp = 0.5 * (((actions - mu) / sigma) ** 2).sum(dim=-1) + 0.5 * LOG_2PI * mu.shape[-1] + logstd.sum(dim=-1)
        return {"actions": actions, "mus": mu, "sigmas": sigma.expand_as(mu), "neglogpacs": nlp, "values": self._unnorm_value(self.model.critic(x))}

    # ------------------------------------------------------------------ rollout (v2p_agent.py:220-297)
    def _env_reset(self, ids):
        """`env_reset(done_indices)`: the task resets those envs (and serves its own reaction / recovery flags); the observation the agent
        sees is the wrapper's clamp of `obs_buf`"""
        self.ctl.reset(ids)

    def _reset_lists(self, dones_row):
        """(done_ids, changed_ids) in ONE host read: the envs to reset (`dones.nonzero()`, :259) and the envs whose observation the
        reset can rewrite - the done ones and those whose `_reset_reaction_buf` / `_reset_recovery_buf` is up, read BEFORE the reset (it
        clears them).  A controller without these flags rewrites the done envs' rows only."""
        done = dones_row != 0
        changed = done
        for name in ("_reset_reaction_buf", "_reset_recovery_buf"):
            flag = getattr(self.ctl, name, None)
            if flag is not None:
                changed = changed | (flag != 0)
        host = torch.stack([done, changed]).cpu().numpy()  # (one device-to-host copy of 2 N bytes)
        ids = lambda m: torch.from_numpy(np.flatnonzero(m)).to(self.device)
        return ids(host[0]), ids(host[1])

    @torch.no_grad()
    def play_steps(self):
        """The rollout, straight into the [T, N, ...] buffer.  Order per step, the reference's: env_reset(done) -> obses[n] -> actor ->
        head -> ctl.step -> record -> critic -> next_values[n].  The critic pass on the observation after step n (before the reset) is
        `next_values[n]` and, for the envs whose observation the reset leaves alone, `values[n + 1]`.  The reset rewrites the observation
        of the done envs AND of every env whose reaction or recovery flag is up (`_reset_envs`, physics_mvae_controller.py:173-199: a
        new ball, a new target): after it the input launch runs over all rows again, so the actor of step n + 1 reads what `obses[n + 1]`
        holds, and where any row can have changed (`_reset_lists`) the critic runs once more over all rows for `values[n + 1]`; where none
        has, the second pass is skipped.  This equals the reference's two full passes: the critic is in eval mode in both, a row's value
        depends on that row alone, and without a changed row every row is the same row (tested bit for bit against `reuse_next_values =
        False`, on a scripted env whose reset rewrites non-done rows and on the racket + ball controller over steps in which reaction
        flags fire).  The second pass is NOT cut down to the changed rows: another GEMM shape rounds a row differently in the last bit."""
        self.set_eval()
        td, T, N, A = self.tensor_dict, self.horizon_length, self.num_actors, self.num_actions
        ctl, c = self.ctl, self.clip_obs
        self.running_mean_std.sync()
        torch.exp(self.model.sigma, out=self.sigma_exp)
        self.acc.zero_()
        self.sub_acc.zero_()
        noise_all = None if self.noise_fn else torch.randn((T, N, A), device=self.device, generator=self.action_gen)
        no_ids = self._done_ids[:0]
        self._env_reset(no_ids)  # (:229, `done_indices = []`)
        torch.clamp(ctl.obs_buf, -c, c, out=td["obses"][0])
        self._policy_input(td["obses"][0], self.x)
        if self.reuse_next_values:
            self._value_record(self.model.critic(self.x), None, td["values"][0], None)
        for n in range(T):
            if not self.reuse_next_values:
                self._value_record(self.model.critic(self.x), None, td["values"][n], None)
            mu = self.model.actor(self.x)
            noise = (self.noise_fn(n) if self.noise_fn else noise_all[n]).contiguous()
            self._policy_head(mu, noise, n)
            ctl.step(self.actions_clamped)
            self._rollout_record(n)
            # the critic on the observation after the step, before the reset: next_values[n]; values[n + 1] where no reset follows
            self._policy_input(td["next_obses"][n], self.x)
            last = n + 1 == T
            self._value_record(self.model.critic(self.x), self.terminated, None if last or not self.reuse_next_values else td["values"][n + 1], td["next_values"][n])
            if self.reset_mode == "flags":
                ctl.reset_by_flags()  # (:280, by `reset_buf` on the device: no host read, one fixed sequence of launches)
                changed = True  # (the host does not know whether a row changed: the second critic pass always runs, the same numbers)
            else:
                done_ids, changed_ids = self._reset_lists(td["dones"][n])  # the ONE host read of the step (:259)
                self._env_reset(done_ids)  # (:280)
                changed = changed_ids.numel() > 0
            if last:
                break
            torch.clamp(ctl.obs_buf, -c, c, out=td["obses"][n + 1])
            # the reset rewrites observations: the actor of step n + 1 reads the new rows (one launch over all rows) ...
            self._policy_input(td["obses"][n + 1], self.x)
            if self.reuse_next_values and changed:
                # ... and where the reset rewrote any row the critic runs again, over ALL rows: a pass over the changed rows alone is another
                # GEMM shape, which rounds the same row differently in the last bit (measured: 113 of 1024 values at 64 envs)
                self._value_record(self.model.critic(self.x), None, td["values"][n + 1], None)
        adv = torch.empty((T, N), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.v2p_gae(T, N, _lib.ptr(td["dones"]), _lib.ptr(td["values"]), _lib.ptr(td["rewards"]), _lib.ptr(td["next_values"]), self.gamma, self.tau,
                                     _lib.ptr(adv), self._stream()), "v2p_gae")
        batch = {k: td[k].transpose(0, 1).reshape((N * T,) + tuple(td[k].shape[2:])) for k in ("obses", "dones", "values", "actions", "neglogpacs", "mus", "sigmas")}
        batch["returns"] = (adv + td["values"]).transpose(0, 1).reshape(N * T)  # swap_and_flatten01
        batch["played_frames"] = self.batch_size
        return batch

    # ------------------------------------------------------------------ update
    def _calc_advs(self, batch):
        """learning/common_agent.py:522-536: over the whole batch, torch's default (unbiased) std"""
        adv = batch["returns"] - batch["values"]
        if self.normalize_advantage:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        return adv

    @torch.no_grad()
    def prepare_dataset(self, batch):
        """learning/common_agent.py:283-313: advantages from the un-normalised values; then the value normaliser, in training mode,
        takes in and normalises the values and then the returns.  The arrays are [N * T, ...] in env-major order (swap_and_flatten01)."""
        values, returns = batch["values"], batch["returns"]
        advantages = self._calc_advs(batch)
        if self.normalize_value:
            values = self.value_mean_std(values.reshape(-1, 1)).reshape(-1)
            returns = self.value_mean_std(returns.reshape(-1, 1)).reshape(-1)
        c = lambda t: t.contiguous()
        self.dataset = {"old_values": c(values), "old_neglogp": c(batch["neglogpacs"]), "advantages": c(advantages), "returns": c(returns),
                        "actions": c(batch["actions"]), "obs": c(batch["obses"]), "old_mu": c(batch["mus"]), "old_sigma": c(batch["sigmas"][0]),
                        "logstd": self.model.sigma.detach(), "sigma": self.sigma_exp}
        return self.dataset

    @property
    def _idx_buf(self):
        return self.sampler.idx_buf

    def _get_item(self, i):
        """the frame indices of minibatch i: the loss head reads the dataset through them (`FrameSampler`)"""
        return self.sampler.get(i, self.perm_fn)

    def _loss_kwargs(self):
        return dict(e_clip=self.e_clip, critic_coef=self.critic_coef, entropy_coef=self.entropy_coef, bounds_loss_coef=self.bounds_loss_coef,
                    dof_res_weight=self.dof_res_weight, c0=self.res_cols[0], c1=self.res_cols[1])

    def calc_gradients(self, idx):
        """v2p_agent.py:299-414 on the minibatch of frames idx.  `running_mean_std` in TRAINING mode: the minibatch's observations enter
        the statistics (torch's mean / var) before they are applied (`v2p_policy_input`); the layers under autograd; the loss head
        (`v2p_ppo_loss`, or its torch statement with fused_loss off); clip_grad_norm_; Adam.  Returns the 8 statistics (a device tensor)."""
        self.set_train()
        obs = self.dataset["obs"].index_select(0, idx)
        self.running_mean_std.update(obs)
        x = self._policy_input(obs, torch.empty_like(obs))
        torch.exp(self.model.sigma, out=self.sigma_exp)
        mu, value = self.model.actor(x), self.model.critic(x)
        if self.fused_loss:
            loss = _PpoLossFn.apply(mu, value, self, idx)
            stats = self._loss_stats.clone()
        else:
            loss, stats = ppo_loss_torch(mu, value, self.dataset, idx, **self._loss_kwargs())
            stats = stats.double()
        params = [p for p in self.model.parameters() if p.requires_grad]
        for p in self.model.parameters():
            p.grad = None
        loss.backward()
        if self.truncate_grads:
            nn.utils.clip_grad_norm_(params, self.grad_norm)
        self.optimizer.step()
        self.train_result = stats
        return stats

    def train_epoch(self):
        """learning/common_agent.py:146-216; the statistics of the epoch come back in ONE read."""
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        batch = self.play_steps()
        torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        self.set_train()
        frames = batch.pop("played_frames")
        self.prepare_dataset(batch)
        infos = []
        for _ in range(self.mini_epochs):
            for i in range(self.num_minibatches):
                infos.append(self.calc_gradients(self._get_item(i)))
        torch.cuda.synchronize(self.device)
        t2 = time.perf_counter()
        host = torch.cat([self.acc, self.sub_acc[:self.S], torch.stack(infos).mean(0)]).tolist()  # the ONE read-back
        acc, sub, info = host[:4], host[4:4 + self.S], host[4 + self.S:]
        self.epoch_num += 1
        self.frame += frames
        steps = float(self.batch_size)
        r = {"play_time": t1 - t0, "update_time": t2 - t1, "total_time": t2 - t0, "frames": frames, "fps_step": frames / (t1 - t0), "fps_total": frames / (t2 - t0),
             "episodes": acc[0], "mean_rewards": acc[1] / max(acc[0], 1.0), "mean_lengths": acc[2] / max(acc[0], 1.0) if acc[0] > 0 else 0.0,
             "step_rewards": acc[3] / steps, "step_sub_rewards": [s / steps for s in sub]}
        r.update({k: v for k, v in zip(STAT_NAMES, info)})
        return r

    def format_epoch_line(self, r, cfg_name=""):
        """the reference's per-epoch line (v2p_agent.py:146-150)"""
        eta = str(datetime.timedelta(seconds=round(r["total_time"] * (self.max_epochs - self.epoch_num - 1))))
        subs = ("[" + ",".join("%.4f" % s for s in r["step_sub_rewards"]) + "]") if self.S else ""
        return "{}\tT_play {:.2f}\tT_update {:.2f}\tETA {}\tstep_rewards {:.4f} {}\teps_len {:.2f}\tfps step {}\tfps total {}\t{}".format(
            self.epoch_num, r["play_time"], r["update_time"], eta, r["step_rewards"], subs, r["mean_lengths"], int(r["frames"] // r["play_time"]),
            int(r["frames"] // r["total_time"]), cfg_name)

    def train(self, max_epochs=None, log=print, network_path=None, cfg_name=""):
        """V2PAgent.train (v2p_agent.py:98-209): epochs of train_epoch with the reference's line; checkpoints `<name>_latest` /
        `<name>_epoch%05d` every save_frequency epochs and at the end.  Not the reference's: its mean episode length is over a window of
        past episodes (here: the episodes that ended in the epoch); it also saves `_latest` every `save_best_after` epochs and a `_best`
        checkpoint when the windowed mean reward rises by more than 1 (:192-202; neither is written here); its ETA multiplies the last
        epoch's time by `max_epochs - epoch_num - 1` with ITS epoch counter, which `update_epoch` has already advanced - here the same
        product with this agent's counter after the epoch; no tensorboard / observer logging."""
        last = self.max_epochs if max_epochs is None else self.epoch_num + int(max_epochs)
        r = None
        while self.epoch_num < last:
            if hasattr(self.ctl, "pre_epoch"):
                self.ctl.pre_epoch(self.epoch_num)  # (:119-120)
            r = self.train_epoch()
            if r["episodes"] > 0:
                self.last_mean_rewards = r["mean_rewards"]
            if log:
                log(self.format_epoch_line(r, cfg_name))
            if network_path and self.save_freq > 0 and self.epoch_num % self.save_freq == 0:
                self.save(os.path.join(network_path, "%s_epoch%05d" % (self.config_name, self.epoch_num)))
        if network_path:
            self.save(os.path.join(network_path, "%s_latest" % self.config_name))
        return r

    # ------------------------------------------------------------------ checkpoints
    def get_full_state_weights(self):
        """rl_games A2CBase.get_full_state_weights: model (the reference's key names), running_mean_std, reward_mean_std, optimizer, epoch, frame"""
        v = self.value_mean_std
        return {"model": {k: t.detach().clone() for k, t in self.model.state_dict().items()}, "running_mean_std": self.running_mean_std.state_dict(),
                "reward_mean_std": {"running_mean": v.running_mean.clone(), "running_var": v.running_var.clone(), "count": v.count.clone()},
                "optimizer": self.optimizer.state_dict(), "epoch": self.epoch_num, "frame": self.frame, "last_mean_rewards": self.last_mean_rewards}

    def set_full_state_weights(self, weights):
        self.model.load_state_dict({k: torch.as_tensor(v) for k, v in weights["model"].items()}, strict=True)
        set_stats_weights(self.running_mean_std, self.value_mean_std, weights, True, self.normalize_value)
        self.optimizer.load_state_dict(weights["optimizer"])
        self.epoch_num, self.frame = int(weights.get("epoch", 0)), int(weights.get("frame", 0))
        self.last_mean_rewards = weights.get("last_mean_rewards", -100500)

    def save(self, fn):
        torch.save(self.get_full_state_weights(), fn + ".pth")
        return fn + ".pth"

    def restore(self, path):
        self.set_full_state_weights(torch.load(path, map_location=self.device, weights_only=False))

    def load_pretrained(self, checkpoint):
        """v2p_agent.py:27-44; checkpoint: a path or the loaded dict"""
        if isinstance(checkpoint, (str, os.PathLike)):
            checkpoint = torch.load(checkpoint, map_location=self.device, weights_only=False)
        load_pretrained(self.model, self.running_mean_std, self.value_mean_std, checkpoint, self.discard_pretrained_sigma, True, self.normalize_value)

    def set_network_weights(self, weights):
        return set_network_weights(self.model, dict(weights))

    def set_stats_weights(self, checkpoint):
        set_stats_weights(self.running_mean_std, self.value_mean_std, checkpoint, True, self.normalize_value)

    def policy(self):
        """A `policies.ControllerPolicy` that SHARES the trained weights (the actor's parameters are the network's) and carries the current
        input statistics: the trained controller plays through the existing path.  Make a new one after further training."""
        from . import policies

        a = self.model.a2c_network
        actor = policies.ActorMLP(self.obs_dim, self.model.units, self.num_actions)
        actor.actor_mlp, actor.mu = a.actor_mlp, a.mu
        rms = self.running_mean_std
        norm = policies.Normaliser("mean_var", rms.running_mean.float(), rms.running_var.float(), eps=OBS_EPS, clip=OBS_NORM_CLIP)
        return policies.ControllerPolicy(self.ctl, actor, norm, self.clip_obs, self.clip_actions)
