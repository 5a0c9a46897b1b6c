"""What the tests of the controller's PPO agent share: the sizes, a scripted "environment" made from a seed, seeded inputs for the three
kernels, the settings copied from the `params` blocks of the reference's controller yamls (vid2player/cfg/controller/*.yaml), synthetic
checkpoints, and the torch statement of `V2PAgent.play_steps` (agents/v2p_agent.py:220-297) the agent's rollout is compared with."""
import copy
import math
import os

import numpy as np
import torch

N, T, OBS_DIM, A, S = 6, 8, 21, 35, 3
UNITS, MINIBATCH, MINI_EPOCHS = (32, 16), 16, 2
INF = math.inf
CLIP_OBS, CLIP_ACTIONS = 3.0, 1.5   # the env wrapper's clamps in the fixture's runs
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "ctl_ppo.npz")

# the keys of `params` the agent reads, as the six single-player yamls hold them (federer_train_stage_1/2/3, federer, nadal, djokovic)
_NETWORK = {"name": "vid2player", "separate": True,
            "space": {"continuous": {"mu_activation": "None", "sigma_activation": "None", "mu_init": {"name": "default"},
                                     "sigma_init": {"name": "const_initializer", "val": -2.9}, "fixed_sigma": True}},
            "mlp": {"units": [1024, 1024, 512], "activation": "relu", "d2rl": False, "initializer": {"name": "default"}, "regularizer": {"name": "None"}}}
_CONFIG = {"name": "tennis_v1", "env_name": "rlgpu", "multi_gpu": False, "ppo": True, "mixed_precision": False, "normalize_input": True, "normalize_value": True,
           "reward_shaper": {"scale_value": 1}, "normalize_advantage": True, "gamma": 0.99, "tau": 0.95, "learning_rate": 1e-5, "lr_schedule": "constant",
           "score_to_win": 20000, "max_epochs": 1000, "save_best_after": 50, "save_frequency": 100, "print_stats": True, "entropy_coef": 0.0, "truncate_grads": True,
           "grad_norm": 50.0, "e_clip": 0.2, "horizon_length": 32, "minibatch_size": 16384, "mini_epochs": 3, "critic_coef": 5, "clip_value": False, "seq_len": 4,
           "bounds_loss_coef": 10, "clip_actions_val": 5.0}


def _params(sigma=-2.9, lr=1e-5, horizon=32, **config):
    p = {"seed": 10, "algo": {"name": "vid2player"}, "model": {"name": "vid2player"}, "network": copy.deepcopy(_NETWORK), "load_checkpoint": False,
         "config": dict(copy.deepcopy(_CONFIG), learning_rate=lr, horizon_length=horizon, **config)}
    p["network"]["space"]["continuous"]["sigma_init"]["val"] = sigma
    return p


YAML_PARAMS = {
    "federer_train_stage_1": _params(-0.69, 1e-4, 64),
    "federer_train_stage_2": _params(-0.69, 2e-5, 32, discard_pretrained_sigma=True),
    "federer_train_stage_3": _params(-2.9, 1e-5, 32, discard_pretrained_sigma=True),
    "federer": _params(), "nadal": _params(), "djokovic": _params(),
}
# the two-player yamls (nadal_federer, federer_djokovic): refused
DUAL_PARAMS = _params(lr=2e-5, normalize_input=False)
DUAL_PARAMS["network"].update({"name": "vid2player_dual", "use_running_obs": True})


def small_params():
    """the fixture's agent: the yaml's keys at the sizes of the table above"""
    p = _params(-0.69, 1e-4, T, minibatch_size=MINIBATCH, mini_epochs=MINI_EPOCHS)
    p["network"]["mlp"]["units"] = list(UNITS)
    return p


def golden():
    with np.load(PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def initial_weights(seed=31):
    """The network's state dict (the reference's key names) from a seed; `mu` large enough for means beyond +-1."""
    r = np.random.RandomState(seed)
    out, shapes = {}, []
    for part in ("actor_mlp", "critic_mlp"):
        d = OBS_DIM
        for k, u in enumerate(UNITS):
            shapes += [("a2c_network.%s.%d.weight" % (part, 2 * k), (u, d)), ("a2c_network.%s.%d.bias" % (part, 2 * k), (u,))]
            d = u
    shapes += [("a2c_network.mu.weight", (A, UNITS[-1])), ("a2c_network.mu.bias", (A,)), ("a2c_network.value.weight", (1, UNITS[-1])), ("a2c_network.value.bias", (1,))]
    for name, shp in shapes:
        scale = (1.5 if name == "a2c_network.mu.weight" else 1.0) / np.sqrt(shp[-1]) if len(shp) == 2 else 0.05
        out[name] = (scale * r.standard_normal(shp)).astype(np.float32)
    out["a2c_network.sigma"] = np.full(A, -0.69, np.float32)
    return out


def initial_statistics(seed=9):
    r = np.random.RandomState(seed)
    return {"obs_mean": r.uniform(-0.3, 0.3, OBS_DIM), "obs_var": r.uniform(0.5, 2.0, OBS_DIM), "obs_count": 50.0, "value_mean": 0.3, "value_var": 1.7}


def permutations(seed=13, count=8):
    """the recorded minibatch permutations: the first is AMPDataset's initial `_idx_buf`, the next ones its reshuffles"""
    r = np.random.RandomState(seed)
    return [r.permutation(N * T) for _ in range(count)]


# ------------------------------------------------------------------------------------------------------------------ kernel inputs
def head_case(n, A, seed, clip):
    r = np.random.RandomState(seed)
    mu = (r.standard_normal((n, A)) * 2).astype(np.float32)
    logstd = r.uniform(-3.0, 0.0, A).astype(np.float32)
    sigma = np.exp(logstd).astype(np.float32)
    noise = r.standard_normal((n, A)).astype(np.float32)
    flat_mu, flat_nz = mu.reshape(-1), noise.reshape(-1)
    for k, val in enumerate([np.nan, np.inf, -np.inf]):
        flat_mu[(3 + 11 * k) % flat_mu.size] = val
    if clip != INF:  # actions exactly on the clip: noise 0, mu = +-clip
        flat_nz[5 % flat_nz.size] = 0.0
        flat_mu[5 % flat_mu.size] = clip
        flat_nz[7 % flat_nz.size] = 0.0
        flat_mu[7 % flat_mu.size] = -clip
    return mu, logstd, sigma, noise


def record_case(n, obs_dim, S, flags, seed):
    r = np.random.RandomState(seed)
    obs = (r.standard_normal((n, obs_dim)) * 3).astype(np.float32)
    obs.reshape(-1)[0] = np.nan
    rew = r.standard_normal(n).astype(np.float32)
    reset = {"all": np.ones(n), "none": np.zeros(n), "mixed": (r.uniform(size=n) < 0.4)}[flags].astype(np.int64)
    if flags == "mixed" and n > 1:
        reset[0], reset[-1] = 1, 0
    terminate = (reset * (r.uniform(size=n) < 0.5)).astype(np.int64)
    sub = r.uniform(0, 1, (n, S)).astype(np.float32)
    cur_r, cur_l = (r.standard_normal(n) * 5).astype(np.float32), r.randint(0, 40, n).astype(np.float32)
    acc, sub_acc = r.uniform(0, 100, 4), r.uniform(0, 100, S)
    return obs, rew, reset, terminate, sub, cur_r, cur_l, acc, sub_acc


def loss_case(B, A, rows, seed, e_clip=0.2):
    """mu / value [B], a dataset of `rows` frames and a permutation's first B indices; ratios on, inside and outside the clip and
    advantages of both signs and zero are placed by construction in the first rows of the minibatch."""
    r = np.random.RandomState(seed)
    logstd = r.uniform(-1.5, -0.3, A).astype(np.float32)
    sigma = np.exp(logstd).astype(np.float32)
    old_mu = (r.standard_normal((rows, A)) * 0.8).astype(np.float32)
    actions = (old_mu + sigma * r.standard_normal((rows, A))).astype(np.float32)
    idx = r.permutation(rows)[:B].astype(np.int64)
    mu = (old_mu[idx] + 0.02 * r.standard_normal((B, A))).astype(np.float32)
    mu[r.uniform(size=mu.shape) < 0.1] *= 2.5  # means beyond +-1: the bound loss binds
    value = r.standard_normal(B).astype(np.float32)
    adv = r.standard_normal(rows).astype(np.float32)
    ret = r.standard_normal(rows).astype(np.float32)
    data = {"actions": actions, "old_mu": old_mu, "old_sigma": sigma.copy(), "logstd": logstd, "sigma": sigma, "advantages": adv, "returns": ret}
    # old_neglogp = the new neglogp + log(wanted ratio)
    t = (actions[idx].astype(np.float64) - mu) / sigma
    nlp = 0.5 * (t * t).sum(-1) + 0.5 * math.log(2 * math.pi) * A + logstd.astype(np.float64).sum()
    want = np.exp(r.uniform(-0.5, 0.5, B))
    for bound in (1.0 - e_clip, 1.0 + e_clip):  # no drawn ratio within 2e-3 of a bound: float32 leaves a ratio exp(-neglogp) uncertain by ~1e-5 at neglogp ~ 100
        near = np.abs(want / bound - 1.0) < 2e-3
        want[near] = bound * np.where(want[near] < bound, 1.0 - 2e-3, 1.0 + 2e-3)
    # (a ratio comes out of exp(): it cannot be placed ON a bound to the bit, and there the gradient jumps - so next to the bounds, on
    # either side, at a distance no rounding crosses; inside the clip both sides of the max tie exactly, which is the tie rule's case)
    edge = [1.0, (1.0 - e_clip) * 1.001, (1.0 + e_clip) * 0.999, (1.0 - e_clip) * 0.999, (1.0 + e_clip) * 1.001, 1.0 + 3 * e_clip, 1.0 - 3 * e_clip]
    want[:min(B, len(edge))] = edge[:min(B, len(edge))]
    old = np.zeros(rows, np.float32)
    old[idx] = (nlp + np.log(want)).astype(np.float32)
    data["old_neglogp"] = old
    adv[idx[:min(B, 3)]] = [0.0, 1.0, -1.0][:min(B, 3)]
    return mu, value, data, idx


# ------------------------------------------------------------------------------------------------------------------ the scripted env
class ScriptedController:
    """A stand-in for the controller with the attributes the agent touches, scripted from a seed: the observation after step n is a
    fixed function of the step count, the env and (weakly) the action it was stepped on; done envs are reset to observations that
    depend on how often the env has been reset.  The script holds a step with no done env, done envs with terminate 0 and with 1, an env
    done twice within the horizon, a done env at the last step and rewards of both signs (asserted below).  As the controller's
    `_reset_envs` does, `reset(ids)` also serves every env whose reaction or recovery flag is up - the step raises them by the script, for
    done envs and for envs that are NOT done, also at a step with no done env - and rewrites the observation of those envs too."""

    def __init__(self, device, seed=5, dtype=torch.float32):
        r = np.random.RandomState(seed)
        self.device, self.num_envs = device, N
        f = dict(dtype=dtype, device=device)
        self.base = torch.from_numpy((r.standard_normal((4 * T + 1, N, OBS_DIM)) * 1.5).astype(np.float32)).to(**f)
        self.reset_obs = torch.from_numpy((r.standard_normal((4 * T + 1, N, OBS_DIM)) * 1.5).astype(np.float32)).to(**f)
        self.rew_script = torch.from_numpy(r.standard_normal((4 * T, N)).astype(np.float32)).to(**f)
        self.sub_script = torch.from_numpy(r.uniform(0, 1, (4 * T, N, S)).astype(np.float32)).to(**f)
        done = np.zeros((T, N), np.int64)
        term = np.zeros((T, N), np.int64)
        done[1, 0] = done[4, 0] = 1          # env 0: done twice
        term[4, 0] = 1
        done[2, 3] = 1                       # terminate 0
        done[5, 1] = term[5, 1] = 1
        done[T - 1, 4] = 1                   # at the last step
        done[T - 1, 2] = term[T - 1, 2] = 1
        assert (done.sum(1) == 0).any() and (done.sum(0) == 2).any() and done[T - 1].any() and (done & (1 - term)).any() and (done & term).any()
        assert bool((self.rew_script[:T] > 0).any()) and bool((self.rew_script[:T] < 0).any())
        self.done_script = torch.from_numpy(np.tile(done, (4, 1))).to(device)
        self.term_script = torch.from_numpy(np.tile(term, (4, 1))).to(device)
        self.proj = torch.from_numpy((0.05 * r.standard_normal((A, OBS_DIM))).astype(np.float32)).to(**f)
        self.obs_buf, self.rew_buf = self.base[0].clone(), torch.zeros(N, **f)
        self.reset_buf, self._terminate_buf = torch.zeros(N, dtype=torch.long, device=device), torch.zeros(N, dtype=torch.long, device=device)
        self._sub_rewards = torch.zeros((N, S), **f)
        self.extras = {"terminate": self._terminate_buf, "sub_rewards": self._sub_rewards}
        self.cfg_v2p = {"aux_loss_specs": {"dof_res": 0.01}}
        self._num_res_dof_action = 3
        self.steps, self.resets = 0, torch.zeros(N, dtype=torch.long, device=device)
        self.seen_actions = []
        self.flag_obs = torch.from_numpy((r.standard_normal((4 * T + 1, N, OBS_DIM)) * 1.5).astype(np.float32)).to(**f)
        react, recov = done.astype(bool), np.zeros((T, N), bool)   # a done env gets a reaction task
        react[0, 5] = react[3, 2] = react[6, 1] = True              # not done; steps 0, 3 and 6 have no done env at all
        recov[3, 4] = recov[5, 5] = True
        assert (react & ~done.astype(bool)).any() and (recov & ~done.astype(bool)).any() and ((react | recov)[done.sum(1) == 0]).any()
        self.react_script, self.recov_script = (torch.from_numpy(np.tile(m, (4, 1))).to(device) for m in (react, recov))
        self._reset_reaction_buf, self._reset_recovery_buf = torch.zeros(N, dtype=torch.bool, device=device), torch.zeros(N, dtype=torch.bool, device=device)

    def get_action_size(self):
        return A

    def reset(self, ids):
        if len(ids):
            self.resets[ids] += 1
            self.obs_buf[ids] = self.reset_obs[self.resets[ids], ids]
        served = self._reset_reaction_buf | self._reset_recovery_buf
        if len(ids):
            served[ids] = False  # (their rows are the reset's)
        self.obs_buf.copy_(torch.where(served.unsqueeze(1), self.flag_obs[self.steps], self.obs_buf))
        self._reset_reaction_buf[:] = False
        self._reset_recovery_buf[:] = False

    def step(self, actions):
        n = self.steps
        self.seen_actions.append(actions.clone())
        self.obs_buf.copy_(self.base[n + 1] + torch.tanh(actions) @ self.proj)
        self.rew_buf.copy_(self.rew_script[n])
        self._sub_rewards.copy_(self.sub_script[n])
        self.reset_buf.copy_(self.done_script[n])
        self._terminate_buf.copy_(self.term_script[n])
        self._reset_reaction_buf |= self.react_script[n]
        self._reset_recovery_buf |= self.recov_script[n]
        self.steps += 1
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras


def play_steps_statement(agent, ctl, noise):
    """`V2PAgent.play_steps` (agents/v2p_agent.py:220-297) as the reference writes it, in torch, on `ctl`: two full critic passes per step
    through the agent's `get_action_values` / `_eval_critic`, the bookkeeping in torch ops.  Returns the buffer dict ([T, N, ...]), the
    returns [T, N] and what the meters received."""
    from vid2player3d_amd.learning import discount_values

    agent.set_eval()
    agent.running_mean_std.sync()
    dev, c = ctl.device, agent.clip_obs
    z = lambda *s: torch.zeros(s, device=dev)
    td = {"obses": z(T, N, OBS_DIM), "next_obses": z(T, N, OBS_DIM), "rewards": z(T, N), "dones": z(T, N), "values": z(T, N), "next_values": z(T, N),
          "actions": z(T, N, A), "mus": z(T, N, A), "sigmas": z(T, N, A), "neglogpacs": z(T, N)}
    cur_r, cur_l = z(N), z(N)
    game_r, game_l, step_r, step_sub = [], [], [], []
    done_ids = torch.zeros(0, dtype=torch.long, device=dev)
    ctl.reset(done_ids)
    obs = torch.clamp(ctl.obs_buf, -c, c)
    for n in range(T):
        td["obses"][n] = obs
        res = agent.get_action_values(obs, noise[n])
        for k in ("actions", "mus", "sigmas", "neglogpacs"):
            td[k][n] = res[k]
        td["values"][n] = res["values"].reshape(-1)
        ctl.step(torch.clamp(res["actions"], -agent.clip_actions, agent.clip_actions))
        obs, rewards, dones = torch.clamp(ctl.obs_buf, -c, c), ctl.rew_buf.clone(), ctl.reset_buf.clone()
        td["rewards"][n], td["next_obses"][n], td["dones"][n] = rewards, obs, dones.float()
        terminated = ctl.extras["terminate"].float()
        td["next_values"][n] = agent._eval_critic(obs).reshape(-1) * (1.0 - terminated)
        cur_r += rewards
        cur_l += 1
        done_ids = dones.nonzero(as_tuple=False).flatten()
        game_r.append(cur_r[done_ids].clone())
        game_l.append(cur_l[done_ids].clone())
        step_r.append(rewards.mean())
        step_sub.append(ctl.extras["sub_rewards"].mean(0))
        not_dones = 1.0 - dones.float()
        cur_r, cur_l = cur_r * not_dones, cur_l * not_dones
        ctl.reset(done_ids)
        obs = torch.clamp(ctl.obs_buf, -c, c)
    advs = discount_values(td["dones"], td["values"].unsqueeze(-1).contiguous(), td["rewards"].unsqueeze(-1).contiguous(), td["next_values"].unsqueeze(-1).contiguous(),
                           agent.gamma, agent.tau).squeeze(-1)
    meters = {"game_rewards": torch.cat(game_r), "game_lengths": torch.cat(game_l), "step_rewards": torch.stack(step_r).mean(), "step_sub_rewards": torch.stack(step_sub).mean(0)}
    return td, advs + td["values"], meters


# ------------------------------------------------------------------------------------------------------------------ checkpoints
# the loading cases recorded from the reference's load_pretrained: (columns of the checkpoint's observation, its actions, discard_pretrained_sigma)
LOAD_CASES = {"same": (OBS_DIM, A, False), "narrow_obs": (OBS_DIM - 4, A, False), "narrow_act": (OBS_DIM, A - 3, False), "narrow_both": (OBS_DIM - 4, A - 3, False),
              "discard_sigma": (OBS_DIM, A, True)}


def synthetic_checkpoint(obs_dim, num_actions, units=UNITS, seed=77):
    """A checkpoint dict with the reference's key names, of a network obs_dim -> num_actions."""
    r = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))
    model, d = {}, obs_dim
    for part in ("actor_mlp", "critic_mlp"):
        d = obs_dim
        for k, u in enumerate(units):
            model["a2c_network.%s.%d.weight" % (part, 2 * k)], model["a2c_network.%s.%d.bias" % (part, 2 * k)] = t(u, d), t(u)
            d = u
    model["a2c_network.mu.weight"], model["a2c_network.mu.bias"] = t(num_actions, d), t(num_actions)
    model["a2c_network.value.weight"], model["a2c_network.value.bias"] = t(1, d), t(1)
    model["a2c_network.sigma"] = t(num_actions)
    f64 = lambda *s: torch.from_numpy(r.uniform(0.1, 2.0, s))
    return {"model": model, "running_mean_std": {"running_mean": f64(obs_dim) - 1.0, "running_var": f64(obs_dim), "count": torch.tensor(321.0, dtype=torch.float64)},
            "reward_mean_std": {"running_mean": f64(1), "running_var": f64(1), "count": torch.tensor(55.0, dtype=torch.float64)}}
