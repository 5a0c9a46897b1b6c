"""Policy inference for the tennis controller: the low-level imitation policy and the controller's own actor, closed into the control step.

What `ImitatorPlayer.run_one_step` (vid2player/players/im_player.py:187-199) does around the physics player's task - clamp `obs_buf` to
+-clip_obs, `ImitatorBuilder.Network.eval_actor` (models/im_network_builder.py:53-81: `RunningNorm` in eval mode, models/running_norm.py:31-42,
`actor_mlp`, `mu`), clamp to +-clip_actions, `_action_to_pd_targets` - and what `V2PPlayer.get_action` (players/v2p_player.py:113-131)
does for the controller: rl_games' `RunningMeanStd` (normalize_input) or the network's own `running_obs`, then `V2PBuilder.Network.eval_actor`.
Under the match configs the networks are `ImitatorBuilderDual.Network` / `V2PBuilderDual.Network` (models/im_network_builder_dual.py:37-45):
rows 0::2 through `network1`, rows 1::2 through `network2`, outputs interleaved.

The dense layers are torch's (hipBLASLt; `ppo._mlp_forward`: bias + ReLU in the GEMM's epilogue).  Everything around them is three
kernels of csrc/policy_io.hip: `v2p_policy_input`, `v2p_ll_policy_input` (the 734-d imitation observation computed in place from the
engine's state, then the same tail), `v2p_ll_policy_actions`.  A two-player batch is written in side-major order - env i is row
(i & 1) * (N / 2) + (i >> 1) - so each network reads one contiguous half and writes one: no gather, no interleaving cat.
`LowLevelPolicy.step()` is launch -> GEMMs per side -> launch, without a host synchronisation or an allocation.

`policy_input_reference`, `ll_policy_actions_reference` and `actor_reference` are the numpy statement of the same calls - the checker of
the tests; the product never calls them.  There is no CPU path for the policies: a CPU device or a missing library is a RuntimeError.

Checkpoints: the caller loads the file (`torch.load`) and hands over the dict, as `mvae.weights_from_state_dict` has it; no class of the
reference is unpickled.  Built: the shipped option set - ReLU MLPs, no mu activation, fixed sigma, no CNN, no RNN.  Anything else raises.
Critics, sampling, `neglogp` and the controller's PPO agent for these networks: `ctl_ppo.py`.  Not built: `vid2player_dual_v2`.
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, mvae_target
from .ppo import _mlp_forward

NORM_KINDS = _lib.NORM_KINDS
NUM_OBS_IM = mvae_target.NUM_OBS_IM
RUNNING_EPS = 1e-8       # models/running_norm.py:39
MEAN_VAR_EPS = 1e-5      # rl_games RunningMeanStd(epsilon=1e-05)
NORM_CLIP = 5.0          # RunningNorm(clip=5.0); rl_games clamps to +-5.0
PREFIX = "a2c_network."


# ------------------------------------------------------------------------------------------------------------------ normalisers
class Normaliser:
    """The input normaliser of one network: kind 'none' (identity: a `RunningNorm` with n == 0), 'running'
    (clamp((x - mean) / (spread + 1e-8), +-clip), spread = std) or 'mean_var' (clamp((x - mean) / sqrt(spread + eps), +-clip), spread = var)."""

    def __init__(self, kind, mean=None, spread=None, eps=MEAN_VAR_EPS, clip=NORM_CLIP):
        if kind not in NORM_KINDS:
            raise ValueError("Normaliser: kind %r is none of %s" % (kind, sorted(NORM_KINDS)))
        self.kind, self.eps, self.clip = kind, float(eps), float(clip)
        if kind == "none":
            self.mean = self.spread = None
            return
        if mean is None or spread is None:
            raise ValueError("Normaliser: kind %r needs mean and spread" % kind)
        self.mean = np.ascontiguousarray(_to_numpy(mean), dtype=np.float32).reshape(-1)
        self.spread = np.ascontiguousarray(_to_numpy(spread), dtype=np.float32).reshape(-1)
        if self.mean.shape != self.spread.shape:
            raise ValueError("Normaliser: mean %s and spread %s differ in shape" % (self.mean.shape, self.spread.shape))
        if not self.clip > 0:
            raise ValueError("Normaliser: clip %r is not > 0" % (clip,))

    @property
    def dim(self):
        return None if self.mean is None else len(self.mean)


def _to_numpy(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _padded(v, dim, fill):
    v = np.asarray(_to_numpy(v), dtype=np.float32).reshape(-1)
    if dim is None or len(v) == dim:
        return v
    if len(v) > dim:
        raise ValueError("the checkpoint's statistics have %d columns, the observation %d" % (len(v), dim))
    out = np.full(dim, fill, np.float32)
    out[:len(v)] = v
    return out


def network_norm(checkpoint, obs_dim=None, prefix=PREFIX):
    """The normaliser INSIDE the network (`running_obs`, use_running_obs) as the reference's loaders leave it.  `running_obs.n / mean / std`
    in the model dict: they are the `RunningNorm`'s (kind 'running', or 'none' while n == 0).  Without them, `load_dual_cp`'s rule
    (players/v2p_player.py:54-69, players/im_player.py:76-91): the checkpoint's `running_mean_std`, else the model's
    `running_obs.running_mean / running_var / count`, cast to float32, zero-padded to obs_dim, std = sqrt(var), n = count.  Neither: the
    network's fresh `RunningNorm` stays at n == 0, kind 'none'."""
    model = checkpoint["model"]
    key = lambda k: prefix + "running_obs." + k
    if key("n") in model:
        if int(_to_numpy(model[key("n")])) == 0:
            return Normaliser("none")
        return Normaliser("running", _padded(model[key("mean")], obs_dim, 0.0), _padded(model[key("std")], obs_dim, 0.0), clip=NORM_CLIP)
    if "running_mean_std" in checkpoint:
        rms = checkpoint["running_mean_std"]
        mean, var, count = rms["running_mean"], rms["running_var"], rms["count"]
    elif key("running_mean") in model:
        mean, var, count = model[key("running_mean")], model[key("running_var")], model[key("count")]
    else:
        return Normaliser("none")
    if int(np.asarray(_to_numpy(count)).astype(np.int64)) == 0:  # (`count.long()`)
        return Normaliser("none")
    var32 = _padded(var, obs_dim, 0.0)
    return Normaliser("running", _padded(mean, obs_dim, 0.0), np.sqrt(var32), clip=NORM_CLIP)


def input_norm(checkpoint, obs_dim=None):
    """The normaliser in FRONT of the network (`normalize_input`: rl_games' `RunningMeanStd`, `_preproc_obs`) from the checkpoint's
    `running_mean_std`, statistics cast to float32; a narrower checkpoint fills the first columns of a fresh one (mean 0, var 1:
    players/v2p_player.py:93-95).  Kind 'mean_var'."""
    if "running_mean_std" not in checkpoint:
        raise ValueError("input_norm: the checkpoint has no running_mean_std")
    rms = checkpoint["running_mean_std"]
    return Normaliser("mean_var", _padded(rms["running_mean"], obs_dim, 0.0), _padded(rms["running_var"], obs_dim, 1.0), eps=MEAN_VAR_EPS, clip=NORM_CLIP)


def _clamp_np(v, c, dt):
    """torch.clamp(v, -c, c) on arrays: compare-and-select, so that a NaN stays a NaN and an infinite clip changes nothing."""
    c = dt(c)
    v = np.where(v < -c, -c, v)
    return np.where(v > c, c, v).astype(dt)


def normalise_reference(norm, x, dt=np.float32):
    """One `Normaliser` on rows x [n,dim], elementwise in dt."""
    x = np.asarray(x, dtype=dt)
    if norm.kind == "none":
        return x.copy()
    with np.errstate(all="ignore"):
        if norm.kind == "running":
            y = (x - norm.mean.astype(dt)) / (norm.spread.astype(dt) + dt(RUNNING_EPS))
        else:
            y = (x - norm.mean.astype(dt)) / np.sqrt(norm.spread.astype(dt) + dt(norm.eps))
        return _clamp_np(y.astype(dt), norm.clip, dt)


def side_major_rows(n, sides):
    """row[i]: the network's row of env i."""
    i = np.arange(n, dtype=np.int64)
    return i if sides == 1 else (i & 1) * (n // 2) + (i >> 1)


def policy_input_reference(obs, norms, sides=1, clip_obs=math.inf, dt=np.float32):
    """`v2p_policy_input` on arrays: obs [n,dim] in env order -> x [n,dim] in side-major order."""
    obs = np.asarray(obs, dtype=dt)
    n = len(obs)
    norms = _as_list(norms, sides, "norms")
    if sides == 2 and n % 2:
        raise ValueError("policy_input_reference: n %d is odd with two sides" % n)
    with np.errstate(all="ignore"):
        c = _clamp_np(obs, clip_obs, dt)
    x = np.empty_like(c)
    rows = side_major_rows(n, sides)
    for s in range(sides):
        x[rows[s::sides]] = normalise_reference(norms[s], c[s::sides], dt)
    return x


def env_order(rows_side_major, sides):
    """Side-major rows [n,...] back in env order (the interleave of models/im_network_builder_dual.py:45)."""
    a = np.asarray(rows_side_major)
    return a[side_major_rows(len(a), sides)]


def ll_policy_actions_reference(st, mu, sides=1, clip_actions=math.inf, dt=np.float32, **bases):
    """`v2p_ll_policy_actions` on arrays: mu [n,75] side-major -> `_action_to_pd_targets` of clamp(mu, +-clip_actions) in env order.
    st and **bases (target, dof_state, pd_action_scale, pd_action_offset): as `mvae_target.target_actions_reference`."""
    with np.errstate(all="ignore"):
        a = _clamp_np(env_order(np.asarray(mu, dtype=dt), sides), clip_actions, dt)
    return mvae_target.target_actions_reference(st, a, dt=dt, **bases)


def actor_reference(weights, x, dt=np.float32):
    """`eval_actor` behind the normaliser on arrays: weights = [(W, b), ...] of actor_mlp's Linear layers and last of `mu`; ReLU between."""
    h = np.asarray(x, dtype=dt)
    for k, (w, b) in enumerate(weights):
        h = h @ np.asarray(w, dtype=dt).T + np.asarray(b, dtype=dt)
        if k + 1 < len(weights):
            h = np.maximum(h, dt(0))
    return h.astype(dt)


def _as_list(v, sides, what):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    if len(v) != sides:
        raise ValueError("%s: %d given for %d side%s" % (what, len(v), sides, "" if sides == 1 else "s"))
    return v


# ------------------------------------------------------------------------------------------------------------------ the actor
def check_network_params(params):
    """Refuse what is outside the shipped option set of a `network` section (cfg/*/train yaml: mlp.activation relu, no cnn / rnn,
    space.continuous with mu_activation None and fixed_sigma True)."""
    p = dict(params or {})
    act = (p.get("mlp") or {}).get("activation", "relu")
    if act != "relu":
        raise NotImplementedError("ActorMLP: mlp.activation %r is not built (only relu)" % (act,))
    for k in ("cnn", "rnn"):
        if p.get(k):
            raise NotImplementedError("ActorMLP: a %s section is not built" % k)
    space = p.get("space") or {}
    if space and "continuous" not in space:
        raise NotImplementedError("ActorMLP: only a continuous action space is built")
    cont = space.get("continuous") or {}
    if cont.get("mu_activation", "None") not in ("None", None):
        raise NotImplementedError("ActorMLP: mu_activation %r is not built" % (cont.get("mu_activation"),))
    if not cont.get("fixed_sigma", True):
        raise NotImplementedError("ActorMLP: a learned sigma (fixed_sigma: False) is not built")


class ActorMLP(nn.Module):
    """`actor_mlp` (Linear + ReLU pairs: modules 0, 2, 4, ...) and `mu` of an `ImitatorBuilder.Network` / `V2PBuilder.Network`."""

    def __init__(self, obs_dim, units, num_actions):
        super().__init__()
        layers, d = [], int(obs_dim)
        for u in units:
            layers += [nn.Linear(d, int(u)), nn.ReLU()]
            d = int(u)
        self.actor_mlp = nn.Sequential(*layers)
        self.mu = nn.Linear(d, int(num_actions))
        self.obs_dim, self.num_actions = int(obs_dim), int(num_actions)
        for p in self.parameters():
            p.requires_grad_(False)

    @classmethod
    def from_state_dict(cls, model, obs_dim=None, prefix=PREFIX, params=None):
        """From a checkpoint's `model` dict (keys `<prefix>actor_mlp.{0,2,4}.weight/bias`, `<prefix>mu.weight/bias`).  A first layer
        narrower than obs_dim is zero-padded on the right (players/v2p_player.py:41-50, 79-90); a wider one is a ValueError."""
        check_network_params(params)
        sd = {k[len(prefix):]: v for k, v in model.items() if k.startswith(prefix)}
        if not sd:
            raise ValueError("ActorMLP: no key of the model dict starts with %r" % prefix)
        for k in sd:
            if k.startswith(("actor_cnn.", "critic_cnn.")) or "rnn" in k.split(".")[0]:
                raise NotImplementedError("ActorMLP: the checkpoint has a CNN / RNN (%s): not built" % k)
        if "sigma.weight" in sd:
            raise NotImplementedError("ActorMLP: the checkpoint has a learned sigma layer: not built")
        idx = sorted(int(k.split(".")[1]) for k in sd if k.startswith("actor_mlp.") and k.endswith(".weight"))
        if not idx or idx != list(range(0, 2 * len(idx), 2)) or "mu.weight" not in sd:
            raise ValueError("ActorMLP: the model dict has no actor_mlp.{0,2,..} Linear layers followed by mu (found actor_mlp layers %s)" % idx)
        w0 = sd["actor_mlp.0.weight"]
        width = int(w0.shape[1])
        obs_dim = width if obs_dim is None else int(obs_dim)
        if width > obs_dim:
            raise ValueError("ActorMLP: the checkpoint's first layer reads %d columns, the observation has %d" % (width, obs_dim))
        net = cls(obs_dim, [int(sd["actor_mlp.%d.weight" % i].shape[0]) for i in idx], int(sd["mu.weight"].shape[0]))
        with torch.no_grad():
            for i in idx:
                lin = net.actor_mlp[i]
                w = torch.as_tensor(sd["actor_mlp.%d.weight" % i], dtype=torch.float32)
                if i == 0:
                    lin.weight.zero_()
                    lin.weight[:, :width] = w
                else:
                    lin.weight.copy_(w)
                lin.bias.copy_(torch.as_tensor(sd["actor_mlp.%d.bias" % i], dtype=torch.float32))
            net.mu.weight.copy_(torch.as_tensor(sd["mu.weight"], dtype=torch.float32))
            net.mu.bias.copy_(torch.as_tensor(sd["mu.bias"], dtype=torch.float32))
        return net

    def layer_arrays(self):
        """[(W, b), ...] as numpy arrays: what `actor_reference` takes."""
        lins = [m for m in self.actor_mlp if isinstance(m, nn.Linear)] + [self.mu]
        return [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in lins]

    def forward(self, x, out=None):
        """mu [rows, A] of normalised rows x; `out` receives it (a slice of a side-major buffer)."""
        h = _mlp_forward(self.actor_mlp, x)
        if out is None:
            return self.mu(h)
        return torch.addmm(self.mu.bias, h, self.mu.weight.t(), out=out)


# ------------------------------------------------------------------------------------------------------------------ the launches
class InputCfg:
    """v2p_policy_input_cfg of a list of `Normaliser`s, with the device copies of their statistics kept alive next to it."""

    def __init__(self, norms, sides, dim, clip_obs, device, who):
        norms = _as_list(norms, sides, who + ": norms")
        if not float(clip_obs) > 0:
            raise ValueError("%s: clip_obs %r is not > 0" % (who, clip_obs))
        self.cfg = _lib.PolicyInputCfg(sides=int(sides), clip_obs=float(clip_obs))
        self._keep = []
        for s, nm in enumerate(norms):
            if not isinstance(nm, Normaliser):
                raise TypeError("%s: norms are Normaliser objects (network_norm / input_norm), got %s" % (who, type(nm).__name__))
            c = self.cfg.norm[s]
            c.kind, c.eps, c.clip = NORM_KINDS[nm.kind], nm.eps, nm.clip
            if nm.kind == "none":
                continue
            if nm.dim != dim:
                raise ValueError("%s: side %d's normaliser has %d columns, the observation %d" % (who, s, nm.dim, dim))
            mean, spread = (torch.from_numpy(a).to(device).contiguous() for a in (nm.mean, nm.spread))
            self._keep += [mean, spread]
            c.mean, c.spread = mean.data_ptr(), spread.data_ptr()


def launch_policy_input(cfg, n, dim, obs, x):
    dev = x.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_policy_input(C.byref(cfg), int(n), int(dim), _lib.ptr(obs), _lib.ptr(x), _lib.current_stream(dev)), "v2p_policy_input")


def launch_ll_policy_input(cfg, n, src, raw_obs, x):
    dev = x.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_ll_policy_input(C.byref(cfg), int(n), NUM_OBS_IM, C.byref(src), _lib.ptr(raw_obs), _lib.ptr(x), _lib.current_stream(dev)),
                   "v2p_ll_policy_input")


def launch_ll_policy_actions(st, tensors, n, sides, clip_actions, mu, out, num_shapes=1):
    dev = mu.device
    c, b = mvae_target.cfg_struct(st, num_shapes), mvae_target.buffers_struct(tensors)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_ll_policy_actions(C.byref(c), int(n), int(sides), float(clip_actions), _lib.ptr(mu), C.byref(b), _lib.ptr(out),
                                                     _lib.current_stream(dev)), "v2p_ll_policy_actions")


def _check_actors(actors, sides, obs_dim, num_actions, device, who):
    actors = _as_list(actors, sides, who + ": actors")
    for a in actors:
        if not isinstance(a, ActorMLP):
            raise TypeError("%s: actors are ActorMLP objects, got %s" % (who, type(a).__name__))
        if a.obs_dim != obs_dim or (num_actions is not None and a.num_actions != num_actions):
            raise ValueError("%s: an actor maps %d -> %d, the task needs %d -> %s" % (who, a.obs_dim, a.num_actions, obs_dim, num_actions if num_actions is not None else "A"))
        a.to(device).eval()
    if len({a.num_actions for a in actors}) != 1:
        raise ValueError("%s: the two actors differ in their action width" % who)
    return actors


# ------------------------------------------------------------------------------------------------------------------ the objects
class LowLevelPolicy:
    """`ImitatorPlayer.run_one_step` up to the engine's step, around an `ImitationTarget`: one `ActorMLP` and `Normaliser`, or two of each with
    a two-player target (side 0 = envs 0::2 = `network1`).  clip_obs / clip_actions: the env's `clip_obs` / `clip_actions`."""

    def __init__(self, target, actors, norms, clip_obs=math.inf, clip_actions=math.inf):
        if not isinstance(target, mvae_target.ImitationTarget):
            raise TypeError("LowLevelPolicy wraps an ImitationTarget")
        self.target, self.device, self.num_envs = target, target.device, target.num_envs
        two_player = getattr(target.task, "racket_players", None) is not None
        given = len(actors) if isinstance(actors, (list, tuple)) else 1
        if given == 2 and not two_player:
            raise ValueError("LowLevelPolicy: two actors go with a two-player target")
        self.sides = given
        if self.sides == 2 and self.num_envs % 2:
            raise ValueError("LowLevelPolicy: a two-player batch has an even number of envs, got %d" % self.num_envs)
        if not float(clip_actions) > 0:
            raise ValueError("LowLevelPolicy: clip_actions %r is not > 0" % (clip_actions,))
        _lib.load()
        self.actors = _check_actors(actors, self.sides, NUM_OBS_IM, _lib.NUM_ACTIONS, self.device, "LowLevelPolicy")
        self._input = InputCfg(norms, self.sides, NUM_OBS_IM, clip_obs, self.device, "LowLevelPolicy")
        self.clip_obs, self.clip_actions = float(clip_obs), float(clip_actions)
        f = dict(dtype=torch.float32, device=self.device)
        self.x = torch.zeros((self.num_envs, NUM_OBS_IM), **f)          # the networks' input, side-major
        self.mu = torch.zeros((self.num_envs, _lib.NUM_ACTIONS), **f)   # their output, side-major
        self.pd_actions = torch.zeros((self.num_envs, _lib.NUM_ACTIONS), **f)
        h = self.num_envs // self.sides
        self._halves = [(self.x[s * h:(s + 1) * h], self.mu[s * h:(s + 1) * h]) for s in range(self.sides)]

    def _src(self):
        tg, t = self.target, self.target.task
        row = t._target_bufs[t._cur]
        for name, v in (("_rigid_body_state", t._rigid_body_state), ("_dof_state", t._dof_state), ("target", row)):
            if not v.is_contiguous() or v.dtype != torch.float32:
                raise RuntimeError("LowLevelPolicy: the task's %s must be a contiguous float32 tensor" % name)
        return _lib.LLPolicySrc(rb_state=t._rigid_body_state.data_ptr(), dof_state=t._dof_state.data_ptr(), target=row.data_ptr(),
                                target_stride=row.stride(0), motion_bodies=tg._reset_ref_motion_bodies.data_ptr()), row

    @torch.no_grad()
    def step(self):
        """The [N,75] PD-target actions of this control step (a buffer of this object; the engine clamps them) from the engine's state
        and the current target; `target.obs_buf` receives the raw observation on the way."""
        tg, n = self.target, self.num_envs
        src, row = self._src()
        launch_ll_policy_input(self._input.cfg, n, src, tg.obs_buf, self.x)
        for actor, (x, mu) in zip(self.actors, self._halves):
            actor(x, out=mu)
        launch_ll_policy_actions(tg.settings, tg._tensors(row), n, self.sides, self.clip_actions, self.mu, self.pd_actions, len(tg._joint_pos_bind))
        return self.pd_actions


class ControllerPolicy:
    """`V2PPlayer.get_action(..., is_determenistic=True)` for a controller task: mu [N,A] of `ctl.obs_buf`.  One `ActorMLP` and
    `Normaliser`, or two of each over a two-player controller.  clip_actions_val: the player's clamp of the action (inf: none)."""

    def __init__(self, ctl, actors, norms, clip_obs=math.inf, clip_actions_val=math.inf):
        dev = torch.device(ctl.device)
        if dev.type != "cuda":
            raise RuntimeError("ControllerPolicy: the controller must live on a GPU (no CPU fallback)")
        self.ctl, self.device, self.num_envs = ctl, dev, ctl.num_envs
        two_player = getattr(ctl.task, "racket_players", None) is not None
        given = len(actors) if isinstance(actors, (list, tuple)) else 1
        if given == 2 and not two_player:
            raise ValueError("ControllerPolicy: two actors go with a two-player controller")
        self.sides = given
        if self.sides == 2 and self.num_envs % 2:
            raise ValueError("ControllerPolicy: a two-player batch has an even number of envs, got %d" % self.num_envs)
        if not float(clip_actions_val) > 0:
            raise ValueError("ControllerPolicy: clip_actions_val %r is not > 0" % (clip_actions_val,))
        _lib.load()
        self.obs_dim = int(ctl.obs_buf.shape[1])
        self.actors = _check_actors(actors, self.sides, self.obs_dim, None, dev, "ControllerPolicy")
        self.num_actions = self.actors[0].num_actions
        self._input = InputCfg(norms, self.sides, self.obs_dim, clip_obs, dev, "ControllerPolicy")
        self.clip_actions_val = float(clip_actions_val)
        f = dict(dtype=torch.float32, device=dev)
        self.x = torch.zeros((self.num_envs, self.obs_dim), **f)
        self.mu_side_major = torch.zeros((self.num_envs, self.num_actions), **f)
        self.mu = torch.zeros((self.num_envs, self.num_actions), **f)
        h = self.num_envs // self.sides
        self._halves = [(self.x[s * h:(s + 1) * h], self.mu_side_major[s * h:(s + 1) * h]) for s in range(self.sides)]

    @torch.no_grad()
    def act(self, obs=None):
        """The deterministic action mu [N,A] (a buffer of this object) of `ctl.obs_buf`, or of obs [N,obs_dim]."""
        obs = self.ctl.obs_buf if obs is None else obs
        if obs.dtype != torch.float32 or not obs.is_cuda or not obs.is_contiguous() or tuple(obs.shape) != (self.num_envs, self.obs_dim):
            raise RuntimeError("ControllerPolicy.act: obs must be a contiguous float32 GPU tensor [%d, %d]" % (self.num_envs, self.obs_dim))
        launch_policy_input(self._input.cfg, self.num_envs, self.obs_dim, obs, self.x)
        for actor, (x, mu) in zip(self.actors, self._halves):
            actor(x, out=mu)
        h, c = self.num_envs // self.sides, self.clip_actions_val
        # the interleave (side-major -> env order) and the clamp in one elementwise pass
        torch.clamp(self.mu_side_major.view(self.sides, h, self.num_actions).transpose(0, 1), -c, c, out=self.mu.view(h, self.sides, self.num_actions))
        return self.mu
