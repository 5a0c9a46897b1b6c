"""What the controller's PPO agent (vid2player3d_amd/ctl_ppo.py) costs on the GPU at the sizes of federer_train_stage_1.yaml: 10240 envs,
horizon 64, minibatches of 16384 frames, units 1024 / 1024 / 512, on a racket + ball controller with generator, target and low-level
policy attached.

  (a) per rollout step, the network side of `play_steps` (everything but `ctl.step` and the resets):
        step_kernels   (step_kernels_second_critic: a step whose reset rewrote a row, with the second critic pass) v2p_policy_input -> actor -> v2p_ctl_policy_head -> v2p_ctl_rollout_record -> v2p_policy_input -> critic -> v2p_value_record
        step_torch     the same bookkeeping as the reference writes it in torch ops (v2p_agent.py:231-276: two critic passes, update_data
                       copies, clamp, the meters' means)
        host_read      `dones.nonzero()`; host_read_lists: the one host read of a step as the agent does it (done and changed rows)
        record_kernel / record_torch    `v2p_ctl_rollout_record` alone (one workgroup takes the per-env work) against its torch lines
  (b) per minibatch:
        grads_fused / grads_torch    `calc_gradients` with fused_loss on / off
        head_kernel / head_torch     the loss head alone, forward and backward down to d loss / d mu, d loss / d value
  (c) a whole epoch: T_play / T_update of `train_epoch`, fused_loss on and off.

Device events around `--iters` repetitions after `--warmup`, `--rounds` rounds alternating the candidates; one JSON line per figure and a
summary line (medians, min - max) at the end.
    python tools/ctl_ppo_bench.py [--envs 10240] [--horizon 64] [--minibatch 16384] [--iters 50] [--warmup 5] [--rounds 3] [--epochs 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from mvae_bench import DEV, timed  # noqa: E402

from tests import ctl_ppo_fixture as FX  # noqa: E402
from tests import policies_fixture as PF  # noqa: E402
from vid2player3d_amd import ctl_ppo as CP  # noqa: E402
from vid2player3d_amd import policies as P  # noqa: E402

UNITS = (1024, 1024, 512)


def make(n, horizon, minibatch):
    ctl, task, player, target = PF.single_controller(n)
    ll = P.LowLevelPolicy(target, PF.random_actors(1, 734, 75, units=UNITS, seed=31)[0], PF.random_norms(1, 734, seed=41)[0], 5.0, 1.0)
    ctl.attach_low_level_policy(ll)
    params = FX.YAML_PARAMS["federer_train_stage_1"]
    return ctl, CP.ControllerPPOAgent.from_config(ctl, params, horizon_length=horizon, minibatch_size=minibatch)


def rollout_forms(agent, ctl):
    td, N, A = agent.tensor_dict, agent.num_actors, agent.num_actions
    noise = torch.randn((N, A), device=DEV)
    rms, vms = agent.running_mean_std, agent.value_mean_std
    cur = {"r": torch.zeros(N, device=DEV), "l": torch.zeros(N, device=DEV)}

    @torch.no_grad()
    def step_kernels(second_critic=False):
        agent._policy_input(td["obses"][0], agent.x)
        agent._policy_head(agent.model.actor(agent.x), noise, 0)
        agent._rollout_record(0)
        agent._policy_input(td["next_obses"][0], agent.x)
        agent._value_record(agent.model.critic(agent.x), agent.terminated, td["values"][1], td["next_values"][0])
        agent._policy_input(td["obses"][1], agent.x)  # (behind the reset: all rows again)
        if second_critic:
            agent._value_record(agent.model.critic(agent.x), None, td["values"][1], None)

    def preproc(obs):
        return torch.clamp((obs - rms.running_mean.float()) / torch.sqrt(rms.running_var.float() + 1e-5), -5.0, 5.0)

    @torch.no_grad()
    def step_torch():
        obs = td["obses"][0]
        x = preproc(obs)
        mu = agent.model.actor(x)
        logstd = mu * 0.0 + agent.model.sigma
        sigma = torch.exp(logstd)
        actions = mu + sigma * noise
        nlp = 0.5 * (((actions - mu) / sigma) ** 2).sum(dim=-1) + 0.5 * CP.LOG_2PI * A + logstd.sum(dim=-1)
        value = vms(agent.model.critic(x), True)
        for k, v in (("actions", actions), ("mus", mu), ("sigmas", sigma), ("neglogpacs", nlp), ("values", value.reshape(-1))):
            td[k][0, :] = v
        clipped = torch.clamp(actions, -agent.clip_actions, agent.clip_actions)  # noqa: F841  (what env_step is called on)
        obs2 = torch.clamp(ctl.obs_buf, -agent.clip_obs, agent.clip_obs)
        td["rewards"][0, :] = ctl.rew_buf
        td["next_obses"][0, :] = obs2
        td["dones"][0, :] = ctl.reset_buf
        terminated = ctl.extras["terminate"].float().unsqueeze(-1)
        next_vals = vms(agent.model.critic(preproc(obs2)), True)
        next_vals *= 1.0 - terminated
        td["next_values"][0, :] = next_vals.reshape(-1)
        cur["r"] += ctl.rew_buf
        cur["l"] += 1
        ctl.rew_buf.mean(dim=0)
        ctl.extras["sub_rewards"].mean(dim=0)
        not_dones = 1.0 - ctl.reset_buf.float()
        cur["r"], cur["l"] = cur["r"] * not_dones, cur["l"] * not_dones

    def host_read():
        return td["dones"][0].nonzero(as_tuple=False)

    def host_read_lists():
        return agent._reset_lists(td["dones"][0])

    @torch.no_grad()
    def record_torch():
        td["rewards"][0, :] = ctl.rew_buf
        td["next_obses"][0, :] = torch.clamp(ctl.obs_buf, -agent.clip_obs, agent.clip_obs)
        td["dones"][0, :] = ctl.reset_buf
        ctl.extras["terminate"].float()
        cur["r"] += ctl.rew_buf
        cur["l"] += 1
        ctl.rew_buf.mean(dim=0)
        ctl.extras["sub_rewards"].mean(dim=0)
        not_dones = 1.0 - ctl.reset_buf.float()
        cur["r"], cur["l"] = cur["r"] * not_dones, cur["l"] * not_dones

    return {"step_kernels_ms": step_kernels, "step_kernels_second_critic_ms": lambda: step_kernels(True), "step_torch_ms": step_torch, "host_read_ms": host_read, "host_read_lists_ms": host_read_lists,
            "record_kernel_ms": lambda: agent._rollout_record(0), "record_torch_ms": record_torch}


def update_forms(agent):
    idx = agent._idx_buf[:agent.minibatch_size].clone()
    d = agent.dataset
    mu0 = (d["old_mu"].index_select(0, idx) + 0.01 * torch.randn((agent.minibatch_size, agent.num_actions), device=DEV)).contiguous()
    v0 = torch.randn(agent.minibatch_size, device=DEV)

    def grads(fused):
        def run():
            agent.fused_loss = fused
            agent.calc_gradients(idx)
        return run

    def head_kernel():
        agent._launch_loss(mu0, v0, idx)

    def head_torch():
        mu, v = mu0.clone().requires_grad_(), v0.clone().requires_grad_()
        loss, _ = CP.ppo_loss_torch(mu, v, d, idx, **agent._loss_kwargs())
        torch.autograd.grad(loss, [mu, v])

    return {"grads_fused_ms": grads(True), "grads_torch_ms": grads(False), "head_kernel_ms": head_kernel, "head_torch_ms": head_torch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=10240)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("ctl_ppo_bench measures on a GPU; there is none here")
    ctl, agent = make(args.envs, args.horizon, args.minibatch)
    out = {}

    def note(k, v, **kw):
        out.setdefault(k, []).append(v)
        print(json.dumps(dict({"figure": k, "value": round(v, 5)}, **kw)), flush=True)

    # (c) whole epochs first: they also leave a dataset and a filled buffer for (a) and (b)
    agent.train_epoch()  # warm-up: code objects, GEMM algorithms
    for r in range(args.epochs):
        for fused in (True, False):
            agent.fused_loss = fused
            e = agent.train_epoch()
            tag = "fused" if fused else "torch"
            note("epoch_play_s_" + tag, e["play_time"], round=r)
            note("epoch_update_s_" + tag, e["update_time"], round=r)
            print(agent.format_epoch_line(e, "ctl_ppo_bench"), flush=True)
    batch = agent.play_steps()
    batch.pop("played_frames")
    agent.prepare_dataset(batch)
    figures = dict(rollout_forms(agent, ctl), **update_forms(agent))
    for r in range(args.rounds):
        for k, fn in figures.items():
            note(k, timed(fn, args.iters, args.warmup), round=r, iters=args.iters)
    med = {k: float(np.median(v)) for k, v in out.items()}
    summary = {"summary": "controller PPO agent, %d envs, horizon %d, minibatch %d, units %s, obs %d, actions %d" % (args.envs, args.horizon, args.minibatch, list(UNITS),
                                                                                                                 agent.obs_dim, agent.num_actions),
               **{k: round(v, 5) for k, v in med.items()}, "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()},
               "step_kernels_over_torch": round(med["step_kernels_ms"] / med["step_torch_ms"], 4), "grads_fused_over_torch": round(med["grads_fused_ms"] / med["grads_torch_ms"], 4),
               "head_kernel_over_torch": round(med["head_kernel_ms"] / med["head_torch_ms"], 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
