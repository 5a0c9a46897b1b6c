"""The controller's PPO agent without a GPU: the numpy statements of the three kernels against torch (float64 autograd for the loss
head's analytic gradients, the reference's torch lines for the rest), the loading rules on synthetic checkpoints bit for bit, the
configuration surface, and the argument refusals of the three entry points (no HIP call is made)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import ctl_ppo_fixture as FX
from vid2player3d_amd import _lib
from vid2player3d_amd import ctl_ppo as CP


def test_policy_head_statement_is_the_torch_lines():
    for clip in (1.5, FX.INF):
        mu, logstd, sigma, noise = FX.head_case(7, 35, 3, clip)
        a, mus, sigmas, nlp, ac = CP.policy_head_reference(mu, logstd, sigma, noise, clip)
        tm, ts, tn, tl = (torch.from_numpy(v) for v in (mu, sigma, noise, logstd))
        ta = tm + ts * tn
        assert np.array_equal(a.view(np.uint32), ta.numpy().view(np.uint32))
        assert np.array_equal(ac.view(np.uint32), torch.clamp(ta, -clip, clip).numpy().view(np.uint32))
        assert np.array_equal(mus.view(np.uint32), mu.view(np.uint32)) and np.array_equal(sigmas, np.tile(sigma, (7, 1)))
        want = 0.5 * (((ta - tm) / ts) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * 35 + tl.sum(-1)
        ok = np.isfinite(want.numpy())
        assert ok.sum() >= 4 and np.allclose(nlp[ok], want.numpy()[ok], rtol=2e-6, atol=0)
        assert np.isnan(nlp[~ok]).all() or not (~ok).any()


def test_rollout_record_statement_is_the_torch_lines():
    obs, rew, reset, term, sub, cur_r, cur_l, acc, sub_acc = FX.record_case(300, 5, 3, "mixed", 11)
    out = CP.rollout_record_reference(obs, rew, reset, term, sub, cur_r, cur_l, acc, sub_acc, clip_obs=2.0)
    t = torch.from_numpy
    cr, cl = t(cur_r) + t(rew), t(cur_l) + 1
    ids = t(reset).nonzero().flatten()
    not_dones = 1.0 - t(reset).float()
    assert torch.equal(t(out["cur_rewards"]), cr * not_dones) and torch.equal(t(out["cur_lengths"]), cl * not_dones)
    assert np.array_equal(out["next_obs_row"].view(np.uint32), torch.clamp(t(obs), -2.0, 2.0).numpy().view(np.uint32))
    assert np.array_equal(out["dones_row"], reset.astype(np.float32)) and np.array_equal(out["terminated"], term.astype(np.float32))
    got = out["acc"] - acc
    assert got[0] == len(ids)
    assert abs(got[1] - cr[ids].double().sum().item()) < 1e-9 and abs(got[2] - cl[ids].double().sum().item()) < 1e-9
    assert abs(got[3] - rew.astype(np.float64).sum()) < 1e-9
    assert np.abs(out["sub_acc"] - sub_acc - sub.astype(np.float64).sum(0)).max() < 1e-9


@pytest.mark.parametrize("bounds,c01", [(None, (32, 35)), (10.0, (32, 35)), (10.0, (7, 7))])
def test_loss_statement_has_autograds_gradients(bounds, c01):
    """`ppo_loss_reference` in float64 against float64 autograd of the torch statement of the head: statistics and both gradients."""
    mu, value, data, idx = FX.loss_case(65, 35, 96, 21)
    kw = dict(e_clip=0.2, critic_coef=5.0, entropy_coef=0.0, bounds_loss_coef=bounds, dof_res_weight=0.01, c0=c01[0], c1=c01[1])
    g_mu, g_v, stats = CP.ppo_loss_reference(mu, value, data, idx, **kw)
    d64 = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in data.items()}
    tm, tv = torch.from_numpy(mu.astype(np.float64)).requires_grad_(), torch.from_numpy(value.astype(np.float64)).requires_grad_()
    loss, tstats = CP.ppo_loss_torch(tm, tv, d64, torch.from_numpy(idx), **kw)
    loss.backward()
    assert np.abs(g_mu - tm.grad.numpy()).max() < 1e-13 * max(1.0, np.abs(g_mu).max())
    assert np.abs(g_v - tv.grad.numpy()).max() < 1e-13
    other = [k for k in range(8) if k != 4]
    assert np.abs(stats - tstats.numpy())[other].max() < 1e-12 * max(1.0, np.abs(stats).max())
    assert abs(stats[4] - tstats[4].item()) <= 2.0 ** -24  # (the reference takes this one mean in float32: `clipped.float()`; a fraction < 1)
    assert (np.abs(mu) > 1).any() and (stats[2] > 0) == (bounds is not None) and (stats[3] > 0) == (c01[0] < c01[1])
    assert 0 < stats[4] < 1


def test_loss_statement_without_idx_reads_the_rows_in_order():
    mu, value, data, idx = FX.loss_case(8, 5, 8, 4)
    idx = np.argsort(idx)  # (a permutation of all rows)
    a = CP.ppo_loss_reference(mu, value, data, idx, bounds_loss_coef=10.0)
    gathered = {k: (v[idx] if len(v) == 8 and k not in ("old_sigma", "logstd", "sigma") else v) for k, v in data.items()}
    b = CP.ppo_loss_reference(mu, value, gathered, None, bounds_loss_coef=10.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ loading rules
def _fresh(obs_dim=FX.OBS_DIM, A=FX.A):
    torch.manual_seed(3)
    net = CP.ControllerNetwork(obs_dim, A, FX.UNITS, -0.69)
    return net, CP.ObsMeanStd(obs_dim, "cpu"), CP.ValueMeanStd("cpu")


def test_load_pretrained_same_size_takes_everything():
    net, rms, vms = _fresh()
    ck = FX.synthetic_checkpoint(FX.OBS_DIM, FX.A)
    CP.load_pretrained(net, rms, vms, ck)
    sd = net.state_dict()
    assert set(sd) == set(ck["model"])
    for k, v in ck["model"].items():
        assert torch.equal(sd[k], v), k
    assert torch.equal(rms.running_mean, ck["running_mean_std"]["running_mean"]) and torch.equal(rms.running_var, ck["running_mean_std"]["running_var"])
    assert rms.count.item() == 321.0 and torch.equal(rms.mean32, rms.running_mean.float())
    assert vms.count.item() == 55.0 and torch.equal(vms.running_var, ck["reward_mean_std"]["running_var"])
    assert "a2c_network.sigma" in ck["model"]  # (the caller's dict is not consumed)


def test_load_pretrained_widens_first_layers_mu_and_statistics():
    net, rms, vms = _fresh()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    w_obs, w_act = FX.OBS_DIM - 4, FX.A - 3
    ck = FX.synthetic_checkpoint(w_obs, w_act)
    CP.load_pretrained(net, rms, vms, ck)
    sd, m = net.state_dict(), ck["model"]
    for part in ("actor_mlp", "critic_mlp"):
        w = sd["a2c_network.%s.0.weight" % part]
        assert torch.equal(w[:, :w_obs], m["a2c_network.%s.0.weight" % part]) and not w[:, w_obs:].any()
        assert torch.equal(sd["a2c_network.%s.0.bias" % part], m["a2c_network.%s.0.bias" % part])
        assert torch.equal(sd["a2c_network.%s.2.weight" % part], m["a2c_network.%s.2.weight" % part])
    assert torch.equal(sd["a2c_network.mu.weight"][:w_act], m["a2c_network.mu.weight"]) and not sd["a2c_network.mu.weight"][w_act:].any()
    assert torch.equal(sd["a2c_network.mu.bias"][:w_act], m["a2c_network.mu.bias"]) and not sd["a2c_network.mu.bias"][w_act:].any()
    assert torch.equal(sd["a2c_network.sigma"], before["a2c_network.sigma"])  # dropped with a widened action
    assert torch.equal(sd["a2c_network.value.weight"], m["a2c_network.value.weight"])
    r = ck["running_mean_std"]
    assert torch.equal(rms.running_mean[:w_obs], r["running_mean"]) and not rms.running_mean[w_obs:].any()
    assert torch.equal(rms.running_var[:w_obs], r["running_var"]) and bool((rms.running_var[w_obs:] == 1).all()) and rms.count.item() == 321.0
    assert torch.equal(rms.var32, rms.running_var.float())


def test_discard_pretrained_sigma_and_refusals_of_narrower_networks():
    net, rms, vms = _fresh()
    sigma = net.sigma.detach().clone()
    ck = FX.synthetic_checkpoint(FX.OBS_DIM, FX.A)
    CP.load_pretrained(net, rms, vms, ck, discard_pretrained_sigma=True)
    assert torch.equal(net.sigma, sigma) and torch.equal(net.state_dict()["a2c_network.mu.weight"], ck["model"]["a2c_network.mu.weight"])
    with pytest.raises(ValueError, match="columns"):
        CP.set_network_weights(net, dict(FX.synthetic_checkpoint(FX.OBS_DIM + 1, FX.A)["model"]))
    with pytest.raises(ValueError, match="actions"):
        CP.set_network_weights(net, dict(FX.synthetic_checkpoint(FX.OBS_DIM, FX.A + 1)["model"]))
    with pytest.raises(ValueError, match="running_mean_std"):
        CP.set_stats_weights(rms, vms, {"reward_mean_std": ck["reward_mean_std"]})


def test_checkpoint_keys_go_both_ways_with_the_actor_of_the_player():
    from vid2player3d_amd import policies as P

    net, _, _ = _fresh()
    actor = P.ActorMLP.from_state_dict(net.state_dict())
    x = torch.randn(5, FX.OBS_DIM)
    with torch.no_grad():
        assert torch.equal(actor(x), net.actor(x))
    with pytest.raises(NotImplementedError, match="use_running_obs"):
        CP.ControllerNetwork(FX.OBS_DIM, FX.A, FX.UNITS, use_running_obs=True)


def test_obs_statistics_update_is_the_running_mean_std_of_the_shim():
    """`ObsMeanStd.update` + the normalisation against rl_games' RunningMeanStd as restated under oracle/ref_shim (training mode)."""
    from oracle.ref_shim.rl_games_restated import RunningMeanStd

    ref, own = RunningMeanStd((FX.OBS_DIM,)), CP.ObsMeanStd(FX.OBS_DIM, "cpu")
    ref.train()
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        x = torch.randn(16, FX.OBS_DIM, generator=g) * 2 + 0.5
        y = ref(x)
        own.update(x)
        assert torch.equal(own.running_mean, ref.running_mean) and torch.equal(own.running_var, ref.running_var) and torch.equal(own.count, ref.count)
        mine = torch.clamp((x - own.mean32) / torch.sqrt(own.var32 + 1e-5), -5.0, 5.0)
        assert torch.equal(mine, y)


# ------------------------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("name", sorted(FX.YAML_PARAMS))
def test_config_accepts_the_single_player_yamls(name):
    kw = CP.config_kwargs(FX.YAML_PARAMS[name])
    cfg = FX.YAML_PARAMS[name]["config"]
    assert kw["minibatch_size"] == 16384 and kw["horizon_length"] == cfg["horizon_length"] and kw["units"] == (1024, 1024, 512)
    assert kw["bounds_loss_coef"] == 10.0 and kw["clip_actions"] == 5.0 and kw["clip_obs"] == math.inf and kw["learning_rate"] == cfg["learning_rate"]
    assert kw["sigma_init"] == FX.YAML_PARAMS[name]["network"]["space"]["continuous"]["sigma_init"]["val"]
    assert kw["discard_pretrained_sigma"] == cfg.get("discard_pretrained_sigma", False) and kw["seed"] == 10


def _with(path, value):
    import copy

    p = copy.deepcopy(FX.YAML_PARAMS["federer"])
    d = p
    for k in path[:-1]:
        d = d.setdefault(k, {})
    d[path[-1]] = value
    return p


@pytest.mark.parametrize("path,value,word", [
    (("config", "multi_gpu"), True, "multi_gpu"), (("config", "mixed_precision"), True, "mixed_precision"), (("config", "clip_value"), True, "clip_value"),
    (("config", "lr_schedule"), "adaptive", "lr_schedule"), (("network", "use_running_obs"), True, "use_running_obs"), (("config", "dual_mode"), "different", "dual_mode"),
    (("network", "name"), "vid2player_dual_v2", "vid2player_dual_v2"), (("network", "space", "continuous", "fixed_sigma"), False, "learned sigma"),
    (("network", "mlp", "activation"), "elu", "activation"), (("config", "normalize_input"), False, "normalize_input"), (("network", "rnn"), {"units": 8}, "rnn"),
    (("network", "separate"), False, "separate"), (("config", "reward_shaper"), {"scale_value": 0.5}, "reward_shaper")])
def test_config_refuses_unbuilt_options_by_name(path, value, word):
    with pytest.raises(NotImplementedError, match=word):
        CP.config_kwargs(_with(path, value))


def test_config_refuses_the_two_player_yamls():
    with pytest.raises(NotImplementedError, match="vid2player_dual"):
        CP.config_kwargs(FX.DUAL_PARAMS)


# ------------------------------------------------------------------------------------------------------------------ the entry points
def test_entry_points_refuse_bad_arguments_without_touching_a_gpu():
    """Argument validation of v2p_ctl_policy_head / v2p_ctl_rollout_record / v2p_ppo_loss happens before any HIP call."""
    L = _lib.load()
    INVALID, null = -1, None
    one = ctypes.c_void_p(16)  # (a non-null placeholder: every call below is refused before anything is dereferenced)
    head = lambda n, A, clip=1.0, mu=one, nlp=one, ac=one: L.v2p_ctl_policy_head(n, A, mu, one, one, one, clip, null, null, null, nlp, ac, null)
    assert head(8, 0) == INVALID and b"num_actions" in L.v2p_last_error()
    assert head(8, 129) == INVALID and head(-1, 35) == INVALID and head(8, 35, clip=0.0) == INVALID and head(8, 35, clip=float("nan")) == INVALID
    assert head(8, 35, mu=null) == INVALID and head(8, 35, nlp=null) == INVALID and head(8, 35, ac=null) == INVALID
    assert b"v2p_ctl_policy_head" in L.v2p_last_error()
    assert head(0, 35, mu=null, nlp=null, ac=null) == 0
    rec = lambda n, dim, S, sub=one, obs=one, acc=one, clip=1.0: L.v2p_ctl_rollout_record(n, dim, S, clip, obs, one, one, one, sub, one, one, one, one, one, one, acc, one, null)
    assert rec(8, 21, 9) == INVALID and b"num_sub" in L.v2p_last_error()
    assert rec(8, 21, -1) == INVALID and rec(-1, 21, 3) == INVALID and rec(8, 0, 3) == INVALID and rec(8, 21, 3, clip=0.0) == INVALID
    assert rec(8, 21, 3, sub=null) == INVALID and rec(8, 21, 3, obs=null) == INVALID and rec(8, 21, 3, acc=null) == INVALID
    assert L.v2p_ctl_rollout_record(0, 21, 3, 1.0, *([null] * 14)) == 0
    cfg = lambda **kw: _lib.PpoLossCfg(**dict(dict(num_actions=35, has_bounds_loss=1, c0=32, c1=35, dataset_rows=64, e_clip=0.2, critic_coef=5.0), **kw))
    full = {k: 16 for k in _lib.PPO_LOSS_BUFFER_NAMES}
    buf = lambda **kw: _lib.PpoLossBuffers(**dict(full, **kw))
    loss = lambda c, B, b: L.v2p_ppo_loss(ctypes.byref(c), B, ctypes.byref(b), null)
    assert loss(cfg(), -1, buf()) == INVALID and b"B" in L.v2p_last_error()
    assert loss(cfg(num_actions=0), 8, buf()) == INVALID and loss(cfg(num_actions=129), 8, buf()) == INVALID
    assert loss(cfg(c0=33, c1=32), 8, buf()) == INVALID and loss(cfg(c1=36), 8, buf()) == INVALID and loss(cfg(c0=-1), 8, buf()) == INVALID
    assert loss(cfg(e_clip=0.0), 8, buf()) == INVALID
    assert loss(cfg(dataset_rows=4), 8, buf(idx=None)) == INVALID
    for k in _lib.PPO_LOSS_BUFFER_NAMES:
        if k != "idx":
            assert loss(cfg(), 8, buf(**{k: None})) == INVALID, k
    assert b"v2p_ppo_loss" in L.v2p_last_error()
    assert L.v2p_ppo_loss(None, 8, ctypes.byref(buf()), null) == INVALID and L.v2p_ppo_loss(ctypes.byref(cfg()), 8, None, null) == INVALID
    assert loss(cfg(), 0, _lib.PpoLossBuffers()) == 0
    assert _lib.PPO_LOSS_PARTIALS == 6 * _lib.PPO_LOSS_MAX_BLOCKS


def test_struct_sizes_of_the_loss_head_match_the_header():
    import os
    import subprocess
    import tempfile

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = '#include <stdio.h>\n#include "v2p_rollout.h"\nint main(void){ printf("%zu %zu %d %d %d\\n", sizeof(v2p_ppo_loss_cfg), sizeof(v2p_ppo_loss_buffers), ' \
           'V2P_PPO_LOSS_PARTIALS, V2P_CTL_MAX_ACTIONS, V2P_CTL_MAX_SUB_REWARDS); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(repo, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(_lib.PpoLossCfg), ctypes.sizeof(_lib.PpoLossBuffers), _lib.PPO_LOSS_PARTIALS, _lib.CTL_MAX_ACTIONS, _lib.CTL_MAX_SUB_REWARDS]


# ------------------------------------------------------------------------------------------------------------------ the reference's epoch
def within(got, g, key, what=None):
    """|got - recorded| <= 8 x the recorded fp32-fp64 scatter of the reference's own result (the project's rule, tests/test_policies.py);
    where the scatter is 0 the comparison is exact"""
    want, scatter = g[key].astype(np.float64), float(g[key + "/scatter"])
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    err = np.abs(got - want).max()
    assert err <= 8 * scatter, "%s: %g > 8 x %g" % (what or key, err, scatter)


def cpu_agent_pieces():
    net = CP.ControllerNetwork(FX.OBS_DIM, FX.A, FX.UNITS, -0.69)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in FX.initial_weights().items()})
    st = FX.initial_statistics()
    rms, vms = CP.ObsMeanStd(FX.OBS_DIM, "cpu"), CP.ValueMeanStd("cpu")
    rms.load_state_dict({"running_mean": st["obs_mean"], "running_var": st["obs_var"], "count": st["obs_count"]})
    vms.running_mean[:], vms.running_var[:] = st["value_mean"], st["value_var"]
    return net, rms, vms


def test_statements_meet_the_rollout_the_reference_recorded():
    """tests/golden/ctl_ppo.npz (tools/gen_golden_ctl_ppo.py: V2PAgent.play_steps itself on the scripted env): the numpy statements of the
    head and of the record, the network through `ControllerNetwork`, GAE - every buffer row, the returns and what the meters received."""
    g = FX.golden()
    net, rms, vms = cpu_agent_pieces()
    ctl = FX.ScriptedController(torch.device("cpu"))
    logstd = FX.initial_weights()["a2c_network.sigma"]
    sigma = np.exp(logstd).astype(np.float32)
    cur_r, cur_l, acc, sub_acc = np.zeros(FX.N, np.float32), np.zeros(FX.N, np.float32), np.zeros(4), np.zeros(FX.S)
    norm = lambda o: torch.clamp((o - rms.mean32) / torch.sqrt(rms.var32 + 1e-5), -5.0, 5.0)
    unnorm = lambda v: vms(v, True)
    rows = {k: [] for k in ("obses", "actions", "mus", "sigmas", "neglogpacs", "values", "next_values", "rewards", "dones", "next_obses")}
    ctl.reset(torch.zeros(0, dtype=torch.long))
    with torch.no_grad():
        for n in range(FX.T):
            obs = torch.clamp(ctl.obs_buf, -FX.CLIP_OBS, FX.CLIP_OBS)
            x = norm(obs)
            a, mus, sigmas, nlp, ac = CP.policy_head_reference(net.actor(x).numpy(), logstd, sigma, g["noise"][n].astype(np.float32), FX.CLIP_ACTIONS)
            rows["values"].append(unnorm(net.critic(x)).numpy().reshape(-1))
            ctl.step(torch.from_numpy(ac))
            out = CP.rollout_record_reference(ctl.obs_buf.numpy(), ctl.rew_buf.numpy(), ctl.reset_buf.numpy(), ctl.extras["terminate"].numpy(), ctl.extras["sub_rewards"].numpy(),
                                              cur_r, cur_l, acc, sub_acc, FX.CLIP_OBS)
            cur_r, cur_l, acc, sub_acc = out["cur_rewards"], out["cur_lengths"], out["acc"], out["sub_acc"]
            nv = unnorm(net.critic(norm(torch.from_numpy(out["next_obs_row"])))).numpy().reshape(-1) * (1.0 - out["terminated"])
            for k, v in (("obses", obs.numpy()), ("actions", a), ("mus", mus), ("sigmas", sigmas), ("neglogpacs", nlp), ("next_values", nv), ("rewards", out["rewards_row"]),
                         ("dones", out["dones_row"]), ("next_obses", out["next_obs_row"])):
                rows[k].append(v)
            ctl.reset(torch.from_numpy(np.nonzero(out["dones_row"])[0]))
    buf = {k: np.stack(v) for k, v in rows.items()}
    for k, v in buf.items():
        within(v, g, "buffer/" + k)
    assert np.array_equal(buf["dones"], g["buffer/dones"]) and np.array_equal(buf["rewards"], g["buffer/rewards"])
    last, advs = np.zeros(FX.N, np.float32), np.zeros((FX.T, FX.N), np.float32)
    for t in reversed(range(FX.T)):  # CommonAgent.discount_values
        delta = buf["rewards"][t] + np.float32(0.99) * buf["next_values"][t] - buf["values"][t]
        last = delta + np.float32(0.99) * np.float32(0.95) * (1 - buf["dones"][t]) * last
        advs[t] = last
    within((advs + buf["values"]).T.reshape(-1), g, "returns")
    assert acc[0] == len(g["meters/game_rewards"]) == 6 and acc[2] == g["meters/game_lengths"].sum()
    assert abs(acc[1] - g["meters/game_rewards"].astype(np.float64).sum()) <= 8 * float(g["meters/game_rewards/scatter"]) * 6  # (a sum of 6 recorded values)
    within(acc[3] / (FX.N * FX.T), g, "meters/step_rewards")
    within(sub_acc / (FX.N * FX.T), g, "meters/step_sub_rewards")


def test_update_meets_the_six_steps_the_reference_recorded():
    """prepare_dataset and calc_gradients from the recorded buffer, on the CPU with the torch statement of the head: the dataset, the
    minibatch order (bit for bit, given the recorded permutations), the loss statistics and every parameter after each of the 6 steps,
    and the numpy statement of the head at the first step."""
    g = FX.golden()
    net, rms, vms = cpu_agent_pieces()
    t = lambda k: torch.from_numpy(g["buffer/" + k]).transpose(0, 1).reshape((FX.N * FX.T,) + g["buffer/" + k].shape[2:])
    values, returns = t("values"), torch.from_numpy(g["returns"])
    adv = returns - values
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    vms.train()
    old_values, norm_returns = vms(values.reshape(-1, 1)).reshape(-1), vms(returns.reshape(-1, 1)).reshape(-1)
    within(adv, g, "dataset/advantages")
    within(old_values, g, "dataset/old_values")
    within(norm_returns, g, "dataset/returns")
    assert np.allclose([vms.running_mean.item(), vms.running_var.item(), vms.count.item()], g["dataset/value_mean_var_count"], rtol=1e-6)
    data = {"old_neglogp": t("neglogpacs"), "advantages": adv, "returns": norm_returns, "actions": t("actions"), "old_mu": t("mus"), "old_sigma": t("sigmas")[0],
            "logstd": net.sigma.detach(), "sigma": torch.exp(net.sigma.detach())}
    obs = t("obses")
    kw = dict(e_clip=0.2, critic_coef=5.0, entropy_coef=0.0, bounds_loss_coef=10.0, dof_res_weight=0.01, c0=32, c1=35)
    opt = torch.optim.Adam(net.parameters(), FX.small_params()["config"]["learning_rate"], eps=1e-08, weight_decay=0.0)
    perms, step = FX.permutations(), 0
    sampler, later = CP.FrameSampler(FX.N * FX.T, FX.MINIBATCH, "cpu"), iter(perms[1:])
    sampler.idx_buf[:] = torch.from_numpy(perms[0])
    net.train()
    for e in range(FX.MINI_EPOCHS):
        for i in range(FX.N * FX.T // FX.MINIBATCH):
            idx = sampler.get(i, lambda: next(later))  # AMPDataset's order: the recorded permutations, reshuffled behind the last minibatch
            assert np.array_equal(idx.numpy(), perms[e][i * FX.MINIBATCH:(i + 1) * FX.MINIBATCH])
            rows = obs[idx]
            rms.update(rows)
            x = torch.clamp((rows - rms.mean32) / torch.sqrt(rms.var32 + 1e-5), -5.0, 5.0)
            mu, value = net.actor(x), net.critic(x)
            loss, stats = CP.ppo_loss_torch(mu, value, data, idx, **kw)
            with torch.no_grad():  # ratios leave the clip on each side, frame for frame as in the reference's run
                nlp = 0.5 * (((data["actions"][idx] - mu) / data["sigma"]) ** 2).sum(-1) + 0.5 * CP.LOG_2PI * FX.A + data["logstd"].sum(-1)
                ratio = torch.exp(data["old_neglogp"][idx] - nlp)
                assert [int((ratio < 0.8).sum()), int((ratio > 1.2).sum())] == g["step%d/clip_sides" % step].tolist()
            if step == 0:
                nd = {k: v.numpy() for k, v in data.items()}
                s32 = CP.ppo_loss_reference(mu.detach().numpy(), value.detach().numpy(), nd, idx.numpy(), dt=np.float32, **kw)[2]
                within(s32[:7], g, "step0/stats", "the numpy statement of the head at step 0")
            for p in net.parameters():
                p.grad = None
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 50.0)
            opt.step()
            within(stats[:7].detach(), g, "step%d/stats" % step)
            for k, p in net.state_dict().items():
                if k != "a2c_network.sigma":
                    within(p, g, "step%d/param/%s" % (step, k))
            step += 1
    assert step == 6
    sides = np.stack([g["step%d/clip_sides" % k] for k in range(6)])
    assert sides[1:, 0].sum() > 0 and sides[1:, 1].sum() > 0
    assert np.allclose(rms.running_mean.numpy(), g["final/obs_mean"], rtol=0, atol=1e-6) and rms.count.item() == g["final/obs_count"][0]


@pytest.mark.parametrize("case", sorted(FX.LOAD_CASES))
def test_loading_rules_meet_what_the_reference_loaded(case):
    """`load_pretrained` against the state the reference's own `V2PAgent.load_pretrained` / `set_network_weights` / `set_stats_weights`
    left behind on the same synthetic checkpoint (tests/golden/ctl_ppo.npz, `load/<case>/...`): every tensor bit for bit."""
    g = FX.golden()
    net, rms, vms = cpu_agent_pieces()
    rms, vms = CP.ObsMeanStd(FX.OBS_DIM, "cpu"), CP.ValueMeanStd("cpu")
    w_obs, w_act, discard = FX.LOAD_CASES[case]
    CP.load_pretrained(net, rms, vms, FX.synthetic_checkpoint(w_obs, w_act), discard_pretrained_sigma=discard)
    sd = net.state_dict()
    keys = [k for k in g if k.startswith("load/%s/model/" % case)]
    assert len(keys) == len(sd) == 13
    for k in keys:
        got, want = sd[k.split("/model/")[1]].numpy(), g[k]
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    for nm, m in (("obs", rms), ("value", vms)):
        assert np.array_equal(m.running_mean.numpy().reshape(-1), g["load/%s/%s_mean" % (case, nm)].reshape(-1)), nm
        assert np.array_equal(m.running_var.numpy().reshape(-1), g["load/%s/%s_var" % (case, nm)].reshape(-1)), nm
        assert m.count.item() == g["load/%s/%s_count" % (case, nm)][0], nm
