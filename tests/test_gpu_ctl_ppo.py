"""The controller's PPO agent on the device: the three kernels of csrc/ctl_ppo.hip against their numpy statements (every tensor between
guard rows), the agent's rollout and update on a scripted env against the epoch the reference's own methods recorded
(tests/golden/ctl_ppo.npz), against the torch statement of `V2PAgent.play_steps` and against the torch statement of the loss head, and
one closed epoch on the racket + ball controller."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import ctl_ppo_fixture as FX
from tests import policies_fixture as PF
from tests.guarded import Guarded
from vid2player3d_amd import _lib
from vid2player3d_amd import ctl_ppo as CP

gpu = pytest.mark.gpu
DEV = PF.DEV
INF = math.inf


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r != %r" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def stream():
    return _lib.current_stream(torch.device(DEV))


# ------------------------------------------------------------------------------------------------------------------ v2p_ctl_policy_head
@gpu
@pytest.mark.parametrize("A", [1, 32, 35, 41, 128])
@pytest.mark.parametrize("n", [1, 3, 33, 65, 130])
def test_policy_head_kernel(n, A):
    L = _lib.load()
    for clip, with_rows in ((1.5, True), (INF, True), (1.5, False)):
        mu, logstd, sigma, noise = FX.head_case(n, A, 100 + n + A, clip)
        g = Guarded(DEV)
        d = {k: g.of(k, v) for k, v in (("mu", mu), ("logstd", logstd), ("sigma", sigma), ("noise", noise))}
        out = {k: g.empty(k, (n, A)) for k in ("actions", "mus", "sigmas", "clamped")}
        nlp = g.empty("neglogp", (n,))
        p = lambda k: _lib.ptr(out[k]) if with_rows else None
        _lib.check(L.v2p_ctl_policy_head(n, A, _lib.ptr(d["mu"]), _lib.ptr(d["logstd"]), _lib.ptr(d["sigma"]), _lib.ptr(d["noise"]), clip, p("actions"), p("mus"),
                                         p("sigmas"), _lib.ptr(nlp), _lib.ptr(out["clamped"]), stream()), "v2p_ctl_policy_head")
        g.check()
        a, mus, sigmas, want_nlp, ac = CP.policy_head_reference(mu, logstd, sigma, noise, clip)
        assert_bits(N(out["clamped"]), ac, "actions_clamped")
        if with_rows:
            assert_bits(N(out["actions"]), a, "actions")
            assert_bits(N(out["mus"]), mus, "mus")
            assert_bits(N(out["sigmas"]), sigmas, "sigmas")
        else:
            assert all(bool(torch.isnan(out[k]).all()) for k in ("actions", "mus", "sigmas"))
        if clip != INF and n * A > 7:
            assert (np.abs(ac) == np.float32(clip)).any()
        # neglogp: the float32 statement sums in the kernel's order; the bound is the fp32-fp64 scatter of the statement on these inputs
        nlp64 = CP.policy_head_reference(mu, logstd, sigma, noise, clip, dt=np.float64)[3]
        ok = np.isfinite(nlp64)
        got = N(nlp)
        assert np.isnan(got[~ok]).all() or np.isinf(got[~ok]).all() or not (~ok).any()
        if ok.any():
            scatter = max(np.abs(want_nlp[ok].astype(np.float64) - nlp64[ok]).max(), np.spacing(np.float32(np.abs(nlp64[ok]).max())))
            assert np.abs(got[ok].astype(np.float64) - nlp64[ok]).max() <= 8 * scatter


# ------------------------------------------------------------------------------------------------------------------ v2p_ctl_rollout_record
@gpu
@pytest.mark.parametrize("S", [0, 1, 3, 8])
@pytest.mark.parametrize("obs_dim", [1, 5, 257])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 130])
def test_rollout_record_kernel(n, obs_dim, S):
    L = _lib.load()
    for flags, clip in (("all", INF), ("none", 2.0), ("mixed", 2.0)):
        obs, rew, reset, term, sub, cur_r, cur_l, acc, sub_acc = FX.record_case(n, obs_dim, S, flags, 7 * n + obs_dim + S)
        want = CP.rollout_record_reference(obs, rew, reset, term, sub if S else None, cur_r, cur_l, acc, sub_acc, clip)
        runs = []
        for _ in range(2):
            g = Guarded(DEV)
            d = {k: g.of(k, v) for k, v in (("obs", obs), ("rew", rew), ("reset", reset), ("terminate", term), ("cur_r", cur_r), ("cur_l", cur_l), ("acc", acc))}
            d["sub"] = g.of("sub", sub) if S else None
            d["sub_acc"] = g.of("sub_acc", sub_acc) if S else None
            o = {"next_obs_row": g.empty("next_obs", (n, obs_dim)), "rewards_row": g.empty("rewards", (n,)), "dones_row": g.empty("dones", (n,)),
                 "terminated": g.empty("terminated", (n,))}
            _lib.check(L.v2p_ctl_rollout_record(n, obs_dim, S, clip, _lib.ptr(d["obs"]), _lib.ptr(d["rew"]), _lib.ptr(d["reset"]), _lib.ptr(d["terminate"]),
                                                _lib.ptr(d["sub"]), _lib.ptr(o["next_obs_row"]), _lib.ptr(o["rewards_row"]), _lib.ptr(o["dones_row"]),
                                                _lib.ptr(o["terminated"]), _lib.ptr(d["cur_r"]), _lib.ptr(d["cur_l"]), _lib.ptr(d["acc"]), _lib.ptr(d["sub_acc"]),
                                                stream()), "v2p_ctl_rollout_record")
            g.check()
            got = {k: N(v) for k, v in o.items()}
            got.update(cur_rewards=N(d["cur_r"]), cur_lengths=N(d["cur_l"]), acc=N(d["acc"]), sub_acc=N(d["sub_acc"]) if S else np.zeros(0))
            runs.append(got)
        for k, v in want.items():
            assert_bits(runs[0][k], v, "%s (%s)" % (k, flags))  # (the float64 accumulators too: exact in the kernel's stated order)
            assert_bits(runs[1][k], runs[0][k], "%s, second run" % k)


@gpu
def test_rollout_record_kernel_more_envs_than_one_pass_of_workgroup_0():
    """n > 256: every thread of workgroup 0 takes more than one env (at 10240 envs, forty)"""
    test_rollout_record_kernel(700, 5, 3)
    test_rollout_record_kernel(1025, 7, 0)


# ------------------------------------------------------------------------------------------------------------------ v2p_ppo_loss
def launch_loss(g, mu, value, data, idx, kw):
    L = _lib.load()
    B, A = mu.shape
    d = {k: g.of(k, v) for k, v in data.items()}
    d.update(mu=g.of("mu", mu), value=g.of("value", value), idx=None if idx is None else g.of("idx", idx))
    out = {"grad_mu": g.empty("grad_mu", (B, A)), "grad_value": g.empty("grad_value", (B,)), "stats": g.empty("stats", (8,), torch.float64),
           "partials": g.empty("partials", (_lib.PPO_LOSS_PARTIALS,), torch.float64)}
    c = _lib.PpoLossCfg(num_actions=A, has_bounds_loss=int(kw["bounds_loss_coef"] is not None), c0=kw["c0"], c1=kw["c1"], dataset_rows=len(data["advantages"]),
                        e_clip=kw["e_clip"], critic_coef=kw["critic_coef"], entropy_coef=kw["entropy_coef"], bounds_loss_coef=kw["bounds_loss_coef"] or 0.0,
                        dof_res_weight=kw["dof_res_weight"])
    p = lambda t: None if t is None else t.data_ptr()
    b = _lib.PpoLossBuffers(mu=p(d["mu"]), value=p(d["value"]), idx=p(d["idx"]), old_neglogp=p(d["old_neglogp"]), advantages=p(d["advantages"]), returns=p(d["returns"]),
                            actions=p(d["actions"]), old_mu=p(d["old_mu"]), old_sigma=p(d["old_sigma"]), logstd=p(d["logstd"]), sigma=p(d["sigma"]),
                            grad_mu=p(out["grad_mu"]), grad_value=p(out["grad_value"]), stats=p(out["stats"]), partials=p(out["partials"]))
    _lib.check(L.v2p_ppo_loss(C.byref(c), B, C.byref(b), stream()), "v2p_ppo_loss")
    g.check()
    return N(out["grad_mu"]), N(out["grad_value"]), N(out["stats"])


def within_scatter(got, want32, want64, what):
    """|kernel - float64 statement| <= 8 x the fp32-fp64 scatter of the statement on these inputs (at least one float32 spacing of the
    largest value: a statement that happens to round like float64 does not make the bound zero)."""
    for k, name in enumerate(("grad_mu", "grad_value", "stats")):
        scatter = max(np.abs(want32[k].astype(np.float64) - want64[k]).max(), float(np.spacing(np.float32(np.abs(want64[k]).max()))))
        err = np.abs(got[k].astype(np.float64) - want64[k]).max()
        assert err <= 8 * scatter, "%s %s: %g > 8 x %g" % (what, name, err, scatter)


@gpu
@pytest.mark.parametrize("A", [1, 32, 35, 41])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257, 1031])
def test_ppo_loss_kernel(B, A):
    for with_idx, bounds, cols in ((True, 10.0, (min(32, A - 1), A)), (False, None, (0, min(3, A))), (True, None, (A, A))):
        rows = B + 37 if with_idx else B
        mu, value, data, idx = FX.loss_case(B, A, rows, 1000 + B + A)
        if not with_idx:  # identity: the dataset's first B rows in the minibatch's order
            data = {k: (v[idx] if v.shape[0] == rows and k not in ("old_sigma", "logstd", "sigma") else v) for k, v in data.items()}
            idx = None
        kw = dict(e_clip=0.2, critic_coef=5.0, entropy_coef=0.0, bounds_loss_coef=bounds, dof_res_weight=0.01, c0=cols[0], c1=cols[1])
        got = launch_loss(Guarded(DEV), mu, value, data, idx, kw)
        again = launch_loss(Guarded(DEV), mu, value, data, idx, kw)
        for a, b, name in zip(got, again, ("grad_mu", "grad_value", "stats")):
            assert_bits(b, a, "%s, second run" % name)
        want32 = CP.ppo_loss_reference(mu, value, data, idx, dt=np.float32, **kw)
        want64 = CP.ppo_loss_reference(mu, value, data, idx, dt=np.float64, **kw)
        within_scatter(got, want32, want64, "B %d A %d idx %s bounds %s" % (B, A, with_idx, bounds))
        assert np.isfinite(got[2]).all() and (got[2][2] > 0) == (bounds is not None and bool((np.abs(mu) > 1).any()))
        assert (got[2][3] > 0) == (cols[0] < cols[1])


@gpu
def test_ppo_loss_kernel_more_rows_than_one_pass_of_the_grid():
    """B > 4 x V2P_PPO_LOSS_MAX_BLOCKS: the grid is capped and every wave strides over several rows (a minibatch of 16384 takes four)"""
    assert 4 * _lib.PPO_LOSS_MAX_BLOCKS < 4133
    test_ppo_loss_kernel(4133, 35)
    test_ppo_loss_kernel(9001, 3)


@gpu
def test_ppo_loss_kernel_marks_rows_outside_the_dataset():
    mu, value, data, idx = FX.loss_case(9, 5, 20, 3)
    idx = idx.copy()
    idx[4], idx[7] = 20, -1
    kw = dict(e_clip=0.2, critic_coef=5.0, entropy_coef=0.0, bounds_loss_coef=10.0, dof_res_weight=0.0, c0=0, c1=0)
    g_mu, g_v, stats = launch_loss(Guarded(DEV), mu, value, data, idx, kw)
    bad = np.array([k in (4, 7) for k in range(9)])
    assert np.isnan(g_mu[bad]).all() and np.isfinite(g_mu[~bad]).all() and np.isnan(g_v[bad]).all() and np.isfinite(g_v[~bad]).all() and np.isnan(stats[:6]).all()


# ------------------------------------------------------------------------------------------------------------------ the agent, scripted env
def scripted_agent(**kw):
    """The fixture's agent on the scripted env: the seeded weights, statistics, permutations and the noise the reference's run drew
    (tests/golden/ctl_ppo.npz)."""
    ctl = FX.ScriptedController(torch.device(DEV))
    agent = CP.ControllerPPOAgent.from_config(ctl, FX.small_params(), clip_obs=FX.CLIP_OBS, clip_actions=FX.CLIP_ACTIONS, **kw)
    agent.noise = torch.from_numpy(FX.golden()["noise"].astype(np.float32)).to(DEV)
    agent.noise_fn = lambda n: agent.noise[n]
    perms = FX.permutations()
    agent._idx_buf[:] = torch.from_numpy(perms[0]).to(DEV)
    it = iter(perms[1:])
    agent.perm_fn = lambda: next(it)
    agent.model.load_state_dict({k: torch.from_numpy(v) for k, v in FX.initial_weights().items()})
    st = FX.initial_statistics()
    agent.running_mean_std.load_state_dict({"running_mean": st["obs_mean"], "running_var": st["obs_var"], "count": st["obs_count"]})
    agent.value_mean_std.running_mean[:], agent.value_mean_std.running_var[:] = st["value_mean"], st["value_var"]
    return agent, ctl, perms


def within(got, g, key):
    """|got - recorded| <= 8 x the recorded fp32-fp64 scatter of the reference's own result; exact where the scatter is 0"""
    want, scatter = g[key].astype(np.float64), float(g[key + "/scatter"])
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    err = np.abs(got - want).max()
    assert err <= 8 * scatter, "%s: %g > 8 x %g" % (key, err, scatter)


@gpu
@pytest.mark.parametrize("fused", [True, False])
def test_agent_meets_the_epoch_the_reference_recorded(fused):
    """The agent with the kernels in the path against tests/golden/ctl_ppo.npz (V2PAgent.play_steps / prepare_dataset / calc_gradients
    themselves on the scripted env): every buffer row, returns, the dataset, the loss statistics and every parameter after each of the
    6 optimiser steps, within 8 x the recorded scatter; the minibatch order bit for bit."""
    g = FX.golden()
    agent, ctl, perms = scripted_agent(fused_loss=fused)
    batch = agent.play_steps()
    for k, v in agent.tensor_dict.items():
        within(N(v), g, "buffer/" + k)
    within(N(batch["returns"]), g, "returns")
    acc = N(agent.acc)
    assert acc[0] == len(g["meters/game_rewards"]) and acc[2] == g["meters/game_lengths"].sum()
    within(acc[3] / (FX.N * FX.T), g, "meters/step_rewards")
    within(N(agent.sub_acc) / (FX.N * FX.T), g, "meters/step_sub_rewards")
    batch.pop("played_frames")
    agent.set_train()
    d = agent.prepare_dataset(batch)
    for k, name in (("old_values", "old_values"), ("old_logp_actions", "old_neglogp"), ("advantages", "advantages"), ("returns", "returns")):
        within(N(d[name]), g, "dataset/" + k)
    step = 0
    for e in range(FX.MINI_EPOCHS):
        for i in range(agent.num_minibatches):
            idx = agent._get_item(i)
            assert np.array_equal(N(idx), perms[e][i * FX.MINIBATCH:(i + 1) * FX.MINIBATCH])
            stats = agent.calc_gradients(idx)
            within(N(stats)[:7], g, "step%d/stats" % step)
            for k, p in agent.model.state_dict().items():
                if k != "a2c_network.sigma":
                    within(N(p), g, "step%d/param/%s" % (step, k))
            step += 1
    assert step == 6 and agent.running_mean_std.count.item() == g["final/obs_count"][0]
    assert np.allclose(N(agent.running_mean_std.running_mean), g["final/obs_mean"], rtol=0, atol=1e-6)


@gpu
def test_agent_rollout_is_the_reference_statement():
    """play_steps with the kernels in the path (the critic once per step, once more where the reset rewrote a row) against the torch statement of V2PAgent.play_steps (two full
    critic passes, torch bookkeeping) on the same scripted env: every buffer row, the returns, the meters."""
    agent, ctl, _ = scripted_agent()
    batch = agent.play_steps()
    ref_agent, ref_ctl, _ = scripted_agent()
    td, returns, meters = FX.play_steps_statement(ref_agent, ref_ctl, ref_agent.noise)
    for a, b in zip(ctl.seen_actions, ref_ctl.seen_actions):
        assert torch.equal(a, b)
    assert bool((torch.stack(ctl.seen_actions).abs() == FX.CLIP_ACTIONS).any())
    for k in ("obses", "next_obses", "rewards", "dones", "actions", "mus", "sigmas"):
        assert_bits(N(agent.tensor_dict[k]), N(td[k]), k)
    # (values: the same GEMMs on the same rows; neglogp: the kernel's sum order against torch's)
    for k in ("values", "next_values"):
        assert_bits(N(agent.tensor_dict[k]), N(td[k]), k)
    assert torch.allclose(agent.tensor_dict["neglogpacs"], td["neglogpacs"], rtol=4e-6, atol=0)
    assert torch.allclose(batch["returns"].view(FX.N, FX.T), returns.transpose(0, 1), rtol=0, atol=1e-6)
    assert torch.equal(batch["obses"].view(FX.N, FX.T, -1), td["obses"].transpose(0, 1))
    acc = N(agent.acc)
    assert acc[0] == len(meters["game_rewards"]) == 6
    assert abs(acc[1] - meters["game_rewards"].double().sum().item()) < 1e-5 and acc[2] == meters["game_lengths"].double().sum().item()
    assert abs(acc[3] / (FX.N * FX.T) - meters["step_rewards"].item()) < 1e-6
    assert np.abs(N(agent.sub_acc) / (FX.N * FX.T) - N(meters["step_sub_rewards"])).max() < 1e-6
    # next_values is masked by terminate alone; values of a reset env are values of the NEW observation
    term = N(ctl.term_script[:FX.T]).astype(bool)
    assert (N(agent.tensor_dict["next_values"])[term] == 0).all() and (N(agent.tensor_dict["next_values"])[~term] != 0).all()


@gpu
def test_agent_critic_once_plus_reset_rows_equals_two_passes():
    a1, _, _ = scripted_agent(reuse_next_values=True)
    a2, _, _ = scripted_agent(reuse_next_values=False)
    a1.play_steps()
    a2.play_steps()
    for k in a1.tensor_dict:
        assert_bits(N(a1.tensor_dict[k]), N(a2.tensor_dict[k]), k)


@gpu
def test_agent_update_fused_loss_against_the_torch_statement():
    """Two agents on the same rollout, fused_loss on and off: the same minibatch order (bit for bit, given the recorded permutations), the
    parameter gradients of both forms within 8 x the fp32-fp64 scatter of the statement's head gradients carried through the same
    layers, the loss statistics of every step, and the parameters after each of the 6 optimiser steps.  (Adam divides a gradient by its
    own size: where a gradient is as small as its rounding error the two forms may step in opposite directions, so the only bound that
    holds for EVERY parameter is Adam's own step bound, lr (1 - beta1) / sqrt(1 - beta2) per step and form.)"""
    agents = [scripted_agent(fused_loss=f) for f in (True, False)]
    order = []
    for agent, ctl, perms in agents:
        batch = agent.play_steps()
        batch.pop("played_frames")
        agent.prepare_dataset(batch)
    for k, v in agents[0][0].dataset.items():
        assert torch.equal(v, agents[1][0].dataset[k]), k
    lr = agents[0][0].last_lr
    steps, clip_fracs = 0, []
    for _ in range(FX.MINI_EPOCHS):
        for i in range(agents[0][0].num_minibatches):
            idx = [a._get_item(i) for a, _, _ in agents]
            assert torch.equal(idx[0], idx[1]) and np.array_equal(N(idx[0]), agents[0][2][steps // 3][(steps % 3) * FX.MINIBATCH:(steps % 3 + 1) * FX.MINIBATCH])
            if steps == 0:  # the parameter gradients of the two forms of the head, before anything has moved
                grads, carried = [], []
                for a, _, _ in agents:
                    a.set_train()
                    obs = a.dataset["obs"].index_select(0, idx[0])
                    x = a._policy_input(obs, torch.empty_like(obs))
                    mu, value = a.model.actor(x), a.model.critic(x)
                    torch.exp(a.model.sigma, out=a.sigma_exp)
                    loss = CP._PpoLossFn.apply(mu, value, a, idx[0]) if a.fused_loss else CP.ppo_loss_torch(mu, value, a.dataset, idx[0], **a._loss_kwargs())[0]
                    ps = [p for p in a.model.parameters() if p.requires_grad]
                    flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).double()
                    grads.append(flat(torch.autograd.grad(loss, ps, retain_graph=True)))
                    if not carried:  # the statement's head gradients, float32 and float64, carried through the same layers
                        data = {k: N(a.dataset[k]) for k in ("actions", "old_mu", "old_sigma", "logstd", "sigma", "advantages", "returns", "old_neglogp")}
                        for dt in (np.float32, np.float64):
                            g_mu, g_v, _ = CP.ppo_loss_reference(N(mu), N(value).reshape(-1), data, N(idx[0]), dt=dt, **a._loss_kwargs())
                            outs = [torch.from_numpy(g_mu.astype(np.float32)).to(DEV), torch.from_numpy(g_v.astype(np.float32)).to(DEV).view_as(value)]
                            carried.append(flat(torch.autograd.grad([mu, value], ps, outs, retain_graph=True)))
                scatter = max((carried[0] - carried[1]).abs().max().item(), float(np.spacing(np.float32(carried[1].abs().max().item()))))
                for gr, name in zip(grads, ("fused", "torch")):
                    assert (gr - carried[1]).abs().max().item() <= 8 * scatter, name
            stats = [a.calc_gradients(ix) for (a, _, _), ix in zip(agents, idx)]
            steps += 1
            s0, s1 = N(stats[0]), N(stats[1])
            assert np.isfinite(s0).all() and np.abs(s0 - s1).max() <= 1e-4 * max(1.0, np.abs(s1).max())
            assert s0[2] > 0 and s0[3] > 0  # the bound loss binds, the residual-DoF means are not zero
            clip_fracs.append(s0[4])
            for p, q in zip(agents[0][0].model.parameters(), agents[1][0].model.parameters()):
                assert (p - q).abs().max().item() <= 2 * lr * steps * 0.1 / math.sqrt(0.001)
    assert steps == 6
    # after the first minibatch ratios leave the clip, and not all of them
    assert max(clip_fracs[1:]) > 0 and min(clip_fracs) < 1
    assert all(torch.equal(a.running_mean_std.running_mean, agents[1][0].running_mean_std.running_mean) for a, _, _ in agents)
    assert agents[0][0].running_mean_std.count.item() == 50.0 + 6 * FX.MINIBATCH


@gpu
def test_agent_train_prints_the_reference_line_and_checkpoints_round_trip(tmp_path):
    agent, ctl, _ = scripted_agent()
    agent.noise_fn = agent.perm_fn = None
    ctl.done_script, ctl.term_script = ctl.done_script.repeat(2, 1), ctl.term_script.repeat(2, 1)
    lines = []
    r = agent.train(max_epochs=2, log=lines.append, network_path=str(tmp_path))
    assert len(lines) == 2 and lines[0].startswith("1\tT_play ") and lines[1].startswith("2\tT_play ")
    for word in ("T_update", "ETA", "step_rewards", "eps_len", "fps step", "fps total"):
        assert word in lines[1]
    assert agent.epoch_num == 2 and agent.frame == 2 * FX.N * FX.T and math.isfinite(r["loss"])
    other, _, _ = scripted_agent()
    other.restore(str(tmp_path / "tennis_v1_latest.pth"))
    for (k, a), b in zip(agent.model.state_dict().items(), other.model.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(other.running_mean_std.running_var, agent.running_mean_std.running_var) and other.epoch_num == 2
    assert torch.equal(other.value_mean_std.running_mean, agent.value_mean_std.running_mean)


# ------------------------------------------------------------------------------------------------------------------ the real controller
@gpu
def test_critic_reuse_equals_two_passes_on_the_racket_ball_controller():
    """16 steps on the racket + ball controller, in which reaction / recovery flags fire for envs that are not done (their observation is
    rewritten by the reset: a new ball, a new target): the default rollout and the reference's two full passes fill the buffer alike,
    bit for bit - `mus`, `actions`, `neglogpacs` and `values` of the step after such a reset come from the new observation."""
    from vid2player3d_amd import policies as P

    n, runs = 64, []
    for reuse in (True, False):
        ctl, task, player, target = PF.single_controller(n)
        ctl.attach_low_level_policy(P.LowLevelPolicy(target, PF.random_actors(1, 734, 75)[0], PF.random_norms(1, 734)[0], 5.0, 1.0))
        params = FX.small_params()
        params["config"].update(horizon_length=16, minibatch_size=16 * n, mini_epochs=1)
        agent = CP.ControllerPPOAgent.from_config(ctl, params, reuse_next_values=reuse)
        seen, lists = [], agent._reset_lists

        def watched(dones_row, seen=seen, lists=lists):
            done_ids, changed_ids = lists(dones_row)
            seen.append((done_ids.numel(), changed_ids.numel()))
            return done_ids, changed_ids

        agent._reset_lists = watched
        agent.play_steps()
        runs.append(({k: N(v) for k, v in agent.tensor_dict.items()}, seen))
    (a, seen), (b, _) = runs
    assert sum(c - d for d, c in seen[:-1]) > 0, "no reaction / recovery flag fired for an env that was not done: %s" % seen
    rewritten = (a["obses"][1:] != a["next_obses"][:-1]).any(-1) & (a["dones"][:-1] == 0)
    assert rewritten.any()  # the reset rewrote the observation of envs that were not done
    for k in a:
        assert np.isfinite(a[k]).all(), k
        assert_bits(a[k], b[k], k)


# ------------------------------------------------------------------------------------------------------------------ one closed epoch
@gpu
def test_one_closed_epoch_on_the_racket_ball_controller():
    from vid2player3d_amd import policies as P

    n = 64
    ctl, task, player, target = PF.single_controller(n)
    ll = P.LowLevelPolicy(target, PF.random_actors(1, 734, 75)[0], PF.random_norms(1, 734)[0], 5.0, 1.0)
    ctl.attach_low_level_policy(ll)
    params = FX.small_params()
    params["config"].update(horizon_length=4, minibatch_size=4 * n, mini_epochs=1)
    agent = CP.ControllerPPOAgent.from_config(ctl, params)
    assert agent.num_actions == 38 and agent.res_cols == (32, 35) and agent.dof_res_weight == 0.0 and agent.S == ctl._sub_rewards.shape[1]
    # the buffer between guard rows, pre-filled with NaN
    g = Guarded(DEV)
    for k, v in list(agent.tensor_dict.items()):
        agent.tensor_dict[k] = g.empty(k, tuple(v.shape))
    r = agent.train_epoch()
    g.check()
    for k, v in agent.tensor_dict.items():
        assert bool(torch.isfinite(v).all()), k
    for k in CP.STAT_NAMES + ("step_rewards", "mean_lengths", "play_time", "update_time"):
        assert math.isfinite(r[k]), k
    assert r["frames"] == 4 * n and agent.epoch_num == 1
    if hasattr(task, "check"):
        task.check()
    # the trained controller plays through the existing path: the policy's action is the agent's eval-mode mu, clamped
    pol = agent.policy()
    mu = pol.act()
    agent.set_eval()
    want = torch.clamp(agent.get_action_values(torch.clamp(ctl.obs_buf, -agent.clip_obs, agent.clip_obs))["mus"], -agent.clip_actions, agent.clip_actions)
    assert_bits(N(mu), N(want), "policy().act() against the agent's mu")
    with pytest.raises(ValueError, match="multiple"):
        CP.ControllerPPOAgent.from_config(ctl, FX.small_params(), minibatch_size=7)
