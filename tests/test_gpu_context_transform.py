"""The context transform on the MI355X (cfg env.transform_specs; _transform_target, humanoid_smpl_im.py:565-592, fused into
env_context_kernel): the engine's 402-d windows against the numpy restatement (tests/context_transform_ref.py, itself pinned to the
reference's outputs by tests/test_context_transform.py) applied to the same window's clean body_pos_gt block with the draws the task
used, through a whole-batch reset, an env_ids reset and v2p_env_context; the 402-stride network kernels; the draws' seeding and rates;
one PPO epoch and a player rollout with all three ops."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.context_transform_ref import apply_transform, near_threshold
from tests.gpu_util import DEV, N, make_task

pytestmark = pytest.mark.gpu

NENV = 1024
SPECS = json.loads(str(load_golden("context_transform.npz")["specs"]))
ALL3 = {"noisy_joints": {"prob": 0.5, "noise_std": 0.03, "conf_std": 0.03, "min_conf": 0.2}, "mask_random_joints": {"prob": 0.3},
        "mask_joints": {"joints": ["L_Ankle", "Head", "R_Hand"]}}


@pytest.fixture(scope="module")
def mlib():
    from vid2player3d_amd import motion_tables, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    bm = load_baked_model()
    tabs = motion_tables.build_tables(synth.make_clips(13, 16, 90, 200), bm.parents, bm.local_pos)
    return MotionLib(tabs, DEV)


@pytest.fixture(scope="module")
def plain(mlib):
    task = make_task(NENV, mlib)
    yield task
    task.close()


def _task(mlib, specs, n=NENV, **kw):
    return make_task(n, mlib, transform_specs=dict((k, v) for k, v in specs) if isinstance(specs, list) else specs, **kw)


def _check_window(task, plain, specs, what):
    torch.cuda.synchronize()
    ctx, ref = N(task.context_feat), N(plain.context_feat)
    n, w = ctx.shape[:2]
    assert ctx.shape == (n, w, 402) and ref.shape == (n, w, 378)
    # every block but body_pos, and the mask, are the clean window's, bit for bit
    assert np.array_equal(ctx[..., 72:378].view(np.uint32), ref[..., 72:].view(np.uint32)), what
    assert torch.equal(task.context_mask, plain.context_mask), what
    gt = ctx[..., 237:309].reshape(n * w, 24, 3)
    if task._context_draws is None:
        d = np.zeros((n * w, 24, 5), dtype=np.float32)
    else:
        d = N(task._context_draws).reshape(n * w, 24, 5)
    args = (specs, gt, d[..., 0], d[..., 1:4], d[..., 4], task.body_names)
    pos, conf = apply_transform(*args)
    near = near_threshold(*args)
    got_pos, got_conf = ctx[..., :72].reshape(n * w, 24, 3), ctx[..., 378:].reshape(n * w, 24)
    flips = (got_conf == 0) != (conf == 0)
    assert not (flips & ~near).any(), "%s: %d occlusion decisions differ away from min_conf" % (what, int((flips & ~near).sum()))
    ok = ~flips
    assert np.array_equal(got_pos[ok].view(np.uint32), pos[ok].view(np.uint32)), "%s: positions differ" % what
    assert np.abs(got_conf[ok] - conf[ok]).max() <= 1e-6, what
    print("[context transform] %-34s %d bodies, %d within 1e-5 of min_conf, %d occlusion decisions flipped there" %
          (what, conf.size, int(near.sum()), int(flips.sum())))
    return ctx


@pytest.mark.parametrize("key", list(SPECS))
def test_engine_window_equals_the_restatement(mlib, plain, key):
    specs = SPECS[key]
    task = _task(mlib, specs)
    assert task.context_names[-1] == "joint_conf" and task.context_dims[-1] == 24
    rng = np.random.default_rng(3)
    lengths = N(mlib._motion_lengths[task._reset_ref_motion_ids])
    times = torch.tensor((rng.uniform(0.0, 1.0, NENV) * np.maximum(lengths - 1.2, 0.05)).astype(np.float32), device=DEV)
    for t in (task, plain):
        t.reset_with_times(None, times)
    ctx = _check_window(task, plain, specs, key + ": whole-batch reset")
    if key == "empty":  # `transform_specs: {}`: joint_conf all ones, the 378-d frame unchanged
        assert (ctx[..., 378:] == 1.0).all()
        assert np.array_equal(ctx[..., :378].view(np.uint32), N(plain.context_feat).view(np.uint32))
    ids = torch.arange(5, NENV, 3, device=DEV)
    sub = torch.tensor(rng.uniform(0.0, 0.6, ids.shape[0]).astype(np.float32), device=DEV)
    before = N(task.context_feat)
    for t in (task, plain):
        t.reset_with_times(ids, sub)
    ctx = _check_window(task, plain, specs, key + ": env_ids reset")
    keep = np.setdiff1d(np.arange(NENV), N(ids))
    assert np.array_equal(ctx[keep].view(np.uint32), before[keep].view(np.uint32))  # the other envs' windows stay
    later = torch.tensor(rng.uniform(0.0, 0.5, NENV).astype(np.float32), device=DEV)
    for t in (task, plain):
        t._init_context(t._reset_ref_motion_ids, later)
    _check_window(task, plain, specs, key + ": v2p_env_context")
    task.close()


def test_set_context_transform_after_a_reset_is_refused(mlib):
    from vid2player3d_amd import _lib

    task = _task(mlib, SPECS["mask"], n=64)
    task.reset()
    t = _lib.ContextTransform(num_ops=0)
    assert task._lib.v2p_env_set_context_transform(task._h_env, ctypes.byref(t), None) == -1
    assert b"before the first reset" in task._lib.v2p_last_error()
    task.close()


def test_402_stride_network_kernels_equal_the_378_ones():
    from vid2player3d_amd import _lib
    from vid2player3d_amd.learning import ImitationObs

    L = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(1)
    n, w, pad, t = 256, 48, 8, 5
    obs = torch.randn((n, _lib.NUM_OBS), device=DEV, generator=g)
    q = torch.randn((n, w, 24, 4), device=DEV, generator=g)
    ctx = torch.randn((n, w, 402), device=DEV, generator=g)
    ctx[..., 72:168] = (q / q.norm(dim=-1, keepdim=True)).reshape(n, w, 96)
    r = obs[:, 72:168].reshape(n, 24, 4)
    obs[:, 72:168] = (r / r.norm(dim=-1, keepdim=True)).reshape(n, 96)
    ctx378 = ctx[..., :378].contiguous()
    enc = ImitationObs(pad)
    assert torch.equal(enc.rollout(obs, ctx, t), enc.rollout(obs, ctx378, t))
    obs_t = torch.randn((n, 32, _lib.NUM_OBS), device=DEV, generator=g)
    obs_t[..., 72:168] = obs[:, None, 72:168]
    assert torch.equal(enc.training(obs_t, ctx), enc.training(obs_t, ctx378))
    logstd = torch.full((75,), -1.0, device=DEV)
    noise = torch.randn((n, 75), device=DEV, generator=g)
    mu0 = torch.randn((n, 75), device=DEV, generator=g)
    s = _lib.current_stream(DEV)
    outs = []
    for c, dim, new in ((ctx378, 378, False), (ctx378, 378, True), (ctx, 402, True)):
        mu, a, sg, nlp = mu0.clone(), torch.empty_like(mu0), torch.empty_like(mu0), torch.empty(n, device=DEV)
        if new:
            _lib.check(L.v2p_policy_head_w(n, _lib.ptr(mu), _lib.ptr(c), w, dim, pad + t, _lib.ptr(logstd), _lib.ptr(noise), _lib.ptr(a), _lib.ptr(sg),
                                           _lib.ptr(nlp), s), "v2p_policy_head_w")
        else:
            _lib.check(L.v2p_policy_head(n, _lib.ptr(mu), _lib.ptr(c), w, pad + t, _lib.ptr(logstd), _lib.ptr(noise), _lib.ptr(a), _lib.ptr(sg),
                                         _lib.ptr(nlp), s), "v2p_policy_head")
        rows = [torch.empty_like(mu0) for _ in range(3)] + [torch.empty(n, device=DEV)]
        mu_r, a_r = mu0.clone(), torch.empty_like(mu0)
        if new:
            _lib.check(L.v2p_policy_head_record_w(n, _lib.ptr(mu_r), _lib.ptr(c), w, dim, pad + t, _lib.ptr(logstd), _lib.ptr(noise), _lib.ptr(a_r),
                                                  _lib.ptr(rows[2]), _lib.ptr(rows[3]), _lib.ptr(rows[0]), _lib.ptr(rows[1]), s), "v2p_policy_head_record_w")
        else:
            _lib.check(L.v2p_policy_head_record(n, _lib.ptr(mu_r), _lib.ptr(c), w, pad + t, _lib.ptr(logstd), _lib.ptr(noise), _lib.ptr(a_r),
                                                _lib.ptr(rows[2]), _lib.ptr(rows[3]), _lib.ptr(rows[0]), _lib.ptr(rows[1]), s), "v2p_policy_head_record")
        outs.append([mu, a, sg, nlp, mu_r, a_r] + rows)
    for k in (1, 2):
        for x, y in zip(outs[0], outs[k]):
            assert torch.equal(x, y)
    # a width below 378 is refused
    assert L.v2p_policy_head_w(n, _lib.ptr(mu0), _lib.ptr(ctx), w, 377, pad, _lib.ptr(logstd), _lib.ptr(noise), _lib.ptr(a), _lib.ptr(sg),
                               _lib.ptr(nlp), s) == -1


def test_seeding_and_draw_rates(mlib):
    specs = [("noisy_joints", ALL3["noisy_joints"]), ("mask_random_joints", ALL3["mask_random_joints"])]
    task = _task(mlib, specs)

    def window(seed):
        torch.manual_seed(seed)
        task.reset()
        torch.cuda.synchronize()
        return task.context_feat.clone(), task._context_draws.clone()

    a, da = window(11)
    b, _ = window(11)
    c, _ = window(12)
    assert torch.equal(a, b) and not torch.equal(a, c)
    m = da[..., 0].numel()
    for u, p in ((da[..., 0], 0.5), (da[..., 4], 0.3)):
        frac = float((u < p).float().mean())
        assert abs(frac - p) < 5 * np.sqrt(p * (1 - p) / m), (frac, p)
    conf = N(a[..., 378:])
    noised = N(da[..., 0]) < 0.5
    dropped = N(da[..., 4]) < 0.3
    dropped[..., 0] = False
    assert np.array_equal(conf != 1.0, noised | dropped)  # an un-noised body that is not dropped reports exactly 1
    assert (conf[dropped] == 0).all()
    assert abs(float(dropped[..., 1:].mean()) - 0.3) < 5 * np.sqrt(0.21 / dropped[..., 1:].size)
    assert np.isfinite(N(a)).all()
    task.close()


def test_ppo_epoch_and_player_rollout_with_all_three_ops(mlib):
    from vid2player3d_amd import _lib
    from vid2player3d_amd.learning import ImitationObs
    from vid2player3d_amd.player import ImitatorPlayer
    from vid2player3d_amd.ppo import PPOAgent

    n = 128
    task = _task(mlib, ALL3, n=n)
    assert task.context_feat.shape[-1] == 402
    agent = PPOAgent(task, minibatch_envs=64, mini_epochs=1, seed=2, units=(64, 32))
    torch.manual_seed(4)
    batch = agent.play_steps()
    agent.prepare_dataset(batch)
    _lib.check(task._lib.v2p_env_check(task._h_env, task._stream()), "v2p_env_check")
    feat = agent.dataset["feat_raw"]
    assert torch.isfinite(feat).all()
    # the masked joints' targets (mask_joints runs last: positions 0 in every frame) are what the 734-d observation was built from
    ctx = batch["context_feat"]
    masked = [task.body_names.index(j) for j in ALL3["mask_joints"]["joints"]]
    assert (ctx.view(n, -1, 402)[..., :72].view(n, -1, 24, 3)[:, :, masked] == 0).all()
    clean = ctx[..., :378].clone()
    clean[..., :72] = clean[..., 237:309]
    zeroed = clean.clone()
    zeroed.view(n, -1, 378)[..., :72].view(n, -1, 24, 3)[:, :, masked] = 0.0
    pad = task.context_padding
    f_clean = ImitationObs(pad).training(batch["obses"].contiguous(), clean).view(feat.shape)
    f_zero = ImitationObs(pad).training(batch["obses"].contiguous(), zeroed).view(feat.shape)
    for j in masked:
        sl = slice(507 + 3 * j, 510 + 3 * j)
        assert torch.equal(feat[..., sl], f_zero[..., sl])
        assert not torch.equal(feat[..., sl], f_clean[..., sl])
    r = agent.train_epoch()
    assert np.isfinite([r["a_loss"], r["c_loss"], r["kl"]]).all()
    _lib.check(task._lib.v2p_env_check(task._h_env, task._stream()), "v2p_env_check")
    # a 40-step player rollout past the 32-step window: ImitatorPlayer.run's loop (im_player.py:192-311), the window rebuilt and re-drawn
    # at step 32
    player = ImitatorPlayer.from_agent(agent, games_num=1, max_steps=40, log=None)
    obs = player.env_reset()
    for k in range(40):
        t = k % task.context_length
        if k > 0 and t == 0:
            before = task._context_draws.clone()
            task._init_context(task._reset_ref_motion_ids, task._cur_ref_motion_times)
            assert not torch.equal(before, task._context_draws)
        obs["t"] = t
        action = player.get_action(obs, False)
        obs, r, done, _ = player.env_step(action)
        assert torch.isfinite(r).all()
    _lib.check(task._lib.v2p_env_check(task._h_env, task._stream()), "v2p_env_check")
    assert torch.isfinite(task.context_feat).all() and torch.isfinite(task.obs_buf).all()
    task.close()
