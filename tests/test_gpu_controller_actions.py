"""GPU checks of `v2p_controller_actions` (csrc/controller_actions.hip): the action part of the controller's pre_physics_step with
`random_walk_in_recovery`, between the guard rows of tests/guarded.py, against `controller_actions_reference` fed the words of
`device_rng.philox_words`; the independence of an env's draws from the rest of the launch; and `TennisControllerTask` /
`DualTennisControllerTask` running a shipped config's values (`random_walk_in_recovery: True`, `vae_action_scale: 1.5`,
`add_residual_dof: euler`, `residual_dof_scale: 0.4`) through `attach_motion_generator` and `pre_physics_step`.

The tolerance of the drawn latents is 8 x max |statement float32 - statement float64| over the test's own draws (printed; the float32
statement rounds the angle 2 pi u2 to float32 as the kernel does, the float64 one does not: an absolute error of up to |z| 2^-23, which
is what the scatter measures).  Everything else - copies, the scaled columns, the clamp at +-clamp - is exact."""
import numpy as np
import pytest
import torch

from tests.guarded import Guarded
from vid2player3d_amd import device_rng as R
from vid2player3d_amd.tasks import tennis_controller as tc

gpu = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EEDC0FFEE123457
UNUSED = 3  # columns behind the row's width that the kernel must not read as its own
WIDTHS = ((0, 0), (3, 0), (3, 3))  # action widths 32, 35, 38
f32, i64 = torch.float32, torch.int64


def settings(nr, nroot, walk=True, clamp=5.0):
    return tc.action_settings(num_res_dof=nr, num_res_root=nroot, vae_action_scale=1.5, residual_dof_scale=0.4, residual_root_scale=0.02, random_walk=walk, clamp=clamp,
                              seed=SEED)


def inputs(n, st, seed=0):
    rng = np.random.default_rng(100 * n + seed)
    actions = rng.normal(0, 1, (n, tc.action_width(st) + UNUSED)).astype(np.float32)
    tar_action = rng.integers(0, 2, n).astype(np.int64)
    tar_action[0] = 0  # (n = 1: the env walks)
    if n > 2:
        tar_action[1], tar_action[n - 1] = 1, 0
    return actions, tar_action


def run(st, n, actions, tar_action, call, words=None):
    """one launch between guards; returns the four outputs as arrays.  Inputs must come back with their bits."""
    G = Guarded(DEV)
    a, t = G.of("actions", actions), G.of("tar_action", tar_action)
    w = None if words is None else G.of("words", words.view(np.int32), dtype=torch.int32)
    out = dict(actions_out=G.empty("actions_out", (n, tc.action_width(st))), mvae_actions=G.empty("mvae_actions", (n, 32)),
               res_dof_actions=G.empty("res_dof_actions", (n, st["num_res_dof"])), res_root_actions=G.empty("res_root_actions", (n, st["num_res_root"])))
    tc.launch_actions(st, n, a, t, out, call=call, words=w)
    G.check()
    assert np.array_equal(a.cpu().numpy(), actions) and np.array_equal(t.cpu().numpy(), tar_action), "the launch wrote an input"
    if w is not None:
        assert np.array_equal(w.cpu().numpy().view(np.uint32), words)
    # torch's own lines on the same device tensors: the scaled columns must be these bits
    nr, nroot = st["num_res_dof"], st["num_res_root"]
    torch_lines = dict(mvae_actions=a[:, :32].clone() * st["vae_action_scale"], res_dof_actions=a[:, 32:32 + nr].clone() * st["residual_dof_scale"],
                       res_root_actions=a[:, 32 + nr:32 + nr + nroot].clone() * st["residual_root_scale"])
    return {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in torch_lines.items()}


def compare(st, got, torch_lines, actions, tar_action, words, what):
    want = tc.controller_actions_reference(st, actions, tar_action, words)
    want64 = tc.controller_actions_reference(st, actions, tar_action, words, dt=np.float64)
    walk = (tar_action == 0) if st["random_walk"] else np.zeros(len(tar_action), bool)
    for k in ("actions_out", "res_dof_actions", "res_root_actions"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs from the statement" % (what, k)
    for k in ("res_dof_actions", "res_root_actions"):
        assert np.array_equal(got[k], torch_lines[k]), "%s: %s is not torch's product" % (what, k)
    z = got["mvae_actions"]
    assert np.array_equal(z[~walk], torch_lines["mvae_actions"][~walk]), "%s: a latent outside recovery is not torch's actions[:, :32] * scale" % what
    assert np.array_equal(z[~walk], want["mvae_actions"][~walk])
    if not walk.any():
        return 0.0
    scatter = float(np.abs(want["mvae_actions"][walk].astype(np.float64) - want64["mvae_actions"][walk]).max())
    err = float(np.abs(z[walk].astype(np.float64) - want64["mvae_actions"][walk]).max())
    err32 = float(np.abs(z[walk] - want["mvae_actions"][walk]).max())
    print("%s: %d drawn latents, scatter |f32 - f64| %.3e, kernel against f64 %.3e, against f32 %.3e" % (what, int(walk.sum()) * 32, scatter, err, err32))
    assert scatter > 0 and err <= 8 * scatter and err32 <= 8 * scatter, what
    c = np.float32(st["clamp"])
    free = R.normals(words[walk], np.float64)  # (before the clamp, in double: away from the bound the kernel's side of it is not in doubt)
    assert (z[walk][free > c + 1e-5] == c).all() and (z[walk][free < -c - 1e-5] == -c).all(), "%s: the clamp is not exact" % what
    assert np.abs(z[walk]).max() <= c
    assert not np.array_equal(z[walk], torch_lines["mvae_actions"][walk]), "%s: the scale reached the walk" % what
    return scatter


@gpu
@pytest.mark.parametrize("n", [1, 3, 65, 130])
@pytest.mark.parametrize("width", WIDTHS)
def test_kernel_against_the_statement(width, n):
    st = settings(*width)
    actions, tar_action = inputs(n, st)
    what = "%d envs, width %d" % (n, tc.action_width(st))
    # ---- the generator's own words: the statement is fed philox_words
    call = 3 + n
    got, lines = run(st, n, actions, tar_action, call)
    compare(st, got, lines, actions, tar_action, R.philox_words(SEED, call, R.STREAM_WALK, n, 8), what + ", generator")
    # ---- words supplied: every edge of the pair law in the rows that walk (the largest normal, r = 0, a quarter turn)
    words = np.random.default_rng(n).integers(0, 2 ** 32, (n, 32), dtype=np.uint64).astype(np.uint32)
    words[0, :8] = [0, 0, 0xFFFFFFFF, 0, 0, 0x40000000, 255, 0xFFFFFFFF]
    got, lines = run(st, n, actions, tar_action, call, words)
    compare(st, got, lines, actions, tar_action, words, what + ", words given")
    assert got["mvae_actions"][0, 0] == 5.0 and got["mvae_actions"][0, 5] == 5.0 and (got["mvae_actions"][0, 2:4] == 0).all(), "the largest normal is clamped, r = 0 gives 0"
    # ---- the clamp at 1: reached on both sides by the generator's draws
    st1 = settings(*width, clamp=1.0)
    got, lines = run(st1, n, actions, tar_action, call)
    compare(st1, got, lines, actions, tar_action, R.philox_words(SEED, call, R.STREAM_WALK, n, 8), what + ", clamp 1")
    assert (got["mvae_actions"] == 1.0).any() and (got["mvae_actions"] == -1.0).any()
    # ---- without the walk, and with every env or no env in recovery
    st0 = settings(*width, walk=False)
    got, lines = run(st0, n, actions, tar_action, call)
    compare(st0, got, lines, actions, tar_action, None, what + ", no walk")
    for flags in (np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 2, np.int64)):
        got, lines = run(st, n, actions, flags, call)
        compare(st, got, lines, actions, flags, R.philox_words(SEED, call, R.STREAM_WALK, n, 8), what + ", every tar_action %d" % flags[0])


@gpu
def test_an_envs_draws_are_its_own():
    st = settings(3, 3)
    a130, t130 = inputs(130, st)
    big, _ = run(st, 130, a130, np.zeros(130, np.int64), 9)
    small, _ = run(st, 65, a130[:65], np.zeros(65, np.int64), 9)
    assert np.array_equal(big["mvae_actions"][:65], small["mvae_actions"]), "rows 0..64 of 130 envs and of 65 envs differ"
    # flipping another env's flag leaves an env's draws alone
    flags = np.zeros(130, np.int64)
    flags[0::2] = 1
    other, lines = run(st, 130, a130, flags, 9)
    assert np.array_equal(other["mvae_actions"][1::2], big["mvae_actions"][1::2])
    assert np.array_equal(other["mvae_actions"][0::2], lines["mvae_actions"][0::2])
    # the next call, and another seed, change them
    nxt, _ = run(st, 130, a130, np.zeros(130, np.int64), 10)
    assert not (nxt["mvae_actions"] == big["mvae_actions"]).all(1).any()
    reseeded, _ = run(dict(st, seed=SEED + 1), 130, a130, np.zeros(130, np.int64), 9)
    assert not (reseeded["mvae_actions"] == big["mvae_actions"]).all(1).any()
    # the draws look like what they are: 130 x 32 clamped normals
    z = big["mvae_actions"].astype(np.float64)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs((z * z).mean() - 1) < 5 * np.sqrt(2 / z.size)


# ------------------------------------------------------------------------------------------------------------------ the controller
SHIPPED = {"random_walk_in_recovery": True, "vae_action_scale": 1.5, "add_residual_dof": "euler", "residual_dof_scale": 0.4}  # cfg/controller/federer_train_stage_*.yaml


def walk_step(ctl, player, gen_ref, actions, call, what, scatter, judge):
    """one pre_physics_step of `ctl`: its four action tensors against the statement of (seed, call), then the generator's state
    against its numpy statement stepped with the STATEMENT's latents; returns how many rows were judged."""
    n = ctl.num_envs
    tar_action = ctl._tar_action.cpu().numpy().copy()
    before = player.state_arrays()
    assert ctl._walk_calls == call
    ctl.pre_physics_step(actions)
    torch.cuda.synchronize()
    assert ctl._walk_calls == call + 1
    st = ctl.action_settings()
    a = actions.cpu().numpy()
    words = R.philox_words(ctl.seed, call, R.STREAM_WALK, n, 8)
    got = dict(actions_out=ctl._actions, mvae_actions=ctl._mvae_actions, res_dof_actions=ctl._res_dof_actions,
               res_root_actions=torch.zeros((n, 0)) if ctl._res_root_actions is None else ctl._res_root_actions)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    lines = dict(mvae_actions=a[:, :32] * np.float32(1.5), res_dof_actions=a[:, 32:35] * np.float32(0.4), res_root_actions=got["res_root_actions"])
    compare(st, got, lines, a, tar_action, words, what)
    want = tc.controller_actions_reference(st, a, tar_action, words)
    rows = judge(gen_ref(before, want["mvae_actions"], want["res_dof_actions"], np.float32), gen_ref(before, want["mvae_actions"], want["res_dof_actions"], np.float64), before,
                 want["mvae_actions"], want["res_dof_actions"])
    return rows, int((tar_action == 0).sum())


@gpu
def test_controller_runs_a_shipped_config():
    """8 envs, racket + ball, generator and target attached: on the parent `attach_motion_generator` raised NotImplementedError."""
    from tests import mvae_fixture as MF
    from tests import mvae_target_fixture as FX
    from tests import tennis_fixture as F
    from tests.gpu_util import synth_tables
    from vid2player3d_amd import ball_traj, mvae
    from vid2player3d_amd import mvae_target as mt
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    n, steps = 8, 4
    torch.manual_seed(7)
    tg, g, mg = F.golden(), FX.golden(), MF.golden()
    gen = ball_traj.TennisBallGenerator({"num_samples": 500}, device=DEV, seed=3)
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = dict(SHIPPED, ball_generator=gen, restitution=1.4, ball_friction=0.2, spin_scale=5, reward_type="return_w_estimate",
                      reward_weights={"pos": 0.5, "ball_pos": 0.5}, court_min=[-30.0, -30.0], court_max=[30.0, 30.0], obs_ball_traj_length=10, reset_reaction_nframes=6,
                      ball_traj_out_x_file=tg["traj_out_x"], ball_traj_out_y_file=tg["traj_out_y"])
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in tg["grids"]]

    ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"], "params": {"seed": 42}}, params=SmallGrid)
    assert ctl.seed == 42
    assert tc.TennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"]}, params=SmallGrid).seed == 0
    ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"], "params": {"seed": 42}}, params=SmallGrid, seed=SEED)
    assert ctl.seed == SEED
    w, avg, std = MF.weights()
    rot = g["H/in/joint_rotmat"][0][np.arange(n) % 12]
    init = np.tile(avg, (n, 1)).astype(np.float32)
    init[:, 2] = 0.92
    init[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(n, 144)
    bind = g["H/joint_pos_bind"][0]
    player = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, n, w, avg, std, init, bind - bind[:1], True, DEV)
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)  # (the parent refused here)
    assert ctl.get_action_size() == 35
    task.reset()
    ctl.reset()
    torch.cuda.synchronize()
    sc = MF.scatter_of(mg, "step")

    def gen_ref(before, z, r, dt):
        return mvae.mvae_step_reference(player.settings, w, avg, std, before, z, r) if dt is np.float32 else mvae.mvae_step_reference(player.settings, w, avg, std, before, z, r, dt=dt)

    def judge(want, want64, before, z, r):
        sure = ~MF.near_threshold(player.settings, w, avg, std, before, z, r) & MF.well_conditioned(want, want64, sc)
        MF.assert_state(player.state_arrays(), want, sc, "the generator under the statement's latents", rows=np.nonzero(sure)[0])
        return int(sure.sum())

    rng = np.random.default_rng(2)
    judged = walked = 0
    buffers = None
    for k in range(steps):
        ctl._tar_action.copy_(torch.as_tensor((np.arange(n) + k) % 3 != 0, dtype=i64))  # a third of the envs in recovery, another third each step
        actions = torch.as_tensor(rng.normal(0, 0.5, (n, 35 + UNUSED)).astype(np.float32), device=DEV)
        rows, w_rows = walk_step(ctl, player, gen_ref, actions, k, "controller step %d" % k, sc, judge)
        judged, walked = judged + rows, walked + w_rows
        ptrs = (ctl._actions.data_ptr(), ctl._mvae_actions.data_ptr(), ctl._res_dof_actions.data_ptr())
        assert buffers in (None, ptrs), "the action tensors are allocated once"
        buffers = ptrs
        ctl.physics_step(torch.zeros((n, 75), device=DEV))
        ctl.post_physics_step()
        torch.cuda.synchronize()
        for x in (ctl.obs_buf, ctl.rew_buf, player._conditions, target.obs_buf):
            assert torch.isfinite(x).all()
    assert walked >= 8 and judged >= n * steps // 2, "too few rows judged: %d of %d (%d walked)" % (judged, n * steps, walked)
    # without the key the parent's torch lines run, and nothing is counted
    plain = tc.TennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": {k: v for k, v in cfg["v2p"].items() if k != "random_walk_in_recovery"}}, params=SmallGrid)
    plain.attach_imitation_target(target)
    plain.attach_motion_generator(player)
    actions = torch.as_tensor(rng.normal(0, 0.5, (n, 35)).astype(np.float32), device=DEV)
    plain.pre_physics_step(actions)
    assert plain._walk_calls == 0 and torch.equal(plain._mvae_actions, actions[:, :32] * 1.5) and torch.equal(plain._res_dof_actions, actions[:, 32:35] * 0.4)
    task.close()


@gpu
def test_two_player_controller_runs_a_shipped_config():
    """4 envs, `dual_mode: different`: the two-player controller inherits the action launch."""
    from tests import mvae_dual_fixture as DX
    from tests import mvae_fixture as MF
    from tests import mvae_target_fixture as TX
    from tests import tennis_dual_fixture as F
    from tests.gpu_util import synth_tables
    from vid2player3d_amd import mvae
    from vid2player3d_amd import mvae_target as mt
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg
    from vid2player3d_amd.tasks import tennis_controller_dual as td

    n, steps = 4, 3
    torch.manual_seed(19)
    d, tg, g = F.golden(), TX.golden(), DX.golden()
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = dict(SHIPPED, dual_mode="different", player=["nadal", "federer"], righthand=[False, True], grip=["semi_western", "eastern"], serve_from="near",
                      restitution=1.4, ball_friction=0.2, spin_scale=5, reward_type="return_w_estimate", reward_weights={"pos": 0.5, "ball_pos": 0.5},
                      court_min=[-30.0, -30.0], court_max=[30.0, 30.0], obs_ball_traj_length=10, reset_reaction_nframes=6, ball_traj_in_file=d["traj_in"])
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class InGrid:
        HEIGHT_RANGE, VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE = [tuple(r) for r in d["in_grids"]]

    ctl = td.DualTennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"], "params": {"seed": 5}}, traj_in_params=InGrid)
    assert ctl.seed == 5
    w, avg, std = DX.weights()
    rot = tg["H/in/joint_rotmat"][0][:4]
    frames = np.stack([avg[0], avg[1], avg[0], avg[1]]).astype(np.float32)
    frames[:, 2] = 0.92
    frames[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(4, 144)
    bind = np.stack([tg["H/joint_pos_bind"][0], tg["H/joint_pos_bind"][0] * np.float32(1.06)])
    player = mvae.MotionVAEPlayer(cfg["v2p"], n, w, avg, std, None, bind[0] - bind[0, :1], True, DEV, init_data_ready=[frames[0:1], frames[1:2]],
                                  init_data_serve=[frames[2:3], frames[3:4]])
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)  # (the parent refused here)
    assert ctl.get_action_size() == 35
    task.reset()
    ctl.reset(None, serve_vel_draws=np.random.default_rng(3).uniform(0, 1, (n // 2, 3)).astype(np.float32))
    torch.cuda.synchronize()
    sc = MF.scatter_of(g, "step")

    def gen_ref(before, z, r, dt):
        if dt is np.float32:
            return mvae.mvae_dual_step_reference(player.settings, w, avg, std, before, z, r)
        gen_ref.probes = ({}, {})
        return mvae.mvae_dual_step_reference(player.settings, w, avg, std, before, z, r, dt=dt, probes=gen_ref.probes)

    def judge(want, want64, before, z, r):
        sure = np.ones(n, bool)
        for i in (0, 1):  # (the rows the statement itself is sure of, as tests/test_gpu_mvae_dual.py judges them)
            pr = gen_ref.probes[i]
            near = np.abs(pr["phase"][:, None] - np.array([2.0, 2.5, 3.0, 3.1, 3.2, 3.3, 3.5])[None]).min(1) < 1e-3
            sure[i::2] &= ~(near | (np.abs(pr["atan2"]) < 1e-3) | (np.abs(pr["wrist_x"]) < 1e-3))
        for name, x in want.items():
            if x.dtype.kind == "f":
                sure &= np.abs(x.astype(np.float64) - want64[name]).reshape(n, -1).max(1) <= 2 * sc[name]
        MF.assert_state(player.state_arrays(), want, sc, "the two-player generator under the statement's latents", rows=np.nonzero(sure)[0])
        return int(sure.sum())

    rng = np.random.default_rng(23)
    judged = walked = 0
    for k in range(steps):
        ctl._tar_action.copy_(torch.as_tensor([k % 2, 1 - k % 2, 0, 1], dtype=i64))
        actions = torch.as_tensor(rng.normal(0, 0.5, (n, 35)).astype(np.float32), device=DEV)
        rows, w_rows = walk_step(ctl, player, gen_ref, actions, k, "two-player step %d" % k, sc, judge)
        judged, walked = judged + rows, walked + w_rows
        ctl.physics_step(torch.zeros((n, 75), device=DEV))
        ctl.post_physics_step()
        ctl.reset(ctl.reset_buf.nonzero(as_tuple=False).flatten())
        torch.cuda.synchronize()
        assert np.isfinite(ctl.obs_buf.cpu().numpy()).all() and np.isfinite(target.obs_buf.cpu().numpy()).all()
    assert walked == 2 * steps and judged >= 6, "too few rows judged: %d of %d" % (judged, n * steps)
    task.close()
