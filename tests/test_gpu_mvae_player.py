"""GPU checks of the MotionVAE motion generator's kernels (csrc/mvae_player.hip) against the fixture recorded from the reference and
against the numpy statement."""
import numpy as np
import pytest
import torch

from tests import mvae_fixture as FX
from vid2player3d_amd import mvae

gpu = pytest.mark.gpu
DEV = "cuda:0"
OUTPUT_ONLY = ("root_vel", "joint_rot6d", "joint_rotmat", "joint_rot", "phase_pred")


def N(t):
    return t.detach().cpu().numpy()


def make_player(g, v, n=None, init=None):
    w, avg, std = FX.weights()
    st = FX.settings(g, v)
    cfg = {"player": st["player"], "righthand": st["righthand"], "add_residual_dof": "euler"}
    init = g[v + "/init_feature"] if init is None else init
    return mvae.MotionVAEPlayer(cfg, len(init) if n is None else n, w, avg, std, init, g["joint_pos_bind_rel"], st["is_train"], DEV)


def poison(p, names):
    for k in names:
        t = getattr(p, "_" + k)
        t.fill_(float("nan") if t.dtype.is_floating_point else -7)


def load(p, s):
    for k, x in s.items():
        getattr(p, "_" + k).copy_(torch.as_tensor(np.ascontiguousarray(x)).reshape(getattr(p, "_" + k).shape))


@gpu
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_step_kernel_matches_the_reference_step_by_step(v):
    """every step teacher-forced from the recorded state, outputs poisoned beforehand; every env compared; what the step only reads comes
    back bit-identical"""
    g = FX.golden()
    p = make_player(g, v)
    train = p.settings["is_train"]
    read_only = {k: x.clone() for k, x in p._weights.items()}
    for t in range(len(g[v + "/latents"])):
        poison(p, OUTPUT_ONLY + ("racket_pos", "racket_normal"))
        load(p, FX.state_before(g, v, t))
        z, r = torch.as_tensor(g[v + "/latents"][t], device=DEV), torch.as_tensor(g[v + "/residual"][t], device=DEV)
        z0, r0 = z.clone(), r.clone()
        p.step(z, r)
        torch.cuda.synchronize()
        got = p.state_arrays()
        want = FX.state_after(g, v, t)
        assert len(want["root_pos"]) == p.num_envs
        FX.assert_state(got, want, FX.scatter_of(g, "step"), "variant %s step %d" % (v, t))
        assert torch.equal(z, z0) and torch.equal(r, r0) and p._latents is z
        if train:
            assert np.isnan(got["joint_rot"]).all(), "a training step writes no joint_rot"
        assert np.isnan(got["racket_pos"]).all() and np.isnan(got["racket_normal"]).all(), "the racket is the reset's"
    for k, x in read_only.items():
        assert torch.equal(p._weights[k], x), "the step wrote into %s" % k


@gpu
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_free_run_follows_the_recorded_trajectory(v):
    g = FX.golden()
    p = make_player(g, v)
    n = p.num_envs
    p.reset(torch.arange(n, device=DEV), torch.as_tensor(g[v + "/root_xy"], device=DEV))
    p._swing_type.copy_(torch.as_tensor(g[v + "/preset_swing"]))
    p._swing_type_cycle.copy_(torch.as_tensor(g[v + "/preset_swing"]))
    for t in range(len(g[v + "/latents"])):
        p.step(torch.as_tensor(g[v + "/latents"][t], device=DEV), torch.as_tensor(g[v + "/residual"][t], device=DEV))
        FX.assert_state(p.state_arrays(), FX.state_after(g, v, t), FX.scatter_of(g, "free"), "variant %s free run, step %d" % (v, t))


@gpu
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_reset_of_a_subset_of_ids(v):
    """the named rows match the fixture, all other rows are bit-identical, ids num_envs and -1 are skipped"""
    g = FX.golden()
    p = make_player(g, v)
    n = p.num_envs
    names = tuple(k for k in mvae.STATE_NAMES)
    poison(p, names)
    before = p.state_arrays()
    ids = [3, n, 0, -1, n - 1, 6]
    xy = np.zeros((len(ids), 2), np.float32)
    for i, e in enumerate(ids):
        xy[i] = g[v + "/root_xy"][e] if 0 <= e < n else (99.0, 99.0)
    p.reset(torch.as_tensor(ids, device=DEV), torch.as_tensor(xy, device=DEV))
    torch.cuda.synchronize()
    got = p.state_arrays()
    named = [e for e in ids if 0 <= e < n]
    others = [e for e in range(n) if e not in named]
    want = {k[len(v + "/reset/"):]: x for k, x in g.items() if k.startswith(v + "/reset/")}
    want = {k: x for k, x in want.items() if k != "phase_pred" and (k != "joint_rot" or not p.settings["is_train"])}
    FX.assert_state(got, want, FX.scatter_of(g, "reset"), "variant %s reset" % v, rows=named)
    for k in names:
        assert np.array_equal(got[k][others], before[k][others], equal_nan=True), "reset wrote %s of an env it was not given" % k
    assert np.isnan(got["phase_pred"]).all(), "the reset leaves the phase alone"


@pytest.fixture(scope="module")
def edge_inputs():
    return FX.edge_inputs()


_near_threshold, _well_conditioned = FX.near_threshold, FX.well_conditioned


@gpu
@pytest.mark.parametrize("n", [1, 33, 70, 257])
def test_tile_edges_against_the_numpy_statement(n, edge_inputs):
    """one reset and one step at batch sizes around the 32-env tile, federer in evaluation mode (every output is written)"""
    w, avg, std = FX.weights()
    e = edge_inputs
    cfg = {"player": "federer", "righthand": True, "add_residual_dof": "euler"}
    p = mvae.MotionVAEPlayer(cfg, n, w, avg, std, e["init"][:n], e["bind"], False, DEV)
    poison(p, mvae.STATE_NAMES)
    p.reset(torch.arange(n, device=DEV), torch.as_tensor(e["xy"][:n], device=DEV))
    g = FX.golden()
    zero = {k: np.zeros_like(x) for k, x in p.state_arrays().items()}
    want = mvae.mvae_reset_reference(p.settings, avg, std, zero, np.arange(n), e["init"][:n], e["xy"][:n], e["bind"])
    want64 = mvae.mvae_reset_reference(p.settings, avg, std, zero, np.arange(n), e["init"][:n], e["xy"][:n], e["bind"], dt=np.float64)
    got = p.state_arrays()
    sure = _well_conditioned(want, want64, FX.scatter_of(g, "reset"))
    assert sure.sum() >= 0.9 * n, "too few rows to judge: %d of %d" % (sure.sum(), n)
    FX.assert_state(got, {k: x for k, x in want.items() if k != "phase_pred"}, FX.scatter_of(g, "reset"), "N = %d reset" % n, rows=np.nonzero(sure)[0])
    p._swing_type.copy_(torch.as_tensor(e["swing"][:n]))
    p._swing_type_cycle.copy_(torch.as_tensor(e["swing"][:n]))
    before = p.state_arrays()
    poison(p, OUTPUT_ONLY)
    p.step(torch.as_tensor(e["z"][:n], device=DEV), torch.as_tensor(e["res"][:n], device=DEV))
    got = p.state_arrays()
    want = mvae.mvae_step_reference(p.settings, w, avg, std, before, e["z"][:n], e["res"][:n])
    sure = ~_near_threshold(p.settings, w, avg, std, before, e["z"][:n], e["res"][:n])
    want64 = mvae.mvae_step_reference(p.settings, w, avg, std, before, e["z"][:n], e["res"][:n], dt=np.float64)
    scatter = FX.scatter_of(g, "step")
    sure &= _well_conditioned(want, want64, scatter)
    assert sure.sum() >= 0.9 * n, "too few rows to judge: %d of %d" % (sure.sum(), n)
    FX.assert_state(got, want, scatter, "N = %d step" % n, rows=np.nonzero(sure)[0])
    assert all(np.isfinite(got[k]).all() for k in FX.FLOAT_STATE)


@gpu
@pytest.mark.parametrize("n", [1, 33, 70, 257])
def test_a_repeated_row_gives_identical_rows(n, edge_inputs):
    w, avg, std = FX.weights()
    e = edge_inputs
    rep = lambda x: np.repeat(x[5:6], n, 0)
    p = mvae.MotionVAEPlayer({"player": "nadal", "righthand": False, "add_residual_dof": "euler"}, n, w, avg, std, rep(e["init"]), e["bind"], False, DEV)
    p.reset(torch.arange(n, device=DEV), torch.as_tensor(rep(e["xy"]), device=DEV))
    p._swing_type.fill_(2)
    p.step(torch.as_tensor(rep(e["z"]), device=DEV), torch.as_tensor(rep(e["res"]), device=DEV))
    for k, x in p.state_arrays().items():
        assert np.isfinite(x).all()
        assert (x == x[0:1]).all(), "%s: rows of a repeated input differ" % k


@gpu
def test_controller_with_an_attached_player_equals_the_hand_driven_path():
    """TennisControllerTask with an attached player, stepped through pre_physics_step(actions) + post_physics_step(), against
    player.step(...) + post_physics_step(phase, swing, cycle) by hand: bit for bit over 3 steps on a small racket + ball batch, the
    `_swing_type_cycle = -1` of the reaction resets included."""
    from tests import tennis_fixture as F
    from tests.gpu_util import synth_tables
    from vid2player3d_amd import ball_traj
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg
    from vid2player3d_amd.tasks import tennis_controller as tc

    n, steps = 48, 3
    tg = F.golden()
    w, avg, std = FX.weights()
    rng = np.random.default_rng(4)
    init = (avg + std * rng.normal(0, 0.8, (n, FX.FRAME))).astype(np.float32)
    bind = rng.uniform(-0.3, 0.3, (24, 3)).astype(np.float32)
    actions = [torch.as_tensor(rng.normal(0, 1, (n, 35)).astype(np.float32), device=DEV) for _ in range(steps)]

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in tg["grids"]]

    def run(attached):
        torch.manual_seed(11)
        gen = ball_traj.TennisBallGenerator({"num_samples": 200}, device=DEV, seed=3)
        cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                          body_shape_mismatch="ignore", contact_solver="tgs")
        cfg["v2p"] = {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate",
                      "reward_weights": {"pos": 0.5, "ball_pos": 0.5}, "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10,
                      "reset_reaction_nframes": 1, "ball_traj_out_x_file": tg["traj_out_x"], "ball_traj_out_y_file": tg["traj_out_y"], "add_residual_dof": "euler",
                      "vae_action_scale": 0.7, "residual_dof_scale": 0.3}
        task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
        ctl = tc.TennisControllerTask(task, {"env": {"episodeLength": 300, "enableEarlyTermination": False}, "v2p": cfg["v2p"]}, params=SmallGrid)
        player = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, n, w, avg, std, init, bind, True, DEV)
        if attached:
            ctl.attach_motion_generator(player)
            assert ctl._swing_type_cycle is player._swing_type_cycle and ctl.get_action_size() == 35
        everyone = torch.arange(n, device=DEV)
        task.reset()
        torch.manual_seed(12)
        if not attached:
            player.reset(everyone)
        ctl.reset()
        record, cycle_resets = [], 0
        for k in range(steps):
            if attached:
                ctl.pre_physics_step(actions[k])
            else:
                player.step(actions[k][:, :32].clone() * 0.7, actions[k][:, 32:35].clone() * 0.3)
            task.step(torch.zeros((n, 75), device=DEV))
            if attached:
                ctl.post_physics_step()
            else:
                ctl.post_physics_step(player._phase_pred, player._swing_type, player._swing_type_cycle)
            due = ctl._reset_reaction_buf.clone()
            ids = ctl.reset_buf.nonzero(as_tuple=False).flatten()
            if not attached and len(ids):
                player.reset(ids)
            ctl.reset(ids)
            if not attached:
                player._swing_type_cycle[due] = -1  # (what `_reset_reaction_tasks` does to the player, physics_mvae_controller.py:223)
            cycle_resets += int(due.sum())
            assert (player._swing_type_cycle[due] == -1).all() and (ctl._swing_type_cycle[due] == -1).all()
            torch.cuda.synchronize()
            record.append({**{"ctl_" + a: x for a, x in ctl.state_arrays().items()}, **{"player_" + a: x for a, x in player.state_arrays().items()}})
        assert cycle_resets > 0, "no reaction reset happened"
        return record

    a, b = run(True), run(False)
    for k in range(steps):
        for name in a[k]:
            assert np.array_equal(a[k][name], b[k][name], equal_nan=True), "step %d: %s differs between the attached and the hand-driven path" % (k, name)
    assert np.isfinite(a[-1]["player_conditions"]).all() and (a[-1]["player_phase_pred"] != 0).any()
