"""GPU checks of the two-player motion generator (csrc/mvae_player_dual.hip: v2p_mvae_dual_step, v2p_mvae_dual_reset) against the fixture
recorded from the reference's `dual_mode: different`, against the numpy statement and against the single-player kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mvae_dual_fixture as DX
from tests import mvae_fixture as FX
from vid2player3d_amd import _lib, mvae

gpu = pytest.mark.gpu
DEV = "cuda:0"
OUTPUT_ONLY = ("root_vel", "joint_rot6d", "joint_rotmat", "joint_rot", "phase_pred")


def make_player(g, v, n=DX.N, sets=None):
    w, avg, std = DX.weights() if sets is None else sets
    return mvae.MotionVAEPlayer(DX.cfg(v), n, w, avg, std, None, g["joint_pos_bind_rel"], DX.VARIANTS[v]["is_train"], DEV, init_data_ready=list(g[v + "/init_ready"][:, None]),
                                init_data_serve=list(g[v + "/init_serve"][:, None]))


def poison(p, names):
    for k in names:
        t = getattr(p, "_" + k)
        t.fill_(float("nan") if t.dtype.is_floating_point else -7)


def load(p, s, rows=None):
    for k, x in s.items():
        t = getattr(p, "_" + k)
        x = torch.as_tensor(np.ascontiguousarray(x))
        (t if rows is None else t[:rows]).copy_(x.reshape((-1,) + t.shape[1:]))


def dev(x):
    return None if x is None else torch.as_tensor(x, device=DEV)


@gpu
@pytest.mark.parametrize("v", list(DX.VARIANTS))
def test_dual_step_matches_the_reference_step_by_step(v):
    """every step teacher-forced from the recorded state, outputs poisoned beforehand; every env of both sides compared - the even
    envs' root columns, which the reference normalises with side 1's statistics, among them"""
    g = DX.golden()
    p = make_player(g, v)
    train = p.settings["is_train"]
    read_only = [{k: x.clone() for k, x in w.items()} for w in p._weights]
    for t in range(DX.T):
        poison(p, OUTPUT_ONLY + ("racket_pos", "racket_normal"))
        load(p, DX.state_before(g, v, t))
        z, r = dev(g[v + "/latents"][t]), dev(DX.residual(g, v, t))
        z0 = z.clone()
        p.step(z, r)
        torch.cuda.synchronize()
        got = p.state_arrays()
        FX.assert_state(got, DX.state_after(g, v, t), FX.scatter_of(g, "step"), "variant %s step %d" % (v, t))
        assert torch.equal(z, z0) and p._latents is z
        if train:
            assert np.isnan(got["joint_rot"]).all(), "a training step writes no joint_rot"
        assert np.isnan(got["racket_pos"]).all() and np.isnan(got["racket_normal"]).all(), "the racket is the reset's"
    for w, before in zip(p._weights, read_only):
        for k, x in before.items():
            assert torch.equal(w[k], x), "the step wrote into %s" % k


@gpu
@pytest.mark.parametrize("v", list(DX.VARIANTS))
def test_dual_free_run_follows_the_recorded_trajectory(v):
    g = DX.golden()
    p = make_player(g, v)
    p.reset_dual(dev(g[v + "/reaction_ids"]), dev(g[v + "/recovery_ids"]), dev(g[v + "/root_xy"]))
    want = {k: x for k, x in DX.reset_state(g, v).items() if k != "phase_pred" and (k != "joint_rot" or not p.settings["is_train"])}
    FX.assert_state(p.state_arrays(), want, FX.scatter_of(g, "reset"), "variant %s reset of all envs" % v)
    p._swing_type.copy_(torch.as_tensor(g[v + "/preset_swing"]))
    p._swing_type_cycle.copy_(torch.as_tensor(g[v + "/preset_swing"]))
    for t in range(DX.T):
        p.step(dev(g[v + "/latents"][t]), dev(DX.residual(g, v, t)))
        FX.assert_state(p.state_arrays(), DX.state_after(g, v, t), FX.scatter_of(g, "free"), "variant %s free run, step %d" % (v, t))


@gpu
@pytest.mark.parametrize("case", list(enumerate((2, 62, 64, 66, 130))))
def test_dual_tile_edges_against_the_numpy_statement(case):
    """1, 31, 32, 33 and 65 rows per side: the evaluation variant's recorded states, tiled, stepped in tensors two envs longer than n
    and filled with a sentinel - rows n and n + 1 come back bit-identical; under both mappings of workgroups to sides"""
    t, n = case
    v = "B"
    g = DX.golden()
    w, avg, std = DX.weights()
    p = make_player(g, v, n + 2)
    tile = lambda x: np.concatenate([x] * (n // DX.N + 1))[:n]
    before = {k: tile(x) for k, x in DX.state_before(g, v, t).items()}
    z, r = tile(g[v + "/latents"][t]), tile(g[v + "/residual"][t])
    want = mvae.mvae_dual_step_reference(p.settings, w, avg, std, before, z, r)
    zt, rt = dev(z), dev(r)
    for mapping in (mvae.DUAL_MAP_HALVES, mvae.DUAL_MAP_PARITY):
        poison(p, mvae.STATE_NAMES)
        load(p, before, rows=n)
        sentinel = p.state_arrays()
        b = p._buffers()
        _lib.check(_lib.load().v2p_mvae_dual_step(p._cfg_struct, n, p._weights_struct, C.byref(b), _lib.ptr(zt), _lib.ptr(rt), mapping, _lib.current_stream(p.device)),
                   "v2p_mvae_dual_step")
        torch.cuda.synchronize()
        got = p.state_arrays()
        FX.assert_state({k: x[:n] for k, x in got.items()}, want, FX.scatter_of(g, "step"), "n = %d, mapping %d: step" % (n, mapping))
        for k, x in got.items():
            assert np.array_equal(x[n:], sentinel[k][n:], equal_nan=True), "n = %d, mapping %d: the step wrote %s of an env past n" % (n, mapping, k)


@gpu
@pytest.mark.parametrize("mapping", [mvae.DUAL_MAP_PARITY, mvae.DUAL_MAP_HALVES])
def test_dual_step_with_equal_sides_is_the_single_step_bit_for_bit(mapping):
    """both weight sets and both cfgs equal, n = 66 (three tiles of the single kernel, two per side of the dual one): a row's MFMA sums
    do not depend on its tile and the root-column quirk is the identity, so every output equals v2p_mvae_step's bit for bit - under
    either mapping of workgroups to sides"""
    n, v, t = 66, "B", 3
    g = DX.golden()
    w, avg, std = FX.weights()
    cfg = dict(DX.cfg(v), player=["federer", "federer"], righthand=[True, True])
    first = g[v + "/init_ready"][:1, None]
    dual = mvae.MotionVAEPlayer(cfg, n, (w, w), (avg, avg), (std, std), None, g["joint_pos_bind_rel"], False, DEV, init_data_ready=[first, first], init_data_serve=[first, first])
    dual.dual_mapping = mapping
    single = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, n, w, avg, std, first, g["joint_pos_bind_rel"][0], False, DEV)
    tile = lambda x: np.concatenate([x] * (n // DX.N + 1))[:n]
    z, r = dev(tile(g[v + "/latents"][t])), dev(tile(g[v + "/residual"][t]))
    for p in (dual, single):
        poison(p, mvae.STATE_NAMES)
        load(p, {k: tile(x) for k, x in DX.state_before(g, v, t).items()})
        p.step(z, r)
    torch.cuda.synchronize()
    a, b = dual.state_arrays(), single.state_arrays()
    assert np.isfinite(a["joint_rot"]).all() and np.isfinite(a["conditions"]).all()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s of the dual step with equal sides is not the single step's (%d values differ)" % (k, int((a[k] != b[k]).sum()))


@gpu
@pytest.mark.parametrize("v", list(DX.VARIANTS))
def test_dual_reset_of_two_pairs(v):
    """ids [2, 3, 8, 9] of 12 from the state after the last step: the named rows meet the fixture - racket position and normal by the
    server's chain and grip, read from bind rows 0 and 1 - and every other row stays bit-identical"""
    g = DX.golden()
    p = make_player(g, v)
    poison(p, mvae.STATE_NAMES)
    load(p, DX.state_before_part(g, v))
    before = p.state_arrays()
    p.reset_dual(dev(np.array(DX.PART_REACTION)), dev(np.array(DX.PART_RECOVERY)), dev(g[v + "/part/root_xy"]))
    torch.cuda.synchronize()
    got = p.state_arrays()
    rows = list(DX.PART_IDS)
    others = [e for e in range(DX.N) if e not in rows]
    want = {k: g["%s/part/%s" % (v, k)] for k in DX.RESET_STATE if k != "phase_pred" and (k != "joint_rot" or not p.settings["is_train"])}
    FX.assert_state({k: x[rows] for k, x in got.items()}, want, FX.scatter_of(g, "reset"), "variant %s reset of %s" % (v, rows))
    for k in mvae.STATE_NAMES:
        assert np.array_equal(got[k][others], before[k][others], equal_nan=True), "the reset wrote %s of an env it was not given" % k
    assert np.array_equal(got["phase_pred"], before["phase_pred"]), "the reset leaves the phase alone"
    with pytest.raises(ValueError, match="whole pairs"):
        p.reset_dual(dev(np.array([3])), dev(np.array([2, 9])))
    with pytest.raises(RuntimeError, match="reset_dual"):
        p.reset(dev(np.array([2, 3])))


@gpu
def test_two_player_controller_closes_its_control_loop():
    """4 envs, `dual_mode: different` with the match configs' lists over a two-player racket + ball task, the two-player generator and the
    imitation target attached: `reset` and 3 control steps.  Every step: the player's state is the numpy statement's, teacher-forced
    from the state the kernel found; the target rows are `target_step_reference` with the body shape of the env's parity (and not with
    side 0's for all); the task step reads the player's own tensors."""
    from tests import mvae_target_fixture as TX
    from tests import tennis_dual_fixture as F
    from tests.gpu_util import synth_tables
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
    betas = [[0.1 * (k + 1) for k in range(10)], [-0.05 * (k + 1) for k in range(10)]]
    cfg["v2p"] = {"dual_mode": "different", "player": ["nadal", "federer"], "righthand": [False, True], "grip": ["semi_western", "eastern"], "serve_from": "near",
                  "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate", "reward_weights": {"pos": 0.5, "ball_pos": 0.5},
                  "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10, "reset_reaction_nframes": 6, "ball_traj_in_file": d["traj_in"],
                  "add_residual_dof": "euler", "vae_action_scale": 0.7, "residual_dof_scale": 0.3, "smpl_beta": betas}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
    assert task.racket_players == ["nadal", "federer"]

    class InGrid:
        HEIGHT_RANGE, VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE = [tuple(r) for r in d["in_grids"]]

    ctl = td.DualTennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"]}, traj_in_params=InGrid)
    w, avg, std = DX.weights()
    rot = tg["H/in/joint_rotmat"][0][:4]
    frames = np.stack([avg[0], avg[1], avg[0], avg[1]]).astype(np.float32)  # ready of side 0, of side 1, serve of side 0, of side 1
    frames[:, 2] = 0.92
    frames[:, mvae.COL_ROT6D:] = np.concatenate([rot[..., 0], rot[..., 1]], -1).reshape(4, 144)
    bind = np.stack([tg["H/joint_pos_bind"][0], tg["H/joint_pos_bind"][0] * np.float32(1.06)])  # side 1: a taller body
    player = mvae.MotionVAEPlayer(cfg["v2p"], n, w, avg, std, None, bind[0] - bind[0, :1], True, DEV, init_data_ready=[frames[0:1], frames[1:2]],
                                  init_data_serve=[frames[2:3], frames[3:4]])
    single = mvae.MotionVAEPlayer({"player": "federer", "add_residual_dof": "euler"}, n, w[0], avg[0], std[0], frames, bind[0] - bind[0, :1], True, DEV)
    with pytest.raises(ValueError, match="disagree"):
        ctl.attach_motion_generator(single)
    with pytest.raises(ValueError, match="two-player task"):
        mt.ImitationTarget(task, single, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    target = mt.ImitationTarget(task, player, bind, {"v2p": cfg["v2p"], "env": {"no_scale_action": True}})
    bodies = target._reset_ref_motion_bodies.cpu().numpy()
    assert (bodies[:, 0] == 1).all() and np.array_equal(bodies[0::2, 1:], np.tile(np.float32(betas[0]), (2, 1))) and np.array_equal(bodies[1::2, 1:], np.tile(np.float32(betas[1]), (2, 1)))
    assert np.array_equal(target._env_shape_id.cpu().numpy(), np.arange(n) % 2)
    ctl.attach_imitation_target(target)
    ctl.attach_motion_generator(player)
    assert ctl._phase_pred is player._phase_pred and ctl._swing_type is player._swing_type and ctl._swing_type_cycle is player._swing_type_cycle
    assert ctl.get_action_size() == 35
    task.reset()
    ctl.reset(None, serve_vel_draws=np.random.default_rng(3).uniform(0, 1, (n // 2, 3)).astype(np.float32))
    torch.cuda.synchronize()
    A = lambda t: t.detach().cpu().numpy()
    cond = A(player._conditions)
    assert np.allclose(cond[0, 0, 3:], ((frames[0] - avg[0]) / std[0])[3:], atol=1e-5) and np.allclose(cond[1, 0, 3:], ((frames[3] - avg[1]) / std[1])[3:], atol=1e-5), \
        "'near': the even env receives from side 0's ready frame, the odd env serves from side 1's serve frame"
    assert np.array_equal(A(task._humanoid_root_states)[:, 0:3], A(player._root_pos)), "the pairs stand in the generator's pose"
    rng = np.random.default_rng(23)
    st, sc, sct = player.settings, FX.scatter_of(g, "step"), TX.scatter_of(tg, "step")
    judged = 0
    for k in range(steps):
        actions = torch.as_tensor(rng.normal(0, 0.5, (n, 35)).astype(np.float32), device=DEV)
        before = player.state_arrays()
        prev_row = A(task._target_bufs[1 - task._cur]).copy()
        ball, sim_root = A(task._ball_root_states)[:, 0:3].copy(), A(task._rigid_body_state).reshape(n, 24, 13)[:, 0, 0:3].copy()
        ctl.pre_physics_step(actions)
        torch.cuda.synchronize()
        # ---- the generator: the numpy statement from the state the kernel found, rows the statement itself is sure of
        z, r = A(actions)[:, :32] * np.float32(0.7), A(actions)[:, 32:35] * np.float32(0.3)
        pr = ({}, {})
        want = mvae.mvae_dual_step_reference(st, w, avg, std, before, z, r)
        want64 = mvae.mvae_dual_step_reference(st, w, avg, std, before, z, r, dt=np.float64, probes=pr)
        sure = np.ones(n, bool)
        for i in (0, 1):
            near = np.abs(pr[i]["phase"][:, None] - np.array([2.0, 2.5, 3.0, 3.1, 3.2, 3.3, 3.5])[None]).min(1) < 1e-3
            sure[i::2] &= ~(near | (np.abs(pr[i]["atan2"]) < 1e-3) | (np.abs(pr[i]["wrist_x"]) < 1e-3))
        for name, x in want.items():
            if x.dtype.kind == "f":
                sure &= np.abs(x.astype(np.float64) - want64[name]).reshape(n, -1).max(1) <= 2 * sc[name]
        judged += int(sure.sum())
        got = player.state_arrays()
        FX.assert_state(got, want, sc, "control step %d: the generator" % k, rows=np.nonzero(sure)[0])
        # ---- the target: the body shape of the env's parity
        written = A(task._target_bufs[task._cur]).copy()
        s = dict(root_pos=got["root_pos"], joint_rotmat=got["joint_rotmat"], residual_root=None, ball_pos=ball, sim_root_pos=sim_root, joint_pos_bind=bind,
                 env_shape_id=np.arange(n) % 2, prev_target=prev_row)
        TX.assert_row(written, mt.target_step_reference(target.settings, s)["target"], sct, "control step %d: the target" % k)
        side0 = mt.target_step_reference(target.settings, dict(s, env_shape_id=np.zeros(n, np.int64)))["target"]
        assert np.abs(side0[1::2] - written[1::2]).max() > 1e-3 and np.array_equal(side0[0::2], mt.target_step_reference(target.settings, s)["target"][0::2])
        ctl.physics_step(torch.zeros((n, 75), device=DEV))
        ctl.post_physics_step()
        assert ctl._phase_pred is player._phase_pred and np.array_equal(ctl.state_arrays()["phase_pred"], A(player._phase_pred))
        ctl.reset(ctl.reset_buf.nonzero(as_tuple=False).flatten())
        torch.cuda.synchronize()
        assert np.isfinite(A(ctl.obs_buf)).all() and np.isfinite(A(target.obs_buf)).all()
    assert judged >= 8, "too few rows to judge: %d of %d" % (judged, n * steps)
