"""CPU checks of the controller's reset by flags: the numpy statement of the start a reset player draws (`device_rng.root_xy_reference`),
the argument checks of the five new entry points (refused before any HIP call), the agent's `reset_mode` and the refusals by name."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from vid2player3d_amd import _lib, ctl_ppo as CP, device_rng as R, mvae
from vid2player3d_amd import mvae_target as mt

INVALID = -1


# ------------------------------------------------------------------------------------------------------------------ the draw
def test_root_xy_reference_range_and_independence_of_the_batch():
    xy = R.root_xy_reference(11, 3, 4096)
    assert xy.dtype == np.float32 and xy.shape == (4096, 2)
    assert (xy[:, 0] >= -1.0).all() and (xy[:, 0] < 1.0).all() and (xy[:, 1] >= -13.75).all() and (xy[:, 1] < -12.25).all()
    assert xy[:, 0].min() < -0.9 and xy[:, 0].max() > 0.9 and xy[:, 1].min() < -13.6 and xy[:, 1].max() > -12.4  # (the range is used)
    for n in (1, 7, 67):  # an env's draw does not change with n, nor with which envs are asked for
        assert np.array_equal(R.root_xy_reference(11, 3, n), xy[:n])
    assert np.array_equal(R.root_xy_reference(11, 3, 3, envs=[4000, 5, 66]), xy[[4000, 5, 66]])
    assert not np.array_equal(R.root_xy_reference(11, 4, 64), xy[:64]) and not np.array_equal(R.root_xy_reference(12, 3, 64), xy[:64])
    assert np.array_equal(R.root_xy_reference(11, 2 ** 40 + 3, 8), R.root_xy_reference(11, 2 ** 40 + 3, 4096)[:8])


def test_root_xy_reference_is_the_law_on_the_words_of_its_stream():
    """x = (u0 - 0.5) * 2 + 0, y = (u1 - 0.5) * 1.5 + (-13) in float32, one rounding per operation, on words 0 and 1 of block 0 of stream 2"""
    assert R.STREAM_ROOT == 2 and len({R.STREAM_WALK, R.STREAM_RESET, R.STREAM_ROOT}) == 3
    f = np.float32
    n, seed, call = 130, 0x123456789ABCDEF, 2 ** 33 + 5
    w = R.philox_words(seed, call, R.STREAM_ROOT, n, 1)
    u = (w[:, :2] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    x = ((u[:, 0] - f(0.5)).astype(f) * f(2.0)).astype(f) + f(0.0)
    y = ((u[:, 1] - f(0.5)).astype(f) * f(1.5)).astype(f) + f(-13.0)
    got = R.root_xy_reference(seed, call, n)
    assert np.array_equal(got, np.stack([x, y], 1).astype(f))
    # the same law in double, rounded once, is at most an ulp of 13 away: the float32 statement is the law, not an approximation of another
    u64 = (w[:, :2] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    assert np.abs(got - ((u64 - 0.5) * (2.0, 1.5) + (0.0, -13.0))).max() <= 2.0 ** -20
    # another stream gives other words
    assert not np.array_equal(w, R.philox_words(seed, call, R.STREAM_RESET, n, 1))


def test_the_players_torch_draw_is_the_same_law():
    """`MotionVAEPlayer.draw_root_xy` (the id-list path's draw) on a uniform u: the expression the kernel restates, in torch float32"""
    u = torch.rand((64, 2), generator=torch.Generator().manual_seed(1))
    want = (u - 0.5) * torch.tensor([2.0, 1.5]) + torch.tensor([0.0, -13.0])
    f = np.float32
    un = u.numpy()
    got = ((un - f(0.5)) * np.array(R.ROOT_XY_SCALE, f) + np.array(R.ROOT_XY_OFFSET, f)).astype(f)
    assert np.array_equal(got, want.numpy())


# ------------------------------------------------------------------------------------------------------------------ the entry points
def _mvae_structs():
    one = 16  # (a non-null placeholder: every call below is refused before anything is dereferenced)
    cfg = mvae.cfg_struct(dict(player="federer", righthand=True, is_train=True, add_residual_dof=True))
    w = _lib.MvaeWeights(**{k: one for k in _lib.MVAE_WEIGHT_NAMES})
    b = _lib.MvaeBuffers(**{k: one for k in _lib.MVAE_BUFFER_NAMES})
    return cfg, w, b


def test_mvae_reset_flagged_refuses_bad_arguments_without_a_gpu():
    L = _lib.load()
    fn, one = L.v2p_mvae_reset_flagged, C.c_void_p(16)
    cfg, w, b = _mvae_structs()
    draw = _lib.MvaeRootRule(rule=_lib.MVAE_ROOT_RULES["draw"], seed=1, call=0)
    ok = lambda **kw: dict(dict(cfg=C.byref(cfg), n=8, w=C.byref(w), b=C.byref(b), flags=one, init=one, xy=one, rule=C.byref(draw), bind=one), **kw)
    call = lambda a: fn(a["cfg"], a["n"], a["w"], a["b"], a["flags"], a["init"], a["xy"], a["rule"], a["bind"], None)
    bad_cfg = mvae.cfg_struct(dict(player="federer", righthand=True, is_train=True, add_residual_dof=True))
    bad_cfg.frame_size = 100
    no_racket = _lib.MvaeBuffers(**{k: 16 for k in _lib.MVAE_BUFFER_NAMES if k != "racket_pos"})
    bad_rule = _lib.MvaeRootRule(rule=7, seed=1, call=0)
    for what, a in (("null cfg", ok(cfg=None)), ("null weights", ok(w=None)), ("null buffers", ok(b=None)), ("n < 0", ok(n=-1)), ("n above 2^31-1", ok(n=2 ** 31)),
                    ("another architecture", ok(cfg=C.byref(bad_cfg))), ("no racket_pos", ok(b=C.byref(no_racket))), ("null flags", ok(flags=None)),
                    ("null init_feature", ok(init=None)), ("null bind", ok(bind=None)), ("neither root_xy nor a rule", ok(xy=None, rule=None)),
                    ("an unknown rule", ok(xy=None, rule=C.byref(bad_rule)))):
        assert call(a) == INVALID, what
        assert b"v2p_mvae_reset_flagged" in L.v2p_last_error(), what
    assert call(ok(n=0)) == 0 and call(ok(n=0, flags=None, init=None, bind=None)) == INVALID  # n = 0 is a no-op of a well-formed call


def _target_structs():
    st = dict(control_dt=1 / 30, fix_head_orientation=False, head_body=13, smpl_head=15, smpl_neck=12, key_bodies=[4, 8, 18, 23],
              smpl_parents=[-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], smpl_of_body=None, pd_target_base="target_pos",
              no_scale_action=True)
    order = list(range(24))
    order[13], order[15] = 15, 13  # (a body order in which body 13 is SMPL joint 15, the head)
    st["smpl_of_body"] = order
    b = _lib.MvaeTargetBuffers(root_pos=16, joint_rotmat=16, joint_pos_bind=16, target=16)
    return mt.cfg_struct(st), b


def test_target_reset_flagged_refuses_bad_arguments_without_a_gpu():
    L = _lib.load()
    fn, one = L.v2p_mvae_target_reset_flagged, C.c_void_p(16)
    c, b = _target_structs()
    assert fn(C.byref(c), 0, C.byref(b), one, None) == 0, L.v2p_last_error()  # (the cfg is well formed: n = 0 is a no-op)
    no_target = _lib.MvaeTargetBuffers(root_pos=16, joint_rotmat=16, joint_pos_bind=16)
    bad_dt, _ = _target_structs()
    bad_dt.dt = 0.0
    bad_tree, _ = _target_structs()
    bad_tree.smpl_parents[5] = 9
    for what, args in (("null cfg", (None, 8, C.byref(b), one)), ("null buffers", (C.byref(c), 8, None, one)), ("n < 0", (C.byref(c), -1, C.byref(b), one)),
                       ("null flags", (C.byref(c), 8, C.byref(b), None)), ("null target", (C.byref(c), 8, C.byref(no_target), one)),
                       ("dt 0", (C.byref(bad_dt), 8, C.byref(b), one)), ("no tree", (C.byref(bad_tree), 8, C.byref(b), one))):
        assert fn(*args, None) == INVALID, what
        assert b"v2p_mvae_target_reset_flagged" in L.v2p_last_error(), what


def test_push_and_bookkeeping_entries_refuse_bad_arguments_without_a_gpu():
    L = _lib.load()
    one = C.c_void_p(16)
    assert L.v2p_env_push_state_flagged(None, one, 1, None) == INVALID and b"v2p_env_push_state_flagged" in L.v2p_last_error()
    full = _lib.CtlResetBuffers(**{k: 16 for k in _lib.CTL_RESET_BUFFER_NAMES})
    for name, writes in (("v2p_ctl_reset_begin", ("progress", "terminate", "num_reset_reaction", "num_reset", "distance")),
                         ("v2p_ctl_reset_end", ("reset_reaction", "reset_recovery"))):
        fn = getattr(L, name)
        assert fn(-1, one, C.byref(full), None) == INVALID and name.encode() in L.v2p_last_error()
        assert fn(8, None, C.byref(full), None) == INVALID and name.encode() in L.v2p_last_error()
        assert fn(8, one, None, None) == INVALID and name.encode() in L.v2p_last_error()
        for k in writes:
            part = _lib.CtlResetBuffers(**{j: 16 for j in _lib.CTL_RESET_BUFFER_NAMES if j != k})
            assert fn(8, one, C.byref(part), None) == INVALID, (name, k)
            assert name.encode() in L.v2p_last_error() and k.encode() in L.v2p_last_error(), (name, k)
        other = _lib.CtlResetBuffers(**{k: 16 for k in writes})  # (the buffers the other call writes may be null)
        assert fn(0, one, C.byref(other), None) == 0
        assert fn(0, one, C.byref(full), None) == 0


def test_abi_version_stays_15_and_the_entries_are_bound():
    L = _lib.load()
    assert L.v2p_abi_version() == 15 and _lib.ABI_VERSION == 15
    for name in ("v2p_mvae_reset_flagged", "v2p_mvae_target_reset_flagged", "v2p_env_push_state_flagged", "v2p_ctl_reset_begin", "v2p_ctl_reset_end"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def test_from_config_accepts_reset_mode(monkeypatch):
    from tests import ctl_ppo_fixture as FX

    assert inspect.signature(CP.ControllerPPOAgent.__init__).parameters["reset_mode"].default == "ids"
    seen = {}
    monkeypatch.setattr(CP.ControllerPPOAgent, "__init__", lambda self, ctl, **kw: seen.update(kw))
    CP.ControllerPPOAgent.from_config(object(), FX.small_params(), reset_mode="flags")
    assert seen["reset_mode"] == "flags" and seen["horizon_length"] == FX.T
    seen.clear()
    CP.ControllerPPOAgent.from_config(object(), FX.small_params())
    assert "reset_mode" not in seen  # (the default is the constructor's: the id-list path)


def test_refusals_are_raised_by_name():
    from tests import ctl_ppo_fixture as FX
    from vid2player3d_amd.tasks import tennis_controller as tc
    from vid2player3d_amd.tasks import tennis_controller_dual as td

    scripted = FX.ScriptedController(torch.device("cpu"))  # (has `reset(ids)` only)
    with pytest.raises(NotImplementedError, match="reset_by_flags"):
        CP.ControllerPPOAgent(scripted, reset_mode="flags")
    with pytest.raises(ValueError, match="reset_mode"):
        CP.ControllerPPOAgent(scripted, reset_mode="mask")
    two = types.SimpleNamespace(device="cpu", task=types.SimpleNamespace(racket_players=(0, 1)), reset_by_flags=lambda: None)
    with pytest.raises(NotImplementedError, match="two-player"):
        CP.ControllerPPOAgent(two, reset_mode="flags")
    with pytest.raises(RuntimeError, match="GPU"):  # (the default mode gets as far as the device check, as ever)
        CP.ControllerPPOAgent(scripted)
    with pytest.raises(NotImplementedError, match="task_reset 'device'"):
        tc.TennisControllerTask.reset_by_flags(types.SimpleNamespace(_task_reset="torch"))
    with pytest.raises(NotImplementedError, match="pairs"):
        td.DualTennisControllerTask.reset_by_flags(types.SimpleNamespace())
    for cfg, dual in (({"dual_mode": True}, False), ({"dual_mode": "different"}, True)):
        with pytest.raises(NotImplementedError, match="dual_mode"):
            mvae.MotionVAEPlayer.reset_flagged(types.SimpleNamespace(_is_dual=dual, cfg=cfg), torch.zeros(4, dtype=torch.long))


def test_flagged_statements_are_the_id_list_statements_over_the_flagged_envs():
    """the thin wrappers: `*_flagged_reference(flags)` is `*_reference(flatnonzero(flags))` with the per-env rows gathered"""
    from tests import mvae_fixture as MF

    e = MF.edge_inputs()
    _, avg, std = MF.weights()
    n = 9
    st = mvae.player_settings({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, False)
    rng = np.random.default_rng(2)
    shapes = dict(conditions=(n, 1, 288), root_pos=(n, 3), root_vel=(n, 3), joint_rot6d=(n, 24, 6), joint_rotmat=(n, 24, 3, 3), joint_rot=(n, 24, 3), racket_pos=(n, 3),
                  racket_normal=(n, 3), phase_pred=(n,))
    s = {k: rng.normal(size=v).astype(np.float32) for k, v in shapes.items()}
    s.update(swing_type=np.full(n, 2, np.int64), swing_type_cycle=np.full(n, 1, np.int64))
    flags = np.array([0, 2, 0, 0, -1, 0, 0, 0, 1], np.int64)
    xy = R.root_xy_reference(5, 0, n)
    got = mvae.mvae_reset_flagged_reference(st, avg, std, s, flags, e["init"][:n], xy, e["bind"])
    want = mvae.mvae_reset_reference(st, avg, std, s, [1, 4, 8], e["init"][[1, 4, 8]], xy[[1, 4, 8]], e["bind"])
    for k in want:
        assert np.array_equal(got[k], want[k]), k
        keep = [0, 2, 3, 5, 6, 7]
        assert np.array_equal(np.asarray(got[k])[keep].reshape(6, -1), np.asarray(s[k])[keep].reshape(6, -1)), k
    assert np.array_equal(got["root_pos"][[1, 4, 8], :2], xy[[1, 4, 8]])
