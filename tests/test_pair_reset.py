"""CPU checks of the two-player controller's pair reset by flags: the numpy statement of the serve velocity a reset pair draws
(`device_rng.serve_vel_reference`), the flagged statements against the id-list statements, the argument checks of the four new entry
points (refused before any HIP call), the symbols, and that the three refusals of the single-player names still stand."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import pair_reset_fixture as PX
from vid2player3d_amd import _lib, device_rng as R, mvae
from vid2player3d_amd.tasks import tennis_controller_dual as td

INVALID, UNSUPPORTED = -1, -2
NEW_ENTRIES = ("v2p_ctl_pair_reset_begin", "v2p_ctl_pair_reset_end", "v2p_tennis_dual_serve_flagged", "v2p_mvae_dual_reset_flagged")


# ------------------------------------------------------------------------------------------------------------------ the serve draw
def test_serve_vel_reference_range_and_independence_of_the_batch():
    v = R.serve_vel_reference(11, 3, 4096)
    assert v.dtype == np.float32 and v.shape == (4096, 3)
    for k, (lo, hi) in enumerate(((-2.0, 2.0), (28.0, 32.0), (5.0, 8.0))):
        assert (v[:, k] >= lo).all() and (v[:, k] < hi).all(), k
        assert v[:, k].min() < lo + 0.05 * (hi - lo) and v[:, k].max() > hi - 0.05 * (hi - lo), k  # (the range is used)
    for n in (2, 14, 66):  # an env's draw does not change with n, nor with which envs are asked for
        assert np.array_equal(R.serve_vel_reference(11, 3, n), v[:n])
    assert np.array_equal(R.serve_vel_reference(11, 3, 3, envs=[4001, 5, 67]), v[[4001, 5, 67]])
    assert not np.array_equal(R.serve_vel_reference(11, 4, 64), v[:64]) and not np.array_equal(R.serve_vel_reference(12, 3, 64), v[:64])
    assert np.array_equal(R.serve_vel_reference(11, 2 ** 40 + 3, 8), R.serve_vel_reference(11, 2 ** 40 + 3, 4096)[:8])


def test_serve_vel_reference_is_the_law_on_the_words_of_its_stream():
    """u * (4, 4, 3) + (-2, 28, 5) in float32, one rounding per operation, on words 0..2 of block 0 of stream 3"""
    assert R.STREAM_SERVE == 3 and len({R.STREAM_WALK, R.STREAM_RESET, R.STREAM_ROOT, R.STREAM_SERVE}) == 4
    f = np.float32
    n, seed, call = 130, 0x123456789ABCDEF, 2 ** 33 + 5
    w = R.philox_words(seed, call, R.STREAM_SERVE, n, 1)
    u = (w[:, :3] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    cols = [(u[:, k] * f(s)).astype(f) + f(o) for k, (s, o) in enumerate(((4.0, -2.0), (4.0, 28.0), (3.0, 5.0)))]
    got = R.serve_vel_reference(seed, call, n)
    assert np.array_equal(got, np.stack(cols, 1).astype(f))
    u64 = (w[:, :3] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    assert np.abs(got - (u64 * (4.0, 4.0, 3.0) + (-2.0, 28.0, 5.0))).max() <= 2.0 ** -19  # (an ulp of 32)
    assert not np.array_equal(w, R.philox_words(seed, call, R.STREAM_ROOT, n, 1))  # another stream gives other words


def test_the_controllers_torch_serve_is_the_same_law():
    """`DualTennisControllerTask.reset(ids)`'s torch expression on a uniform u, and the statement's on the same u: bit for bit"""
    u = torch.rand((64, 3), generator=torch.Generator().manual_seed(1))
    want = u.reshape(-1, 3) * torch.tensor([4.0, 4.0, 3.0]) + torch.tensor([-2.0, 28.0, 5.0])
    f = np.float32
    got = (u.numpy() * np.array(R.SERVE_VEL_SCALE, f) + np.array(R.SERVE_VEL_OFFSET, f)).astype(f)
    assert np.array_equal(got, want.numpy())
    ball = np.random.default_rng(0).normal(size=(128, 13)).astype(f)
    head = np.random.default_rng(1).normal(size=(128, 3)).astype(f)
    flags = np.zeros(128, np.int64)
    flags[0::2] = 1  # the even env of every pair alone: every pair is flagged
    for serve_from, servers in (("near", np.arange(1, 128, 2)), ("far", np.arange(0, 128, 2))):
        out = td.serve_flagged_reference(flags, serve_from, head, ball, u.numpy())
        assert np.array_equal(out[servers, 7:10], want.numpy()) and np.array_equal(out[servers, 0:3], head[servers])
        assert np.array_equal(out[servers, 10:13], np.tile(np.array([-40, 0, 0], f), (64, 1))) and np.array_equal(out[servers, 3:7], ball[servers, 3:7])
        assert np.array_equal(out[servers ^ 1], ball[servers ^ 1]), "a receiver's ball was written"


# ------------------------------------------------------------------------------------------------------------------ the statements
def test_pair_flags_and_bookkeeping_statements():
    flags = np.array([0, 0, 1, 0, 0, -1, 2, 2, 0, 0], np.int64)
    whole, up = td.pair_flags_reference(flags)
    assert whole.tolist() == [0, 0, 1, 1, 1, -1, 2, 2, 0, 0] and up.tolist() == [False, False, True, True, True, True, True, True, False, False]
    rng = np.random.default_rng(4)
    n = len(flags)
    s = dict(progress=rng.integers(1, 9, n), terminate=rng.integers(0, 2, n), num_reset_reaction=rng.integers(1, 5, n), num_reset=rng.integers(0, 7, n),
             distance=rng.uniform(1, 2, n).astype(np.float32), reset_reaction=rng.integers(0, 2, n).astype(bool), reset_recovery=rng.integers(0, 2, n).astype(bool))
    for serve_from, receivers in (("near", [2, 4, 6]), ("far", [3, 5, 7])):
        o, after = td.pair_reset_begin_reference(s, flags, serve_from)
        assert np.array_equal(after, whole)
        for k in ("progress", "terminate", "num_reset_reaction", "distance"):
            assert not o[k][up].any() and np.array_equal(o[k][~up], s[k][~up]), k
        assert np.array_equal(o["num_reset"], s["num_reset"] + up)
        assert np.flatnonzero(o["reset_reaction"] & up).tolist() == receivers and np.array_equal(o["reset_recovery"][up], ~o["reset_reaction"][up])
        assert np.array_equal(o["reset_reaction"][~up], s["reset_reaction"][~up]) and np.array_equal(o["reset_recovery"][~up], s["reset_recovery"][~up])
    assert not td.pair_reset_end_reference(whole).any()
    with pytest.raises(ValueError, match="serve_from"):
        td.pair_reset_begin_reference(s, flags, "left")
    for name, f in PX.pair_flag_patterns(18).items():
        whole, up = td.pair_flags_reference(f)
        assert np.array_equal(whole != 0, up) and np.array_equal(up[0::2], up[1::2]) and np.array_equal(whole[f != 0], f[f != 0]), name
    assert PX.pair_flag_patterns(18)["even_env_only"][1::2].sum() == 0 and PX.pair_flag_patterns(18)["odd_env_only"][0::2].sum() == 0


def test_flagged_statement_of_the_generator_is_the_id_list_statement_over_the_flagged_pairs():
    from tests import mvae_dual_fixture as DX
    from tests import mvae_fixture as MF

    g = DX.golden()
    _, avg, std = DX.weights()
    n, v = DX.N, "B"
    st = DX.settings(v)
    rng = np.random.default_rng(2)
    shapes = dict(conditions=(n, 1, 288), root_pos=(n, 3), root_vel=(n, 3), joint_rot6d=(n, 24, 6), joint_rotmat=(n, 24, 3, 3), joint_rot=(n, 24, 3), racket_pos=(n, 3),
                  racket_normal=(n, 3), phase_pred=(n,))
    s = {k: rng.normal(size=sh).astype(np.float32) for k, sh in shapes.items()}
    s.update(swing_type=np.full(n, 2, np.int64), swing_type_cycle=np.full(n, 1, np.int64))
    ready, serve = DX.init_rows(g, v)
    bind = MF.edge_inputs()["bind"]
    xy = R.root_xy_reference(5, 0, n)
    flags = np.array([0, 0, 2, -1, 0, 0, 0, 0, 1, 1, 0, 0], np.int64)
    ids = [2, 3, 8, 9]
    for serve_from in ("near", "far"):
        receives = (np.arange(n) % 2 == _lib.SERVE_FROM[serve_from])[:, None]
        table = np.where(receives, ready, serve)
        got = mvae.mvae_dual_reset_flagged_reference(st, avg, std, s, flags, table, xy, bind)
        receivers = [e for e in ids if e % 2 == _lib.SERVE_FROM[serve_from]]
        _, feature = DX.reset_inputs(g, v, receivers, [e ^ 1 for e in receivers])
        want = mvae.mvae_dual_reset_reference(st, avg, std, s, ids, feature, xy[ids], bind)
        keep = [e for e in range(n) if e not in ids]
        for k in want:
            assert np.array_equal(got[k], want[k]), k
            assert np.array_equal(np.asarray(got[k])[keep].reshape(len(keep), -1), np.asarray(s[k])[keep].reshape(len(keep), -1)), k
        assert np.array_equal(got["root_pos"][ids, :2], xy[ids])
    half = flags.copy()
    half[3] = 0
    with pytest.raises(ValueError, match="pair"):
        mvae.mvae_dual_reset_flagged_reference(st, avg, std, s, half, table, xy, bind)
    with pytest.raises(ValueError, match="one \\[24,3\\] row"):
        mvae.mvae_dual_reset_flagged_reference(st, avg, std, s, flags, table, xy, np.tile(bind, (6, 1, 1)))


# ------------------------------------------------------------------------------------------------------------------ the entry points
def test_bookkeeping_and_serve_entries_refuse_bad_arguments_without_a_gpu():
    L = _lib.load()
    one = C.c_void_p(16)
    full = _lib.CtlResetBuffers(**{k: 16 for k in _lib.CTL_RESET_BUFFER_NAMES})
    name = b"v2p_ctl_pair_reset_begin"
    begin = L.v2p_ctl_pair_reset_begin
    for what, args in (("n < 0", (-2, one, C.byref(full), 0)), ("odd n", (7, one, C.byref(full), 0)), ("null flags", (8, None, C.byref(full), 0)),
                       ("null buffers", (8, one, None, 0)), ("unknown serve_from", (8, one, C.byref(full), 2)), ("serve_from -1", (8, one, C.byref(full), -1))):
        assert begin(*args, None) == INVALID and name in L.v2p_last_error(), what
    for k in _lib.CTL_RESET_BUFFER_NAMES:
        part = _lib.CtlResetBuffers(**{j: 16 for j in _lib.CTL_RESET_BUFFER_NAMES if j != k})
        assert begin(8, one, C.byref(part), 0, None) == INVALID and name in L.v2p_last_error() and k.encode() in L.v2p_last_error(), k
    assert begin(0, one, C.byref(full), 1, None) == 0
    name, end = b"v2p_ctl_pair_reset_end", L.v2p_ctl_pair_reset_end
    for what, args in (("n < 0", (-2, one)), ("odd n", (7, one)), ("null flags", (8, None))):
        assert end(*args, None) == INVALID and name in L.v2p_last_error(), what
    assert end(0, one, None) == 0
    name, serve = b"v2p_tennis_dual_serve_flagged", L.v2p_tennis_dual_serve_flagged
    rule = _lib.ServeRule(seed=1, call=0)
    for what, args in (("n < 0", (-2, one, 0, one, one, one, None)), ("odd n", (7, one, 0, one, one, one, None)), ("n above 2^31-1", (2 ** 31, one, 0, one, one, one, None)),
                       ("null flags", (8, None, 0, one, one, one, None)), ("unknown serve_from", (8, one, 5, one, one, one, None)),
                       ("null racket_pos", (8, one, 0, None, one, one, None)), ("null ball_state", (8, one, 0, one, None, one, None)),
                       ("neither draws nor a rule", (8, one, 1, one, one, None, None))):
        assert serve(*args, None) == INVALID and name in L.v2p_last_error(), what
    assert serve(0, one, 1, one, one, None, C.byref(rule), None) == 0 and serve(0, one, 0, one, one, one, None, None) == 0


def _dual_structs():
    one = 16  # (a non-null placeholder: every call below is refused before anything is dereferenced)
    side = lambda: mvae.cfg_struct(dict(player="federer", righthand=True, is_train=True, add_residual_dof=True))
    cfg = (_lib.MvaeCfg * 2)(side(), side())
    w = (_lib.MvaeWeights * 2)(*(_lib.MvaeWeights(**{k: one for k in _lib.MVAE_WEIGHT_NAMES}) for _ in range(2)))
    b = _lib.MvaeBuffers(**{k: one for k in _lib.MVAE_BUFFER_NAMES})
    return cfg, w, b


def test_mvae_dual_reset_flagged_refuses_bad_arguments_without_a_gpu():
    L = _lib.load()
    fn, one = L.v2p_mvae_dual_reset_flagged, C.c_void_p(16)
    cfg, w, b = _dual_structs()
    racket = _lib.MvaeRacket(righthand=1)
    draw = _lib.MvaeRootRule(rule=_lib.MVAE_ROOT_RULES["draw"], seed=1, call=0)
    ok = lambda **kw: dict(dict(cfg=cfg, n=8, w=w, b=C.byref(b), racket=C.byref(racket), flags=one, init=one, xy=one, rule=C.byref(draw), bind=one, rows=1), **kw)
    call = lambda a: fn(a["cfg"], a["n"], a["w"], a["b"], a["racket"], a["flags"], a["init"], a["xy"], a["rule"], a["bind"], a["rows"], None)
    bad_cfg, _, _ = _dual_structs()
    bad_cfg[1].frame_size = 100
    disagree, _, _ = _dual_structs()
    disagree[1].is_train = 0
    no_racket = _lib.MvaeBuffers(**{k: 16 for k in _lib.MVAE_BUFFER_NAMES if k != "racket_pos"})
    bad_rule = _lib.MvaeRootRule(rule=7, seed=1, call=0)
    for what, a in (("null cfg", ok(cfg=None)), ("null weights", ok(w=None)), ("null buffers", ok(b=None)), ("n < 0", ok(n=-2)), ("odd n", ok(n=7)), ("n above 2^31-1", ok(n=2 ** 31)),
                    ("another architecture", ok(cfg=bad_cfg)), ("sides that disagree", ok(cfg=disagree)), ("no racket_pos", ok(b=C.byref(no_racket))),
                    ("null racket", ok(racket=None)), ("null flags", ok(flags=None)), ("null init_feature", ok(init=None)), ("null bind", ok(bind=None)),
                    ("neither root_xy nor a rule", ok(xy=None, rule=None)), ("an unknown rule", ok(xy=None, rule=C.byref(bad_rule))), ("no bind row", ok(rows=0))):
        assert call(a) == INVALID, what
        assert b"v2p_mvae_dual_reset_flagged" in L.v2p_last_error(), what
    assert call(ok(rows=4)) == UNSUPPORTED and b"v2p_mvae_dual_reset_flagged" in L.v2p_last_error() and b"prefix count" in L.v2p_last_error()
    assert call(ok(n=0)) == 0 and call(ok(n=0, flags=None)) == INVALID  # n = 0 is a no-op of a well-formed call


def test_abi_version_stays_15_and_the_new_entries_are_bound():
    L = _lib.load()
    assert L.v2p_abi_version() == 15 and _lib.ABI_VERSION == 15
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    assert _lib.SERVE_FROM == {"near": 0, "far": 1}


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def test_the_three_refusals_of_the_single_player_names_still_stand():
    from vid2player3d_amd import ctl_ppo as CP

    with pytest.raises(NotImplementedError, match="pairs"):
        td.DualTennisControllerTask.reset_by_flags(types.SimpleNamespace())
    for cfg, dual in (({"dual_mode": True}, False), ({"dual_mode": "different"}, True)):
        with pytest.raises(NotImplementedError, match="dual_mode"):
            mvae.MotionVAEPlayer.reset_flagged(types.SimpleNamespace(_is_dual=dual, cfg=cfg), torch.zeros(4, dtype=torch.long))
    two = types.SimpleNamespace(device="cpu", task=types.SimpleNamespace(racket_players=(0, 1)), reset_by_flags=lambda: None)
    with pytest.raises(NotImplementedError, match="two-player"):
        CP.ControllerPPOAgent(two, reset_mode="flags")


def test_new_python_names_check_their_arguments_without_a_gpu():
    from vid2player3d_amd import match

    single = types.SimpleNamespace(_init_data_ready=None)
    with pytest.raises(RuntimeError, match="dual_mode"):
        mvae.MotionVAEPlayer.reset_dual_flagged(single, torch.zeros(4, dtype=torch.long))
    dev = torch.device("cpu")
    p = types.SimpleNamespace(_init_data_ready=torch.zeros(4, 288), _init_data_serve=torch.ones(4, 288), num_envs=4, device=dev, cfg={"serve_from": "far"}, _is_dual=True,
                              _joint_pos_bind_rel=torch.zeros(2, 24, 3), _dual_init_tables={})
    p.dual_init_table = lambda serve_from=None: mvae.MotionVAEPlayer.dual_init_table(p, serve_from)
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(6, dtype=torch.long), [0, 0, 0, 0]):
        with pytest.raises(RuntimeError, match="flags must be"):
            mvae.MotionVAEPlayer.reset_dual_flagged(p, bad)
    with pytest.raises(RuntimeError, match="root_xy must be"):
        mvae.MotionVAEPlayer.reset_dual_flagged(p, torch.zeros(4, dtype=torch.long), torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match="prefix count"):
        mvae.MotionVAEPlayer.reset_dual_flagged(p, torch.zeros(4, dtype=torch.long))
    # the parity table: with 'far' the odd env of a pair receives (the ready frame), with 'near' the even env
    assert p.dual_init_table()[:, 0].tolist() == [1, 0, 1, 0] and p.dual_init_table("near")[:, 0].tolist() == [0, 1, 0, 1]
    assert p.dual_init_table("near") is p.dual_init_table("near"), "the table is built once"
    with pytest.raises(ValueError, match="serve_from"):
        p.dual_init_table("left")
    with pytest.raises(TypeError, match="DualTennisControllerTask"):
        match.MatchPlayer(object(), object())
    assert match.RESET_MODES == ("ids", "flags")
    import inspect

    assert inspect.signature(match.MatchPlayer.__init__).parameters["reset_mode"].default == "ids"
