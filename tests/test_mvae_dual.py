"""CPU checks of the two-player motion generator: the numpy statements against the fixture recorded from the reference's
`dual_mode: different` (float32 within ORDER_ALLOWANCE x the recorded scatter, float64 within the scatter itself), the settings and
their refusals, the C ABI's refusals, the struct mirror, the weights of two sets."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import mvae_dual_fixture as DX
from tests import mvae_fixture as FX
from vid2player3d_amd import _lib, mvae

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = list(DX.VARIANTS)
ZERO_SHAPES = (("conditions", (1, FX.FRAME), np.float32), ("root_pos", (3,), np.float32), ("root_vel", (3,), np.float32), ("joint_rot6d", (24, 6), np.float32),
               ("joint_rotmat", (24, 3, 3), np.float32), ("joint_rot", (24, 3), np.float32), ("racket_pos", (3,), np.float32), ("racket_normal", (3,), np.float32),
               ("phase_pred", (), np.float32), ("swing_type", (), np.int64), ("swing_type_cycle", (), np.int64))


def zero_state():
    return {k: np.zeros((DX.N,) + shape, dt) for k, shape, dt in ZERO_SHAPES}


def assert_within_scatter(got, want, scatter, what):
    """the float64 evaluation against the recorded float32 values: within the float32 - float64 scatter itself (a millionth more)"""
    for k, w in want.items():
        a = np.asarray(got[k]).reshape(np.asarray(w).shape)
        if np.asarray(w).dtype.kind in "iub":
            assert np.array_equal(a, w), "%s: %s differs" % (what, k)
            continue
        err = float(np.abs(a.astype(np.float64) - np.asarray(w, dtype=np.float64)).max())
        print("%s: %s max |float64 statement - fixture| %.3g, scatter %.3g" % (what, k, err, scatter[k]))
        assert err <= scatter[k] * (1 + 1e-6) + 1e-12, "%s: %s differs by %.3g > the scatter %.3g" % (what, k, err, scatter[k])


def reset_want(g, v, st, prefix="reset"):
    return {k: g["%s/%s/%s" % (v, prefix, k)] for k in DX.RESET_STATE if k != "phase_pred" and (k != "joint_rot" or not st["is_train"])}


def test_the_two_seeded_weight_sets_have_the_recorded_sha256():
    g = DX.golden()
    for i, seed in enumerate(DX.WEIGHT_SEEDS):
        assert FX.weights_sha256(*FX.seeded_state_dict(seed)) == g["weights_sha256_%d" % i].tobytes().decode()
    (_, _), avg, std = DX.weights()
    assert not np.array_equal(std[0][:3], std[1][:3]) and not np.array_equal(avg[0][3:], avg[1][3:])


def test_player_settings_accept_different():
    st = mvae.player_settings(DX.cfg("A"), True, DX.N)
    assert st["dual"] and st["is_train"] and st["add_residual_dof"]
    assert [s["player"] for s in st["sides"]] == ["nadal", "federer"] and [s["righthand"] for s in st["sides"]] == [False, True]
    # serve_from 'far': the racket is side 0's (mvae_player.py:56-57) - nadal's left arm, semi-western
    assert st["racket"]["righthand"] is False and st["racket"]["grip"] == "semi_western"
    assert st["racket"]["direction"] == (-1.0, 0.0, 0.0) and np.allclose(st["racket"]["normal"], (0, 2 ** -0.5, 2 ** -0.5), atol=1e-7)
    near = mvae.player_settings(DX.cfg("C"), True, DX.N)["racket"]  # the default: side 1's - federer's right arm, eastern
    assert near["righthand"] is True and near["normal"] == (0.0, 1.0, 0.0)
    assert mvae.player_settings({k: x for k, x in DX.cfg("C").items() if k != "serve_from"}, True)["racket"] == near
    both = mvae.player_settings(dict(DX.cfg("B"), add_residual_dof=["euler", "euler"]), False)
    assert both["add_residual_dof"] and not both["is_train"]
    # the single player's settings are what they were
    assert mvae.player_settings({"player": "federer"}, True) == dict(player="federer", righthand=True, is_train=True, add_residual_dof=False)


def test_player_settings_refuse_with_a_message():
    cfg = DX.cfg("A")
    with pytest.raises(ValueError, match="list of two"):
        mvae.player_settings(dict(cfg, player=["nadal", "federer", "djokovic"]), True)
    with pytest.raises(ValueError, match="list of two"):
        mvae.player_settings(dict(cfg, righthand=[True]), True)
    with pytest.raises(ValueError, match="list of two"):
        mvae.player_settings(dict(cfg, grip=["eastern"]), True)
    with pytest.raises(ValueError, match="even num_envs"):
        mvae.player_settings(cfg, True, 7)
    with pytest.raises(ValueError, match="common to both"):
        mvae.player_settings(dict(cfg, add_residual_dof=["euler", None]), True)
    with pytest.raises(ValueError, match="grip"):
        mvae.player_settings(dict(cfg, grip=["western", "western"]), True)
    with pytest.raises(ValueError, match="player"):
        mvae.player_settings(dict(cfg, player=["nadal", "murray"]), True)
    with pytest.raises(NotImplementedError, match="dual_mode"):
        mvae.player_settings(dict(cfg, dual_mode="same"), True)


def test_whole_pairs():
    assert mvae.whole_pairs([2, 3, 8, 9]) and mvae.whole_pairs([]) and mvae.whole_pairs([0, 1])
    assert not mvae.whole_pairs([2, 3, 8]) and not mvae.whole_pairs([1, 2]) and not mvae.whole_pairs([2, 9]) and not mvae.whole_pairs([2, 3, 3, 4])


def test_pack_weights_of_two_sets():
    """each side's set is packed on its own, in the layout of the single player's"""
    (w0, w1), avg, std = DX.weights()
    assert not np.array_equal(w0["w1"], w1["w1"])
    for w in (w0, w1):
        P = mvae.pack_matrix(w["w2"])
        assert P.shape == (6, 10, 36, 64, 4)
        for e, t, g, l, q in ((0, 0, 0, 0, 0), (5, 9, 35, 63, 3), (2, 9, 7, 1, 2), (3, 4, 20, 40, 1)):
            k, col = 8 * g + 2 * q + (l >> 5), 32 * t + (l & 31)
            assert P[e, t, g, l, q] == (w["w2"][e, k, col] if col < 290 else 0.0)
    packed = [mvae.pack_weights(w, a, s, "cpu") for w, a, s in zip((w0, w1), avg, std)]
    assert set(packed[0]) == set(_lib.MVAE_WEIGHT_NAMES) and not np.array_equal(packed[0]["std"].numpy(), packed[1]["std"].numpy())
    assert packed[0]["w0"].shape == packed[1]["w0"].shape == (6, 8, 40, 64, 4)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("v", VARIANTS)
def test_numpy_statement_reproduces_both_resets(v, dt):
    g = DX.golden()
    _, avg, std = DX.weights()
    st = DX.settings(v)
    check = FX.assert_state if dt == np.float32 else assert_within_scatter
    ids, feature = DX.reset_inputs(g, v, g[v + "/reaction_ids"], g[v + "/recovery_ids"])
    got = mvae.mvae_dual_reset_reference(st, avg, std, zero_state(), ids, feature, g[v + "/root_xy"], g["joint_pos_bind_rel"], dt=dt)
    check(got, reset_want(g, v, st), FX.scatter_of(g, "reset"), "variant %s reset of all envs" % v)
    # four ids from the state after the last step: the pair at list positions 2i, 2i+1 reads bind row i; the other rows stay
    before = DX.state_before_part(g, v)
    ids, feature = DX.reset_inputs(g, v, DX.PART_REACTION, DX.PART_RECOVERY)
    assert ids.tolist() == list(DX.PART_IDS)
    got = mvae.mvae_dual_reset_reference(st, avg, std, before, ids, feature, g[v + "/part/root_xy"], g["joint_pos_bind_rel"], dt=dt)
    check({k: np.asarray(x)[list(DX.PART_IDS)] for k, x in got.items()}, reset_want(g, v, st, "part"), FX.scatter_of(g, "reset"), "variant %s reset of %s" % (v, ids.tolist()))
    others = [e for e in range(DX.N) if e not in DX.PART_IDS]
    for k, x in before.items():
        assert np.array_equal(np.asarray(got[k]).reshape(x.shape)[others], x[others]), "the reset statement wrote %s of an env it was not given" % k
    own_row = mvae.mvae_dual_reset_reference(st, avg, std, before, ids, feature, g[v + "/part/root_xy"], g["joint_pos_bind_rel"][[1, 4]], dt=dt)
    assert np.abs(own_row["racket_pos"][[8, 9]] - g[v + "/part/racket_pos"][2:]).max() > 1e-2, "the fixture does not tell which bind row a reset reads"


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("v", VARIANTS)
def test_numpy_statement_reproduces_every_step(v, dt):
    g = DX.golden()
    w, avg, std = DX.weights()
    st = DX.settings(v)
    check = FX.assert_state if dt == np.float32 else assert_within_scatter
    for t in range(DX.T):
        got = mvae.mvae_dual_step_reference(st, w, avg, std, DX.state_before(g, v, t), g[v + "/latents"][t], DX.residual(g, v, t), dt=dt)
        check(got, DX.state_after(g, v, t), FX.scatter_of(g, "step"), "variant %s step %d" % (v, t))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("v", VARIANTS)
def test_numpy_statement_free_run(v, dt):
    g = DX.golden()
    w, avg, std = DX.weights()
    st = DX.settings(v)
    check = FX.assert_state if dt == np.float32 else assert_within_scatter
    ids, feature = DX.reset_inputs(g, v, g[v + "/reaction_ids"], g[v + "/recovery_ids"])
    s = mvae.mvae_dual_reset_reference(st, avg, std, zero_state(), ids, feature, g[v + "/root_xy"], g["joint_pos_bind_rel"], dt=dt)
    s["swing_type"], s["swing_type_cycle"] = g[v + "/preset_swing"].copy(), g[v + "/preset_swing"].copy()
    for t in range(DX.T):
        o = mvae.mvae_dual_step_reference(st, w, avg, std, s, g[v + "/latents"][t], DX.residual(g, v, t), dt=dt)
        check(o, DX.state_after(g, v, t), FX.scatter_of(g, "free"), "variant %s free run, step %d" % (v, t))
        s = dict(s, **o)


def test_the_fixture_tells_the_root_column_quirk_from_its_absence():
    """the even rows' root columns, normalised with their OWN statistics, would miss the fixture by more than 100 x the allowance"""
    g = DX.golden()
    _, avg, std = DX.weights()
    allowance = FX.ORDER_ALLOWANCE * max(FX.scatter_of(g, "step")["conditions"], FX.scatter_of(g, "free")["conditions"])
    for v in VARIANTS:
        for t in range(1, DX.T + 1):
            own = (g[v + "/traj/root_pos"][t][0::2] - avg[0][:3]) / std[0][:3]
            assert np.abs(g[v + "/traj/conditions"][t][0::2, 0, :3] - own).max(1).min() > 100 * allowance


def test_struct_size_matches_the_header():
    prog = '#include <stdio.h>\n#include "v2p_rollout.h"\nint main(void){ printf("%zu %d %d\\n", sizeof(v2p_mvae_racket), V2P_MVAE_DUAL_MAP_PARITY, V2P_MVAE_DUAL_MAP_HALVES); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out == [C.sizeof(_lib.MvaeRacket), mvae.DUAL_MAP_PARITY, mvae.DUAL_MAP_HALVES]


@pytest.fixture(scope="module")
def lib():
    from vid2player3d_amd import build

    lib = C.CDLL(build.build())
    lib.v2p_last_error.restype = C.c_char_p
    lib.v2p_abi_version.restype = C.c_int
    vp = C.c_void_p
    lib.v2p_mvae_dual_step.argtypes = [C.POINTER(_lib.MvaeCfg), C.c_int64, C.POINTER(_lib.MvaeWeights), C.POINTER(_lib.MvaeBuffers), vp, vp, C.c_int32, vp]
    lib.v2p_mvae_dual_reset.argtypes = [C.POINTER(_lib.MvaeCfg), C.c_int64, C.POINTER(_lib.MvaeWeights), C.POINTER(_lib.MvaeBuffers), C.POINTER(_lib.MvaeRacket), vp, C.c_int64, vp, vp,
                                        vp, C.c_int64, vp]
    return lib


def test_bad_arguments_are_refused_without_a_gpu(lib):
    """every refusal comes before any HIP call (the pointers are never dereferenced)"""
    assert lib.v2p_abi_version() == 15
    full = lambda names: {k: 0x1000 for k in names}
    st = DX.settings("A")
    cfgs = lambda **change: (_lib.MvaeCfg * 2)(*(mvae.cfg_struct(dict(s, **{k: x[i] for k, x in change.items()})) for i, s in enumerate(st["sides"])))
    w = (_lib.MvaeWeights * 2)(_lib.MvaeWeights(**full(_lib.MVAE_WEIGHT_NAMES)), _lib.MvaeWeights(**full(_lib.MVAE_WEIGHT_NAMES)))
    b = _lib.MvaeBuffers(**full(_lib.MVAE_BUFFER_NAMES))
    racket, p = mvae.racket_struct(st["racket"]), C.c_void_p(0x1000)

    def step(c=cfgs(), n=4, ww=w, bb=b, z=p, r=None, mapping=0):
        return lib.v2p_mvae_dual_step(c, n, ww, C.byref(bb) if bb else None, z, r, mapping, None)

    def reset(c=cfgs(), num=4, ww=w, bb=b, rk=racket, ids=p, n=2, f=p, xy=p, bind=p, rows=1):
        return lib.v2p_mvae_dual_reset(c, num, ww, C.byref(bb) if bb else None, C.byref(rk) if rk else None, ids, n, f, xy, bind, rows, None)

    def refused(rc, fn, word):
        assert rc == -1
        msg = lib.v2p_last_error().decode()
        assert msg.startswith(fn + ":") and word in msg, msg

    for fn, call in (("v2p_mvae_dual_step", step), ("v2p_mvae_dual_reset", reset)):
        refused(call(c=None), fn, "null")
        refused(call(ww=None), fn, "null")
        refused(call(bb=None), fn, "null")
        refused(call(c=cfgs(is_train=(True, False))), fn, "disagree")
        refused(call(c=cfgs(add_residual_dof=(True, False))), fn, "disagree")
        other = cfgs()
        other[1].hidden_size = 128  # (the second side is checked like the first)
        refused(call(c=other), fn, "shipped architecture")
        other = cfgs()
        other[1].player = 3
        refused(call(c=other), fn, "player")
        second = (_lib.MvaeWeights * 2)(_lib.MvaeWeights(**full(_lib.MVAE_WEIGHT_NAMES)), _lib.MvaeWeights(**dict(full(_lib.MVAE_WEIGHT_NAMES), std=None)))
        refused(call(ww=second), fn, "null")
    refused(step(n=3), "v2p_mvae_dual_step", "odd")
    refused(step(n=-2), "v2p_mvae_dual_step", "n -2")
    refused(step(mapping=2), "v2p_mvae_dual_step", "mapping")
    refused(step(z=None), "v2p_mvae_dual_step", "latents")
    refused(step(c=cfgs(add_residual_dof=(False, False)), r=p), "v2p_mvae_dual_step", "add_residual_dof")
    second = (_lib.MvaeWeights * 2)(_lib.MvaeWeights(**full(_lib.MVAE_WEIGHT_NAMES)), _lib.MvaeWeights(**dict(full(_lib.MVAE_WEIGHT_NAMES), w1=None)))
    refused(step(ww=second), "v2p_mvae_dual_step", "null")
    refused(reset(rk=None), "v2p_mvae_dual_reset", "racket")
    refused(reset(num=-1), "v2p_mvae_dual_reset", "num_envs")
    refused(reset(ids=None), "v2p_mvae_dual_reset", "env_ids")
    refused(reset(bind=None), "v2p_mvae_dual_reset", "joint_pos_bind_rel")
    refused(reset(rows=0), "v2p_mvae_dual_reset", "rows")
    refused(reset(n=6, rows=2), "v2p_mvae_dual_reset", "rows")
    assert step(n=0) == 0 and reset(n=0) == 0 and reset(num=0) == 0 and reset(n=0, rows=3) == 0


def test_a_cpu_device_raises():
    g = DX.golden()
    w, avg, std = DX.weights()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mvae.MotionVAEPlayer(DX.cfg("A"), DX.N, w, avg, std, None, g["joint_pos_bind_rel"], True, "cpu", init_data_ready=list(g["A/init_ready"][:, None]),
                             init_data_serve=list(g["A/init_serve"][:, None]))
