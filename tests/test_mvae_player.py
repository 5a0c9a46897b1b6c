"""CPU checks of the MotionVAE motion generator: the numpy statement against the fixture recorded from the reference, the C ABI's
refusals, the struct mirrors, the weight helper."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import mvae_fixture as FX
from vid2player3d_amd import _lib, mvae

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seeded_weights_have_the_recorded_sha256():
    sd, avg, std = FX.seeded_state_dict()
    assert FX.weights_sha256(sd, avg, std) == FX.golden()["weights_sha256"].tobytes().decode()
    w = mvae.weights_from_state_dict(sd)
    assert w["w0"].shape == (6, 320, 256) and w["w2"].shape == (6, 288, 290) and w["gate_w2"].shape == (6, 64)
    assert sum(x.nbytes for x in w.values()) > 5.5e6  # (why they are not stored)


def test_weights_from_state_dict_refuses_another_architecture():
    sd, _, _ = FX.seeded_state_dict()
    bad = dict(sd)
    bad["decoder.w1"] = sd["decoder.w1"][:, :, :128]
    with pytest.raises(ValueError, match="w1"):
        mvae.weights_from_state_dict(bad)
    del bad["decoder.w1"]
    with pytest.raises(KeyError, match="decoder.w1"):
        mvae.weights_from_state_dict(bad)


def test_packed_matrix_layout():
    """element q of lane l of column tile t, k-group g is W[e][8g + 2q + (l>>5)][32t + (l&31)], zero past the last column"""
    rng = np.random.default_rng(0)
    W = rng.normal(size=(2, 16, 40)).astype(np.float32)
    P = mvae.pack_matrix(W)
    assert P.shape == (2, 2, 2, 64, 4)
    for e, t, g, l, q in ((0, 0, 0, 0, 0), (1, 1, 1, 37, 3), (0, 1, 0, 7, 2), (1, 0, 1, 63, 1), (0, 1, 1, 40, 0)):
        k, col = 8 * g + 2 * q + (l >> 5), 32 * t + (l & 31)
        assert P[e, t, g, l, q] == (W[e, k, col] if col < 40 else 0.0)


@pytest.mark.parametrize("v", FX.VARIANTS)
def test_numpy_statement_reproduces_the_reset(v):
    g = FX.golden()
    w, avg, std = FX.weights()
    st = FX.settings(g, v)
    want = {k[len(v + "/reset/"):]: x for k, x in g.items() if k.startswith(v + "/reset/")}
    n = len(want["root_pos"])
    zero = {k: np.zeros_like(x) for k, x in want.items()}
    got = mvae.mvae_reset_reference(st, avg, std, zero, np.arange(n), g[v + "/init_feature"], g[v + "/root_xy"], g["joint_pos_bind_rel"])
    FX.assert_state(got, want, FX.scatter_of(g, "reset"), "variant %s reset" % v)


@pytest.mark.parametrize("v", FX.VARIANTS)
def test_numpy_statement_reproduces_every_step(v):
    g = FX.golden()
    w, avg, std = FX.weights()
    st = FX.settings(g, v)
    steps = len(g[v + "/latents"])
    assert steps >= 5
    for t in range(steps):
        got = mvae.mvae_step_reference(st, w, avg, std, FX.state_before(g, v, t), g[v + "/latents"][t], g[v + "/residual"][t])
        FX.assert_state(got, FX.state_after(g, v, t), FX.scatter_of(g, "step"), "variant %s step %d" % (v, t))


def test_reset_reference_skips_ids_outside_the_batch():
    g = FX.golden()
    _, avg, std = FX.weights()
    st = FX.settings(g, "A")
    want = {k[len("A/reset/"):]: x for k, x in g.items() if k.startswith("A/reset/")}
    zero = {k: np.full_like(x, -7) for k, x in want.items()}
    ids = np.array([2, len(want["root_pos"]), -1, 5])
    got = mvae.mvae_reset_reference(st, avg, std, zero, ids, g["A/init_feature"][[2, 0, 1, 5]], g["A/root_xy"][[2, 0, 1, 5]], g["joint_pos_bind_rel"])
    others = [e for e in range(len(want["root_pos"])) if e not in (2, 5)]
    for k in ("conditions", "root_pos", "joint_rotmat", "racket_pos", "swing_type"):
        assert np.array_equal(got[k].reshape(zero[k].shape)[others], zero[k][others])
    FX.assert_state(got, {k: x for k, x in want.items() if k not in ("phase_pred", "joint_rot")}, FX.scatter_of(g, "reset"), "reset of two ids", rows=[2, 5])


def test_struct_sizes_match_the_header():
    prog = '#include <stdio.h>\n#include "v2p_rollout.h"\nint main(void){ printf("%zu %zu %zu\\n", sizeof(v2p_mvae_cfg), sizeof(v2p_mvae_weights), sizeof(v2p_mvae_buffers)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(_lib.MvaeCfg), C.sizeof(_lib.MvaeWeights), C.sizeof(_lib.MvaeBuffers)]


@pytest.fixture(scope="module")
def lib():
    from vid2player3d_amd import build

    lib = C.CDLL(build.build())
    lib.v2p_last_error.restype = C.c_char_p
    vp = C.c_void_p
    lib.v2p_mvae_step.argtypes = [C.POINTER(_lib.MvaeCfg), C.c_int64, C.POINTER(_lib.MvaeWeights), C.POINTER(_lib.MvaeBuffers), vp, vp, vp]
    lib.v2p_mvae_reset.argtypes = [C.POINTER(_lib.MvaeCfg), C.c_int64, C.POINTER(_lib.MvaeWeights), C.POINTER(_lib.MvaeBuffers), vp, C.c_int64, vp, vp, vp, vp]
    return lib


def _full(names):
    """a struct's worth of non-null (never dereferenced: every call below is refused before any HIP call) pointers"""
    return {k: 0x1000 for k in names}


def test_bad_arguments_are_refused_without_a_gpu(lib):
    st = mvae.player_settings({"player": "federer", "add_residual_dof": "euler"}, True)
    cfg, w, b = mvae.cfg_struct(st), _lib.MvaeWeights(**_full(_lib.MVAE_WEIGHT_NAMES)), _lib.MvaeBuffers(**_full(_lib.MVAE_BUFFER_NAMES))
    p = C.c_void_p(0x1000)

    def step(c=cfg, n=4, ww=w, bb=b, z=p, r=None):
        return lib.v2p_mvae_step(C.byref(c) if c else None, n, C.byref(ww) if ww else None, C.byref(bb) if bb else None, z, r, None)

    def reset(c=cfg, num=4, ww=w, bb=b, ids=p, n=2, f=p, xy=p, bind=p):
        return lib.v2p_mvae_reset(C.byref(c) if c else None, num, C.byref(ww) if ww else None, C.byref(bb) if bb else None, ids, n, f, xy, bind, None)

    def refused(rc, fn, word):
        assert rc == -1
        msg = lib.v2p_last_error().decode()
        assert msg.startswith(fn + ":") and word in msg, msg

    for fn, call in (("v2p_mvae_step", step), ("v2p_mvae_reset", reset)):
        refused(call(c=None), fn, "null")
        refused(call(ww=None), fn, "null")
        refused(call(bb=None), fn, "null")
        for field, value in (("hidden_size", 128), ("num_experts", 4), ("frame_size", 286), ("latent_size", 16), ("gate_hidden_size", 32), ("num_condition_frames", 2),
                             ("num_future_predictions", 2), ("predict_phase", 0)):
            other = mvae.cfg_struct(st)
            setattr(other, field, value)
            refused(call(c=other), fn, "shipped architecture")
        other = mvae.cfg_struct(st)
        other.player = 3
        refused(call(c=other), fn, "player")
        nb = _lib.MvaeBuffers(**dict(_full(_lib.MVAE_BUFFER_NAMES), conditions=None))
        refused(call(bb=nb), fn, "null")
        nw = _lib.MvaeWeights(**dict(_full(_lib.MVAE_WEIGHT_NAMES), std=None))
        refused(call(ww=nw), fn, "null")
    refused(step(n=-1), "v2p_mvae_step", "n -1")
    refused(step(z=None), "v2p_mvae_step", "latents")
    refused(step(ww=_lib.MvaeWeights(**dict(_full(_lib.MVAE_WEIGHT_NAMES), gate_w1=None))), "v2p_mvae_step", "null")
    plain = mvae.cfg_struct(mvae.player_settings({"player": "federer"}, True))
    refused(step(c=plain, r=p), "v2p_mvae_step", "add_residual_dof")
    ev = mvae.cfg_struct(mvae.player_settings({"player": "nadal"}, False))  # (evaluation writes joint_rot)
    refused(step(c=ev, bb=_lib.MvaeBuffers(**dict(_full(_lib.MVAE_BUFFER_NAMES), joint_rot=None))), "v2p_mvae_step", "null")
    refused(reset(n=-2), "v2p_mvae_reset", "n -2")
    refused(reset(num=-1), "v2p_mvae_reset", "num_envs")
    refused(reset(ids=None), "v2p_mvae_reset", "env_ids")
    refused(reset(bind=None), "v2p_mvae_reset", "joint_pos_bind_rel")
    refused(reset(bb=_lib.MvaeBuffers(**dict(_full(_lib.MVAE_BUFFER_NAMES), racket_pos=None))), "v2p_mvae_reset", "null")
    # nothing to do: no HIP call either
    assert step(n=0) == 0 and reset(n=0) == 0 and reset(num=0) == 0
    # the training step needs no joint_rot, the reset needs no decoder weights
    assert step(n=0, bb=_lib.MvaeBuffers(**dict(_full(_lib.MVAE_BUFFER_NAMES), joint_rot=None))) == 0
    assert reset(n=0, ww=_lib.MvaeWeights(avg=0x1000, std=0x1000)) == 0


def test_a_cpu_device_raises():
    sd, avg, std = FX.seeded_state_dict()
    g = FX.golden()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mvae.MotionVAEPlayer({"player": "federer"}, 4, mvae.weights_from_state_dict(sd), avg, std, g["A/init_feature"], g["joint_pos_bind_rel"], True, "cpu")


def test_settings_refuse_what_is_not_built():
    with pytest.raises(NotImplementedError, match="dual_mode"):
        mvae.player_settings({"player": "federer", "dual_mode": "different"}, True)
    with pytest.raises(NotImplementedError, match="shipped architecture"):
        mvae.player_settings({"player": "federer", "hidden_size": 512}, True)
    with pytest.raises(ValueError, match="player"):
        mvae.player_settings({"player": "murray"}, True)
