"""CPU checks of the imitation target from the motion generator's pose: the numpy statement against the fixture recorded from the
reference, the C ABI's refusals, the Python refusals, the packed row's slices."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import mvae_target_fixture as FX
from vid2player3d_amd import _lib
from vid2player3d_amd import mvae_target as mt


def _run(g, v, dt, free):
    """The numpy statement over variant v: rows [T+1,n,331] (the first is the reset's) and the joint matrices after every step."""
    st = FX.settings(g, v)
    n = len(g[v + "/env_shape_id"])
    rows = [mt.target_reset_reference(st, dict(FX.reset_inputs(g, v), target=np.zeros((n, mt.ROW), dt)), np.arange(n), dt)["target"]]
    mats = []
    for t in range(FX.steps(g, v)):
        o = mt.target_step_reference(st, FX.step_inputs(g, v, t, rows[-1] if free else None), dt)
        rows.append(o["target"])
        mats.append(o["joint_rotmat"])
    return st, rows, mats


@pytest.mark.parametrize("v", FX.VARIANTS)
def test_numpy_statement_reproduces_the_reset(v):
    g = FX.golden()
    _, rows, _ = _run(g, v, np.float32, True)
    FX.assert_close(rows[0], g[v + "/target"][0], FX.scatter_of(g, "reset")["target"], "variant %s reset row" % v)
    a, b = mt.SLICES["root_vel"][0], mt.SLICES["dof_vel"][1]
    assert not rows[0][:, a:mt.SLICES["root_ang_vel"][1]].any() and not rows[0][:, mt.SLICES["dof_vel"][0]:b].any()


@pytest.mark.parametrize("kind", ["step", "free"])
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_numpy_statement_reproduces_every_step(v, kind):
    g = FX.golden()
    st, rows, mats = _run(g, v, np.float32, kind == "free")
    sc = FX.scatter_of(g, kind)
    for t in range(FX.steps(g, v)):
        FX.assert_row(rows[t + 1], g[v + "/target"][t + 1], sc, "variant %s %s step %d" % (v, kind, t))
        FX.assert_close(mats[t], FX.expected_rotmat(g, v, t, st), sc["joint_rotmat"], "variant %s %s step %d: joint_rotmat" % (v, kind, t))


@pytest.mark.parametrize("kind", ["step", "free"])
@pytest.mark.parametrize("v", FX.VARIANTS)
def test_numpy_statement_in_float64_stays_within_the_scatter(v, kind):
    """in double precision the statement is the reference in double precision: within the recorded scatter of the float32 record,
    teacher-forced and feeding its own previous target, the written-back Head and Neck included"""
    g = FX.golden()
    st, rows, mats = _run(g, v, np.float64, kind == "free")
    once = (1.0 + 1e-6) / FX.ORDER_ALLOWANCE  # (the scatter itself, not the allowance for another order of the sums)
    sc = {k: x * once for k, x in FX.scatter_of(g, kind).items()}
    FX.assert_close(rows[0], g[v + "/target"][0], FX.scatter_of(g, "reset")["target"] * once, "variant %s reset row, float64" % v)
    for t in range(FX.steps(g, v)):
        what = "variant %s %s step %d, float64" % (v, kind, t)
        FX.assert_row(rows[t + 1], g[v + "/target"][t + 1], sc, what)
        FX.assert_close(mats[t], FX.expected_rotmat(g, v, t, st), sc["joint_rotmat"], what + ": joint_rotmat")


def test_numpy_statement_reproduces_the_pd_targets():
    g = FX.golden()
    for base in mt.PD_TARGET_BASES:
        for no_scale in (False, True):
            st = FX.settings(g, "H", pd_target_base=base, no_scale_action=no_scale)
            ds = np.stack([g["actions/dof_pos"], np.zeros_like(g["actions/dof_pos"])], -1)
            for dt, allow in ((np.float32, 1.0), (np.float64, (1.0 + 1e-6) / FX.ORDER_ALLOWANCE)):
                got = mt.target_actions_reference(st, g["actions/in"], g["actions/target"], ds, g["actions/pd_action_scale"], g["actions/pd_action_offset"], dt)
                name = "%s/%d" % (base, int(no_scale))
                FX.assert_close(got[:, :69], g["actions/out/" + name], allow * FX.scatter_of(g, "actions")[name], "pd targets %s %s" % (name, dt.__name__))
                assert np.array_equal(got[:, 69:], g["actions/in"][:, 69:].astype(dt))


def test_reset_reference_touches_only_the_named_rows():
    g = FX.golden()
    st = FX.settings(g, "H")
    n = len(g["H/env_shape_id"])
    rng = np.random.default_rng(5)
    before = dict(target=rng.normal(size=(n, mt.ROW)), root_states=rng.normal(size=(n, 13)), dof_state=rng.normal(size=(n, 69, 2)), rb_state=rng.normal(size=(n, 24, 13)))
    before = {k: x.astype(np.float32) for k, x in before.items()}
    ids = [3, n, 0, -1, n - 1, 6]
    got = mt.target_reset_reference(st, dict(FX.reset_inputs(g, "H"), **before), ids)
    named = [3, 0, n - 1, 6]
    others = [e for e in range(n) if e not in named]
    for k, x in before.items():
        assert np.array_equal(got[k][others], x[others]), k
    FX.assert_close(got["target"][named], g["H/target"][0][named], FX.scatter_of(g, "reset")["target"], "reset rows")
    row = mt.unpack_row(got["target"][named])
    assert np.array_equal(got["root_states"][named, :3], row["root_pos"]) and np.array_equal(got["root_states"][named, 3:7], row["root_rot"])
    assert not got["root_states"][named, 7:].any() and not got["dof_state"][named][..., 1].any() and not got["rb_state"][named][..., 7:].any()
    assert np.array_equal(got["dof_state"][named][..., 0], row["dof_pos"])
    assert np.array_equal(got["rb_state"][named][..., 0:3].reshape(4, 72), row["rb_pos"]) and np.array_equal(got["rb_state"][named][..., 3:7].reshape(4, 96), row["rb_rot"])


def test_packed_row_slices_are_the_tasks():
    from vid2player3d_amd.tasks import HumanoidSMPLIM

    assert {k: (a, b) for k, (a, b, _) in HumanoidSMPLIM._SLICES.items()} == mt.SLICES
    assert max(b for _, b in mt.SLICES.values()) == mt.ROW == _lib.MOTION_STATE_DIM


def test_tree_comes_from_the_body_model():
    m = FX.model()
    parents, of_body = mt.tree_from_model(m.body_names, m.parents)
    assert parents == [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]  # (SMPL's kinematic tree)
    assert [list(m.body_names)[b] for b in range(24)] == [mt.SMPL_JOINT_NAMES[s] for s in of_body]
    with pytest.raises(ValueError, match="SMPL joint names"):
        mt.tree_from_model(list(m.body_names)[:-1] + ["Tail"], m.parents)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    from vid2player3d_amd import build

    lib = C.CDLL(build.build())
    lib.v2p_last_error.restype = C.c_char_p
    vp = C.c_void_p
    lib.v2p_mvae_target_step.argtypes = [C.POINTER(_lib.MvaeTargetCfg), C.c_int64, C.POINTER(_lib.MvaeTargetBuffers), vp]
    lib.v2p_mvae_target_reset.argtypes = [C.POINTER(_lib.MvaeTargetCfg), C.c_int64, C.POINTER(_lib.MvaeTargetBuffers), vp, C.c_int64, vp]
    lib.v2p_mvae_target_actions.argtypes = [C.POINTER(_lib.MvaeTargetCfg), C.c_int64, vp, C.POINTER(_lib.MvaeTargetBuffers), vp, vp]
    return lib


def _bufs(**changes):
    """a struct's worth of non-null (never dereferenced: every call below is refused before any HIP call) pointers, all different"""
    d = {k: 0x1000 * (i + 1) for i, k in enumerate(_lib.MVAE_TARGET_BUFFER_NAMES)}
    d.update(changes)
    return _lib.MvaeTargetBuffers(**d)


def test_bad_arguments_are_refused_without_a_gpu(lib):
    g = FX.golden()
    st = FX.settings(g, "H")
    cfg, p = mt.cfg_struct(st, 2), C.c_void_p(0x1000)

    def step(c=cfg, n=4, b=_bufs()):
        return lib.v2p_mvae_target_step(C.byref(c) if c else None, n, C.byref(b) if b else None, None)

    def reset(c=cfg, num=4, b=_bufs(), ids=p, n=2):
        return lib.v2p_mvae_target_reset(C.byref(c) if c else None, num, C.byref(b) if b else None, ids, n, None)

    def actions(c=cfg, n=4, b=_bufs(), a=p, out=p):
        return lib.v2p_mvae_target_actions(C.byref(c) if c else None, n, a, C.byref(b) if b else None, out, None)

    def refused(rc, fn, word):
        assert rc == -1
        msg = lib.v2p_last_error().decode()
        assert msg.startswith(fn + ":") and word in msg, msg

    def changed(**fields):
        c = mt.cfg_struct(st, 2)
        for k, x in fields.items():
            if isinstance(x, tuple):
                getattr(c, k)[x[0]] = x[1]
            else:
                setattr(c, k, x)
        return c

    for fn, call in (("v2p_mvae_target_step", step), ("v2p_mvae_target_reset", reset), ("v2p_mvae_target_actions", actions)):
        refused(call(c=None), fn, "null")
        refused(call(b=None), fn, "null")
        refused(call(c=changed(dt=0.0)), fn, "dt")
        refused(call(c=changed(dt=-1.0)), fn, "dt")
        refused(call(c=changed(head_body=24)), fn, "outside 0..23")
        refused(call(c=changed(smpl_neck=-1)), fn, "outside 0..23")
        refused(call(c=changed(key_bodies=(2, 24))), fn, "key body")
        refused(call(c=changed(key_bodies=(0, -1))), fn, "key body")
        refused(call(c=changed(smpl_parents=(5, 7))), fn, "smpl_parents")
        refused(call(c=changed(smpl_parents=(0, 0))), fn, "smpl_parents")
        refused(call(c=changed(smpl_of_body=(3, 24))), fn, "smpl_of_body")
        refused(call(c=changed(smpl_of_body=(3, 4))), fn, "permutation")
        refused(call(c=changed(num_shapes=0)), fn, "num_shapes")
    refused(step(n=-1), "v2p_mvae_target_step", "n -1")
    refused(reset(n=-2), "v2p_mvae_target_reset", "n -2")
    refused(actions(n=-3), "v2p_mvae_target_actions", "n -3")
    for name in ("root_pos", "joint_rotmat", "joint_pos_bind", "target", "prev_target"):
        refused(step(b=_bufs(**{name: None})), "v2p_mvae_target_step", "null")
    refused(step(b=_bufs(prev_target=0x7000)), "v2p_mvae_target_step", "same buffer")  # (0x7000 is `target`)
    refused(step(b=_bufs(ball_state=None)), "v2p_mvae_target_step", "ball_state")
    refused(step(b=_bufs(rb_state=None)), "v2p_mvae_target_step", "rb_state")
    plain = mt.cfg_struct(FX.settings(g, "P"), 1)
    optional = dict(ball_state=None, rb_state=None, residual_root=None, env_shape_id=None, root_states=None, dof_state=None, hold_reset=None, hold_progress=None,
                    hold_cur_time=None, pd_action_scale=None, pd_action_offset=None)
    assert step(c=plain, n=0, b=_bufs(**optional)) == 0  # (without the head rule the step needs neither the ball nor the simulated state)
    refused(reset(num=-1), "v2p_mvae_target_reset", "num_envs")
    refused(reset(ids=None), "v2p_mvae_target_reset", "env_ids")
    refused(reset(b=_bufs(target=None)), "v2p_mvae_target_reset", "null")
    assert reset(n=0, b=_bufs(prev_target=None, **{k: None for k in optional})) == 0 and reset(num=0) == 0
    refused(actions(c=changed(pd_target_base=3)), "v2p_mvae_target_actions", "pd_target_base")
    refused(actions(c=changed(pd_target_base=-1)), "v2p_mvae_target_actions", "pd_target_base")
    refused(actions(b=_bufs(target=None)), "v2p_mvae_target_actions", "null")
    refused(actions(c=changed(pd_target_base=1), b=_bufs(dof_state=None)), "v2p_mvae_target_actions", "null")
    refused(actions(c=changed(pd_target_base=2), b=_bufs(pd_action_offset=None)), "v2p_mvae_target_actions", "null")
    refused(actions(b=_bufs(pd_action_scale=None)), "v2p_mvae_target_actions", "pd_action_scale")
    refused(actions(a=None), "v2p_mvae_target_actions", "actions")
    refused(actions(out=None), "v2p_mvae_target_actions", "actions")
    assert actions(c=changed(no_scale_action=1), n=0, b=_bufs(pd_action_scale=None)) == 0
    assert step(n=0) == 0 and actions(n=0) == 0


def test_struct_sizes_match_the_header():
    import os
    import subprocess
    import tempfile

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = '#include <stdio.h>\n#include "v2p_rollout.h"\nint main(void){ printf("%zu %zu\\n", sizeof(v2p_mvae_target_cfg), sizeof(v2p_mvae_target_buffers)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(repo, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(_lib.MvaeTargetCfg), C.sizeof(_lib.MvaeTargetBuffers)]


def test_settings_refuse_what_is_not_built():
    m = FX.model()
    keys = [1, 2, 3, 4]
    with pytest.raises(NotImplementedError, match="dual_mode"):
        mt.target_settings({"dual_mode": "different"}, {}, FX.DT, m.body_names, m.parents, keys)
    with pytest.raises(NotImplementedError, match="obs_type"):
        mt.target_settings({}, {"obs_type": "joint_pos"}, FX.DT, m.body_names, m.parents, keys)
    with pytest.raises(ValueError, match="pd_target_base"):
        mt.target_settings({}, {"pd_target_base": "rest_pos"}, FX.DT, m.body_names, m.parents, keys)
    with pytest.raises(ValueError, match="key bodies"):
        mt.target_settings({}, {}, FX.DT, m.body_names, m.parents, keys[:3])


def test_a_cpu_device_raises():
    task = types.SimpleNamespace(device="cpu", num_envs=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mt.ImitationTarget(task, None, np.zeros((24, 3)), {})
