"""What the imitation-target tests share: the fixture tests/golden/mvae_target.npz (recorded from the reference by
tools/gen_golden_mvae_target.py), the settings of its two variants and the tolerance rule of tests/mvae_fixture.py.

Tolerances are measured, not chosen: the fixture stores `scatter/<kind>/<name>` = max |reference in float32 - reference in float64| per
quantity; the kernel and the numpy statement, which order a product's sums their own way, are allowed ORDER_ALLOWANCE x that.  A
quantity whose scatter is 0 must match exactly.
"""
import os

import numpy as np

from tests.mvae_fixture import ORDER_ALLOWANCE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mvae_target.npz")
VARIANTS = ("H", "P")
KEY_BODIES = ("R_Ankle", "L_Ankle", "L_Hand", "R_Hand")
DT = 1.0 / 30.0
PIECES = ("root_pos", "root_rot", "dof_pos", "root_vel", "root_ang_vel", "dof_vel", "key_pos", "rb_pos", "rb_rot")

_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def model():
    if "m" not in _cache:
        from vid2player3d_amd.model import load_baked_model

        _cache["m"] = load_baked_model()
    return _cache["m"]


def settings(g, v, **env):
    """target_settings of variant v: `<v>/settings` = [fix_head_orientation, body shapes, residual root]."""
    from vid2player3d_amd import mvae_target

    fix, _, res = (int(x) for x in g[v + "/settings"])
    m = model()
    keys = [list(m.body_names).index(b) for b in KEY_BODIES]
    return mvae_target.target_settings({"fix_head_orientation": bool(fix), "add_residual_root": bool(res)}, env, DT, m.body_names, m.parents, keys)


def steps(g, v):
    return len(g[v + "/in/ball_pos"])


def step_inputs(g, v, t, prev_target=None):
    """What step t of variant v reads, under the names target_step_reference takes; the previous target is the recorded one."""
    res = g.get(v + "/in/residual_root")
    return dict(root_pos=g[v + "/in/root_pos"][t + 1], joint_rotmat=g[v + "/in/joint_rotmat"][t + 1], residual_root=None if res is None else res[t],
                ball_pos=g[v + "/in/ball_pos"][t], sim_root_pos=g[v + "/in/sim_root_pos"][t], joint_pos_bind=g[v + "/joint_pos_bind"],
                env_shape_id=g[v + "/env_shape_id"], prev_target=g[v + "/target"][t] if prev_target is None else prev_target)


def reset_inputs(g, v):
    return dict(root_pos=g[v + "/in/root_pos"][0], joint_rotmat=g[v + "/in/joint_rotmat"][0], joint_pos_bind=g[v + "/joint_pos_bind"], env_shape_id=g[v + "/env_shape_id"])


def expected_rotmat(g, v, t, st):
    """joint_rotmat after step t: the input with the recorded Head and Neck."""
    m = g[v + "/in/joint_rotmat"][t + 1].copy()
    if st["fix_head_orientation"]:
        m[:, [st["smpl_head"], st["smpl_neck"]]] = g[v + "/out/head_neck_rotmat"][t]
    return m


def scatter_of(g, kind):
    p = "scatter/%s/" % kind
    s = {k[len(p):]: float(x) for k, x in g.items() if k.startswith(p)}
    if "rb_pos" in s:
        s["key_pos"] = s["rb_pos"]  # (key_pos is a copy of rows of rb_pos)
    return s


def assert_close(got, want, scatter, what):
    """|got - want| <= ORDER_ALLOWANCE x scatter (exactly equal where the scatter is 0); prints the figure first."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s != %s" % (what, got.shape, want.shape)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    tol = ORDER_ALLOWANCE * float(scatter)
    print("%s: max |difference| %.3g, allowance %.3g" % (what, err, tol))
    assert np.isfinite(got).all(), "%s is not finite" % what
    assert err <= tol, "%s differs by %.3g > %g x scatter %.3g" % (what, err, ORDER_ALLOWANCE, float(scatter))


def assert_row(got, want, scatter, what):
    """A packed row [n,331] piece by piece, each against its own scatter."""
    from vid2player3d_amd.mvae_target import SLICES

    for k in PIECES:
        a, b = SLICES[k]
        assert_close(np.asarray(got)[:, a:b], np.asarray(want)[:, a:b], scatter[k], "%s: %s" % (what, k))
