"""Readers of tests/golden/tennis_dual.npz (tools/gen_golden_tennis_dual.py) shared by the CPU and the GPU tests of the two-player rally:
settings, state before and after the step (`step`) and the hand-over (`hand`) of a variant under the names of the buffers, rows tiled to
a batch size, and the comparison both tests hold their subject to - flags, integers, cursors and indices exact, copies / negations /
gathers bit for bit, every other float within ORDER_ALLOWANCE x the scatter the generator recorded (the rule of DESIGN 8 items 8, 9)."""
import os

import numpy as np

from vid2player3d_amd.tasks import tennis_controller_dual as td

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tennis_dual.npz")
VARIANTS = ("A", "B")
ORDER_ALLOWANCE = 8.0
GRIP_NAMES = ("eastern", "semi_western")
# parts of float arrays that are copies, negations or gathers: (columns of the last axis) compared bit for bit
BITWISE = {"ball_state": (0, 1, 3, 4, 5, 6), "ball_traj": (2,)}
_cache = {}


def golden():
    if "d" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["d"] = {k: z[k] for k in z.files}
    return _cache["d"]


def variant(name):
    rt, hist, target, vel, g0, g1, different = [int(x) for x in golden()[name + "/settings"]]
    return dict(reward_type=("reach", "return", "return_w_estimate")[rt], history=bool(hist), target=bool(target), velocity=bool(vel),
                grips=(GRIP_NAMES[g0], GRIP_NAMES[g1]), different=bool(different))


def settings(name):
    d, v = golden(), variant(name)
    return td.dual_settings(grip=list(v["grips"]), in_grids=d["in_grids"], reward_type=v["reward_type"], obs_ball_traj_length=10, use_history_ball_obs=v["history"],
                            use_random_ball_target=v["target"], contact_by_velocity=v["velocity"],
                            reward_scales=dict(zip(("pos", "phase", "bounce_pos", "bounce_time"), d["scales"])), reward_weights={"pos": d["weights"][0], "ball_pos": d["weights"][1]})


def num_envs(kind, name):
    return len(golden()["%s/%s/pre/ball_state" % (kind, name)])


def _rows(n, n0):
    return np.arange(n) % n0  # (n0 is even: pairs and parities survive the tiling)


def inputs(kind, name, n=None):
    """The state before the `step` / the `hand`-over of a variant: every array the launch reads, rows tiled to n envs."""
    d, n0 = golden(), num_envs(kind, name)
    r = _rows(n0 if n is None else n, n0)
    p = "%s/%s/pre/" % (kind, name)
    s = {k[len(p):]: v[r].copy() for k, v in d.items() if k.startswith(p)}
    s["rb_state"], s["racket_state"] = d["rb_state"][r].copy(), d["racket_state"][r].copy()
    s["traj_in"] = d["traj_in"]
    if variant(name)["history"]:
        s.setdefault("ball_traj", None)
        s.setdefault("traj_cursor", None)
    return s


def expected(kind, name, n=None):
    d, n0 = golden(), num_envs(kind, name)
    r = _rows(n0 if n is None else n, n0)
    p = "%s/%s/post/" % (kind, name)
    skip = ("ball_traj", "traj_cursor") if variant(name)["history"] else ()
    return {k[len(p):]: v[r] for k, v in d.items() if k.startswith(p) and k[len(p):] not in skip}


def scatter(kind):
    p = "scatter/%s/" % kind
    return {k[len(p):]: float(v) for k, v in golden().items() if k.startswith(p)}


def compare(got, want, sc, what, rows=None):
    """Prints each float figure before it asserts."""
    for k, w in want.items():
        a = np.asarray(got[k]).reshape(np.asarray(w).shape)
        if rows is not None:
            a, w = a[rows], w[rows]
        if np.asarray(w).dtype.kind in "iub":
            assert np.array_equal(a.astype(w.dtype), w), "%s: %s differs at rows %s" % (what, k, np.nonzero((a.astype(w.dtype) != w).reshape(len(w), -1).any(1))[0][:8])
            continue
        for col in BITWISE.get(k, ()):
            assert np.array_equal(a[..., col], w[..., col]), "%s: %s[..., %d] is a copy / negation / gather and differs in its bits" % (what, k, col)
        tol = ORDER_ALLOWANCE * sc[k]
        err = float(np.abs(a.astype(np.float64) - np.asarray(w, dtype=np.float64)).max()) if a.size else 0.0
        print("%s: %s max |difference| %.3g, allowance %.3g" % (what, k, err, tol))
        assert np.isfinite(a).all(), "%s: %s is not finite" % (what, k)
        assert err <= tol, "%s: %s differs by %.3g > %g x scatter %.3g" % (what, k, err, ORDER_ALLOWANCE, sc[k])
