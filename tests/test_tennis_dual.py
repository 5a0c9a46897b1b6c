"""The two-player rally without a GPU: the numpy statements of the dual step and the ball hand-over (`dual_step_reference`,
`handover_reference`) against what the reference itself computed (tests/golden/tennis_dual.npz), the cases the fixture is built from,
the ctypes mirrors of the two new structs, the argument refusals, and `reset_dual`'s choice of rows."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from tests import mvae_fixture as MF
from tests import tennis_dual_fixture as F
from vid2player3d_amd import mvae
from vid2player3d_amd.tasks import tennis_controller as tc
from vid2player3d_amd.tasks import tennis_controller_dual as td

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 50  # of the fixture's in-table


def _unmodified(keep, s, what):
    for k, v in keep.items():
        assert v is None or np.array_equal(v, s[k], equal_nan=True), "%s modified its input %s" % (what, k)


def _copy(s):
    return {k: None if v is None else np.array(v, copy=True) for k, v in s.items()}


@pytest.mark.parametrize("name", F.VARIANTS)
def test_step_statement_matches_the_fixture(name):
    st, s = F.settings(name), F.inputs("step", name)
    keep = _copy(s)
    out = td.dual_step_reference(st, s)
    F.compare(out, F.expected("step", name), F.scatter("step"), "step " + name)
    for k in ("est_bounce_pos", "est_bounce_time", "est_max_height", "est_bounce_in", "terminate", "vel_x_overflow"):
        assert k not in out, "the dual step does not write " + k
    _unmodified(keep, s, "dual_step_reference")


@pytest.mark.parametrize("name", F.VARIANTS)
def test_handover_statement_matches_the_fixture(name):
    st, s = F.settings(name), F.inputs("hand", name)
    keep = _copy(s)
    out = td.handover_reference(st, s)
    # (what a variant's launch does not write - the target without use_random_ball_target, est_* without return_w_estimate - must stay)
    F.compare(dict(s, **out), F.expected("hand", name), F.scatter("hand"), "hand-over " + name)
    assert np.array_equal(out["table_rows"], F.golden()["hand/%s/table_rows" % name])
    _unmodified(keep, s, "handover_reference")


@pytest.mark.parametrize("name", F.VARIANTS)
def test_truth_table_of_the_step(name):
    """tar_action x hit x miss x second bounce x bounce_in on each side of a pair, the OR over the pair, and `reset` left alone."""
    s, o = F.inputs("step", name), F.expected("step", name)
    n = len(s["ball_state"])
    tar, hit = s["tar_action"] == 1, o["has_racket_contact"].astype(bool)
    root_y = s["rb_state"][:, 0, 1]
    miss = s["ball_state"][:, 1] < root_y - 1
    twice = s["has_bounce"] & (s["ball_state"][:, 2] < 0.05)
    bounce_in = o["bounce_in"].astype(bool)
    for side in (0, 1):
        rows = {(bool(tar[e]), bool(hit[e]), bool(miss[e]), bool(twice[e]), bool(bounce_in[e])) for e in range(side, n, 2)}
        assert len(rows) == 32, "side %d of the pairs sees %d of the 32 rows" % (side, len(rows))
    recovery = tar & (hit | miss | twice)
    terminate = (recovery & ~hit) | (~tar & s["has_bounce"] & ~bounce_in)
    pair = terminate.reshape(-1, 2)
    both = np.repeat(pair.any(1), 2)
    assert (pair[:, 0] & ~pair[:, 1]).any() and (~pair[:, 0] & pair[:, 1]).any(), "no pair in which only the opponent terminates"
    assert np.array_equal(o["reset"], np.where(both, 1, s["reset"]))
    quiet = ~both
    assert (quiet & (s["reset"] == 1)).any() and (o["reset"][quiet] == s["reset"][quiet]).all(), "a quiet pair's reset = 1 must stay"
    assert np.array_equal(o["reset_recovery"], recovery & ~both)
    assert np.array_equal(o["reset_reaction"], recovery.reshape(-1, 2)[:, ::-1].reshape(-1) & ~both)
    if F.variant(name)["velocity"]:
        assert o["has_racket_contact_now"].any() and (hit & ~o["has_racket_contact_now"].astype(bool)).any()


def _frame_index(grid, end):
    lo, hi, step = grid
    return 0 if end == "lo" else int(round((hi - lo) / step)) - 1


@pytest.mark.parametrize("name", F.VARIANTS)
def test_handover_cases(name):
    d, v = F.golden(), F.variant(name)
    s, o = F.inputs("hand", name), F.expected("hand", name)
    rea, rec = s["reset_reaction"].reshape(-1, 2), s["reset_recovery"].reshape(-1, 2)
    assert (rea[:, 0] & ~rea[:, 1]).any() and (~rea[:, 0] & rea[:, 1]).any() and rea.all(1).any()
    # ---- a pair without a flag keeps every bit
    none = np.repeat(~(rea.any(1) | rec.any(1)), 2)
    assert none.any()
    for k, x in o.items():
        assert np.array_equal(x[none], np.asarray(s[k]).reshape(x.shape)[none]), k
    # ---- an env in both lists ends with tar_action = 1; a recovery alone with 0; flags are not cleared by the launch
    in_both = s["reset_reaction"] & s["reset_recovery"]
    assert in_both.any() and (o["tar_action"][in_both] == 1).all() and (o["tar_action"][s["reset_recovery"] & ~s["reset_reaction"]] == 0).all()
    ids = np.nonzero(s["reset_reaction"])[0]
    assert (o["tar_time"][ids] == 0).all() and np.array_equal(o["num_reset_reaction"][ids], s["num_reset_reaction"][ids] + 1) and not o["bounce_in"][ids].any()
    assert not o["has_bounce"][ids].any() and not o["has_racket_contact"][ids].any() and not o["bounce_pos"][ids].any()
    assert np.array_equal(o["prev_ball_vy"][ids], o["ball_state"][ids, 8])
    hitters_only = np.setdiff1d(ids ^ 1, ids)
    assert np.array_equal(o["prev_ball_vy"][hitters_only], s["prev_ball_vy"][hitters_only]), "the opponent's prev_ball_vy is left as it is"
    # ---- both react: out wins - position back where it was, bit for bit
    pair = np.nonzero(rea.all(1))[0][0]
    for e in (2 * pair, 2 * pair + 1):
        assert np.array_equal(o["ball_state"][e, [0, 1, 3, 4, 5, 6]], s["ball_state"][e, [0, 1, 3, 4, 5, 6]])
    # ---- one reacts: its position is the hitter's, negated, and the hitter keeps its own
    single = np.setdiff1d(ids, ids ^ 1)
    assert np.array_equal(o["ball_state"][single, 0:2], -s["ball_state"][single ^ 1, 0:2]) and np.array_equal(o["ball_state"][single, 3:7], s["ball_state"][single ^ 1, 3:7])
    assert np.array_equal(o["ball_state"][single ^ 1, 0:2], s["ball_state"][single ^ 1, 0:2])
    # ---- the clamps of every grid, both ends: the table row's digit of that grid is the first / the last cell
    rows = d["hand/%s/table_rows" % name]
    cells = [int(round((g[1] - g[0]) / g[2])) for g in d["in_grids"]]
    seen = set()
    for e in ids:
        h = s["ball_state"][e ^ 1 if e in single else e].astype(np.float64)
        val = (h[2], np.hypot(h[7], h[8]), h[9], np.linalg.norm(h[10:13]) / (2 * np.pi))
        digits = np.unravel_index(rows[e], cells)
        for g, grid in enumerate(d["in_grids"]):
            for end, beyond in (("lo", val[g] < grid[0]), ("hi", val[g] > grid[1] - grid[2])):
                if beyond:
                    assert digits[g] == _frame_index(grid, end)
                    seen.add((g, end))
    assert seen == {(g, end) for g in range(4) for end in ("lo", "hi")}, seen
    # ---- the window: new frames in front, the stale tail of the old window behind them, frame by frame
    if not v["history"]:
        cur = s["traj_cursor"]
        assert all(c in cur[ids] for c in (0, 37, 99)) and (o["traj_cursor"][ids] == 0).all()
        old = s["ball_traj"].reshape(-1, 100, 3)
        new = o["ball_traj"].reshape(-1, 100, 3)
        for e in ids:
            for f in range(FRAMES, 100):
                src = cur[e] + f
                want = old[e, src] if src < 100 else np.zeros(3, np.float32)
                assert np.array_equal(new[e, f], want), "env %d frame %d (cursor %d)" % (e, f, cur[e])
            table = d["traj_in"][rows[e]]
            assert np.array_equal(new[e, :FRAMES, 2], table[:, 1])
    else:
        L = 10
        assert np.array_equal(o["ball_obs"][ids], np.repeat(o["ball_state"][ids, None, 0:3], L, 1)), "the history of a reacting env is its new ball position"
    if v["target"]:
        u = s["target_draw"][ids]
        assert (u < 0.33).any() and (u > 0.67).any() and ((u > 0.33) & (u < 0.67)).any()
        assert np.array_equal(o["target_bounce_pos"][ids, 0], np.where(u < 0.33, -3.0, np.where(u > 0.67, 3.0, 0.0)).astype(np.float32))
    if v["reward_type"] == "return_w_estimate":
        assert s["est_bounce_pos"][ids].any() and not o["est_bounce_pos"][ids].any() and not o["est_bounce_in"][ids].any()
    else:
        assert np.array_equal(o["est_bounce_pos"], s["est_bounce_pos"])


def test_both_history_modes_are_in_the_fixture():
    assert {F.variant(v)["history"] for v in F.VARIANTS} == {False, True}
    assert {F.variant(v)["different"] for v in F.VARIANTS} == {False, True}


def test_struct_sizes_match_the_header(tmp_path):
    from vid2player3d_amd import _lib

    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "v2p_rollout.h"\nint main(void){ printf("%zu %zu\\n", sizeof(v2p_tennis_dual_cfg), sizeof(v2p_tennis_dual_buffers)); return 0; }\n')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.TennisDualCfg), ctypes.sizeof(_lib.TennisDualBuffers)]
    assert _lib.ABI_VERSION == 15


def _mod(struct, **fields):
    for k, v in fields.items():
        setattr(struct, k, v)
    return struct


def test_bad_arguments_are_refused_without_a_gpu():
    from vid2player3d_amd import _lib, build

    build.build()
    lib = _lib.load()
    one = 16  # (a non-null placeholder: every call below is refused before anything is dereferenced)
    st = F.settings("B")  # (history, target)
    plain = F.settings("A")
    cfg = lambda s=st, **kw: ctypes.byref(_mod(tc.cfg_struct(s, (1, 1), (1, 1, 2)), **kw))
    dual = lambda **kw: ctypes.byref(_mod(td.dual_cfg_struct(st, (144, 50, 2)), **kw))
    full = lambda **kw: ctypes.byref(_mod(_lib.TennisBuffers(**{k: one for k in _lib.TENNIS_BUFFER_NAMES}), **kw))
    dbuf = lambda **kw: ctypes.byref(_mod(_lib.TennisDualBuffers(**{k: one for k in _lib.TENNIS_DUAL_BUFFER_NAMES}), **kw))
    step = lambda c, d, n, b: lib.v2p_tennis_dual_step(c, d, n, b, None, None)
    hand = lambda c, d, n, b, db: lib.v2p_tennis_dual_handover(c, d, n, b, db, None)
    err = lib.v2p_last_error
    # ---- the step
    assert step(cfg(), dual(), 7, full()) == -1 and b"v2p_tennis_dual_step" in err() and b"odd" in err()
    assert step(None, dual(), 8, full()) == -1 and step(cfg(), None, 8, full()) == -1 and step(cfg(), dual(), 8, None) == -1 and b"v2p_tennis_dual_step: null" in err()
    assert step(cfg(), dual(), -2, full()) == -1
    assert step(cfg(obs_ball_traj_length=101), dual(), 8, full()) == -1 and b"obs_ball_traj_length" in err()
    assert step(cfg(reward_type=3), dual(), 8, full()) == -1 and b"reward type" in err()
    for missing in ("rb_state", "obs", "tar_time", "swing_type", "ball_obs", "reset_reaction", "has_bounce", "est_bounce_in", "reset"):
        assert step(cfg(), dual(), 8, full(**{missing: None})) == -1, missing
        assert b"v2p_tennis_dual_step: null buffer" in err()
    assert step(cfg(plain), dual(), 8, full(ball_traj=None)) == -1
    # (what the dual step does not touch may be null: refused only for being odd)
    untouched = {k: None for k in td.UNUSED_BUFFERS}
    assert step(cfg(), dual(), 7, full(**untouched)) == -1 and b"odd" in err()
    # ---- the hand-over
    assert hand(cfg(), dual(), 7, full(), dbuf()) == -1 and b"v2p_tennis_dual_handover" in err() and b"odd" in err()
    assert hand(cfg(), dual(), 8, full(), None) == -1 and hand(cfg(), None, 8, full(), dbuf()) == -1 and hand(None, dual(), 8, full(), dbuf()) == -1
    assert hand(cfg(), dual(), 8, full(), dbuf(target_draw=None)) == -1 and b"target_draw" in err()
    assert hand(cfg(), dual(in_frames=0), 8, full(), dbuf()) == -1 and hand(cfg(), dual(in_frames=101), 8, full(), dbuf()) == -1 and b"in_frames" in err()
    assert hand(cfg(), dual(in_rows=0), 8, full(), dbuf()) == -1
    bad = td.dual_cfg_struct(st, (144, 50, 2))
    bad.in_grid[2][2] = 0.0
    assert hand(cfg(), ctypes.byref(bad), 8, full(), dbuf()) == -1 and b"in_grid 2" in err()
    for missing in ("traj_in", "ball_state", "has_bounce", "bounce_pos", "tar_action", "num_reset_reaction", "target_bounce_pos"):
        assert hand(cfg(), dual(), 8, full(), dbuf(**{missing: None})) == -1, missing
        assert b"v2p_tennis_dual_handover: null dual buffer" in err()
    assert hand(cfg(plain), dual(), 8, full(), dbuf(ball_traj=None)) == -1
    assert hand(cfg(), dual(), 8, full(obs=None), dbuf()) == -1 and b"v2p_tennis_dual_handover: null buffer" in err()
    # ---- zero envs are a no-op
    names = ctypes.c_char_p()
    assert lib.v2p_tennis_dual_step(cfg(), dual(), 0, ctypes.byref(_lib.TennisBuffers()), ctypes.byref(names), None) == 0 and names.value == b"pos_reward,ball_pos_reward"
    assert hand(cfg(), dual(), 0, ctypes.byref(_lib.TennisBuffers()), ctypes.byref(_lib.TennisDualBuffers())) == 0


def test_the_tasks_and_their_modes():
    import torch

    cfg = {"env": {"episodeLength": 300}, "v2p": {"court_min": [-5, -16], "court_max": [5, -1], "reset_reaction_nframes": 6}}
    fake = types.SimpleNamespace(device="cpu", num_envs=4, _ball_root_states=torch.zeros(4, 13), racket_players=None)
    with pytest.raises(NotImplementedError, match="dual_mode"):
        tc.TennisControllerTask(fake, {"env": cfg["env"], "v2p": dict(cfg["v2p"], dual_mode=True)})
    with pytest.raises(NotImplementedError, match="dual_mode"):
        tc.TennisControllerTask(types.SimpleNamespace(**dict(vars(fake), racket_players=["nadal", "federer"])), cfg)
    with pytest.raises(ValueError, match="dual_mode"):
        td.DualTennisControllerTask(fake, cfg)
    with pytest.raises(ValueError, match="two-player"):
        td.DualTennisControllerTask(fake, {"env": cfg["env"], "v2p": dict(cfg["v2p"], dual_mode="different")})
    odd = types.SimpleNamespace(**dict(vars(fake), num_envs=5))
    with pytest.raises(ValueError, match="even"):
        td.DualTennisControllerTask(odd, {"env": cfg["env"], "v2p": dict(cfg["v2p"], dual_mode=True)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        td.DualTennisControllerTask(fake, {"env": cfg["env"], "v2p": dict(cfg["v2p"], dual_mode=True)})
    with pytest.raises(NotImplementedError, match="dual_mode"):
        mvae.player_settings({"player": "federer", "dual_mode": "different"}, True)
    assert mvae.player_settings({"player": "federer", "dual_mode": True}, True)["player"] == "federer"
    # the two-player configs give `grip` as a list of two names: the base settings take the even side's, the dual settings both
    grip = td.DualTennisControllerTask._grip
    assert grip(None, {"dual_mode": "different", "grip": ["semi_western", "eastern"]}) == "semi_western" and grip(None, {"dual_mode": True}) == "eastern"
    assert tc.task_settings(grip=grip(None, {"dual_mode": "different", "grip": ["semi_western", "eastern"]}))["grip_normal"] == tuple(tc.GRIP_NORMALS["semi_western"])
    assert td.dual_settings(grip=["semi_western", "eastern"])["grip_normals"] == (tuple(tc.GRIP_NORMALS["semi_western"]), tuple(tc.GRIP_NORMALS["eastern"]))
    with pytest.raises(ValueError, match="list of two names"):
        grip(None, {"dual_mode": "different", "grip": "eastern"})


def test_reset_dual_takes_ready_rows_for_reaction_ids_and_serve_rows_for_recovery_ids():
    d = F.golden()
    reaction, recovery = d["reset_dual/reaction_ids"], d["reset_dual/recovery_ids"]
    ids, from_ready = mvae.dual_reset_rows(reaction, recovery)
    assert np.array_equal(ids, np.sort(np.concatenate([reaction, recovery])))
    assert np.array_equal(from_ready, np.isin(ids, reaction)) and from_ready.any() and not from_ready.all()
    feature = np.where(from_ready[:, None], d["reset_dual/ready"], d["reset_dual/serve"])
    _, avg, std = MF.weights()
    st = mvae.player_settings({"player": "federer", "dual_mode": True, "add_residual_dof": "euler"}, True)
    post = {k[len("reset_dual/post/"):]: v for k, v in d.items() if k.startswith("reset_dual/post/")}
    zero = {k: np.zeros_like(v) for k, v in post.items()}
    zero["swing_type"], zero["swing_type_cycle"] = zero["swing_type"] + 2, zero["swing_type_cycle"] + 1
    got = mvae.mvae_reset_reference(st, avg, std, zero, ids, feature, d["reset_dual/root_xy"], d["reset_dual/joint_pos_bind_rel"])
    sc = {k[len("scatter/reset_dual/"):]: float(v) for k, v in d.items() if k.startswith("scatter/reset_dual/")}
    rest = np.setdiff1d(np.arange(len(post["root_pos"])), ids)
    for k, want in post.items():
        a = np.asarray(got[k]).reshape(want.shape)
        if want.dtype.kind in "iub":
            assert np.array_equal(a, want), k
            continue
        err = float(np.abs(a.astype(np.float64) - want).max())
        print("reset_dual: %s max |difference| %.3g, allowance %.3g" % (k, err, 8 * sc[k]))
        assert err <= 8 * sc[k], k
        assert not a[rest].any(), "reset_dual touched an env outside both lists: " + k
    assert (post["swing_type"][ids] == -1).all() and (post["swing_type"][rest] == 2).all()
    # an id in both lists starts from the serve frame, which the reference writes last
    assert not mvae.dual_reset_rows([2, 3], [3])[1][1] and mvae.dual_reset_rows([2, 3], [3])[1][0]
