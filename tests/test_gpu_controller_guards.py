"""The controller-side kernels between guard rows (tests/guarded.py): tennis_task.hip with tennis_row.inc, mvae_player.hip,
mvae_player_dual.hip, mvae_target.hip and ball_rollout.hip.  Every tensor handed to a launch lies between guard rows - inputs and in/out
state through `Guarded.of`, outputs through `Guarded.empty` (NaN / 0x5A: an element left unwritten fails the comparison) - at the sizes
that reach each geometry's tails: a wave per env and 4 envs per workgroup (tennis step, observation), a half wave per env and pairs
(hand-over), a 32-env MFMA tile (motion generator), a side per workgroup (dual generator), 32 lanes per env and 8 envs per workgroup
(imitation target), a 16-frame staging area and 64 balls per workgroup (ball roll-out).  After the launch the guard rows are checked, the
results compared with the entry's numpy statement at the tolerances of the entry's own test, and what the entry only reads must come back
with its bits.  Every id list holds `n` and -1: a store to row n lies in the back guard, one to row -1 in the front guard.

The edge inputs of tests/tennis_edges.py (tests/test_tennis_edges.py holds their census) run here on the device.  The last three tests
launch one row too wide on purpose, inside the test's own memory, with the guards armed on valid numbers: the check must then name
exactly what the entry writes, behind."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.test_gpu_mvae_dual as MD
import tests.test_gpu_mvae_player as MP
import tests.test_gpu_mvae_target as TT
import tests.test_gpu_tennis_controller as TC
import tests.test_gpu_tennis_dual as TD
from tests import ball_oracle as B
from tests import mvae_dual_fixture as DX
from tests import mvae_fixture as MX
from tests import mvae_target_fixture as TX
from tests import tennis_dual_fixture as DF
from tests import tennis_edges as E
from tests import tennis_fixture as F
from tests.guarded import BEHIND, Guarded
from vid2player3d_amd import _lib, ball_traj, mvae
from vid2player3d_amd import mvae_target as mt
from vid2player3d_amd.tasks import tennis_controller as tc
from vid2player3d_amd.tasks import tennis_controller_dual as td

gpu = pytest.mark.gpu
DEV = "cuda:0"
f32, i64, u8 = torch.float32, torch.int64, torch.uint8
OBS_ROWS = ("obs", "racket_pos", "racket_normal", "ball_obs")  # what v2p_tennis_task_obs writes, rows of the ids only


def download(t):
    return {k: v.detach().cpu().numpy() for k, v in t.items()}


def id_list(n):
    return np.array([n - 1, n, 0, -1], np.int64)


def unchanged(before, got, written, what):
    for k in before:
        if k not in written:
            assert np.array_equal(before[k], got[k], equal_nan=True), "%s: the kernel wrote %s" % (what, k)


# ================================================================================================================== the tennis kernels
def single_outputs(st):
    return dict(racket_pos=((3,), f32), racket_normal=((3,), f32), obs=((tc.obs_width(st),), f32), rew=((), f32), sub_rewards=((tc.num_sub_rewards(st),), f32),
                reset=((), i64), terminate=((), i64), reset_reaction=((), u8), reset_recovery=((), u8))


def dual_step_outputs(st):
    return {k: v for k, v in single_outputs(st).items() if k not in ("reset", "terminate")}


def tennis_tensors(G, s, outputs, spill=0):
    """Every array of `s` between guard rows under the dtypes of the entry's own test, the outputs poisoned; spill: see Guarded.of."""
    t = {}
    for k, v in s.items():
        if v is None:
            continue
        byte = k in TD.BYTES
        a = np.ascontiguousarray(v)
        t[k] = G.of(k, a.astype(np.uint8) if byte else a, dtype=u8 if byte else TD.DTYPES.get(k, f32), spill=0 if k in E.TABLES else spill)
    n = len(s["rb_state"]) - spill
    for k, (tail, dt) in outputs.items():
        t[k] = G.empty(k, (n,) + tail, dt)
    return t


def step_writes(st):
    return TC.WRITTEN if st["contact_by_velocity"] else TC.WRITTEN - {"has_racket_contact", "has_racket_contact_now"}


def run_step(st, s, what, s_ref=None):
    """v2p_tennis_task_step on `s` between guards against task_step_reference (of s_ref, where the kernel's clamp stands for the input)."""
    G, n = Guarded(DEV), len(s["rb_state"])
    dev = tennis_tensors(G, s, single_outputs(st))
    before = download(dev)
    names = tc.launch_step(st, dev, n)
    G.check()
    got = download(dev)
    want = tc.task_step_reference(st, s if s_ref is None else s_ref)
    assert names == want.pop("sub_rewards_names")
    F.compare(got, want, what)
    unchanged(before, got, step_writes(st), what)
    return got, want


def run_obs(st, s, ids, what, s_ref=None):
    """v2p_tennis_task_obs for `ids` between guards: the rows of the ids in the batch against observation_reference, every other row and
    every other tensor with its bits.  An id that occurs twice has the statement's row: the same values are written twice."""
    G, n = Guarded(DEV), len(s["rb_state"])
    dev = tennis_tensors(G, s, single_outputs(st))
    before = download(dev)
    tc.launch_obs(st, dev, n, G.of("env_ids", np.asarray(ids, np.int64)))
    G.check()
    got = download(dev)
    ids = np.asarray(ids)
    valid = np.unique(ids[(ids >= 0) & (ids < n)])
    obs, hist, rpos, rnorm = tc.observation_reference(st, s if s_ref is None else s_ref, valid)
    want = dict(obs=obs, racket_pos=rpos, racket_normal=rnorm)
    if hist is not None:
        want["ball_obs"] = hist
    F.compare({k: got[k][valid] for k in want}, want, what)
    others = np.setdiff1d(np.arange(n), valid)
    for k in before:
        rows = others if k in OBS_ROWS else slice(None)
        assert np.array_equal(before[k][rows], got[k][rows], equal_nan=True), "%s: the observation call wrote %s outside the rows of its ids" % (what, k)
    return got, want


def dual_step_writes(st):
    w = set(TD.STEP_WRITES)
    if not st["contact_by_velocity"]:
        w -= {"has_racket_contact", "has_racket_contact_now"}
    if st["use_history"]:
        w -= {"traj_cursor"}
    return w


def run_dual_step(st, s, what, fixture=None):
    G, n = Guarded(DEV), len(s["rb_state"])
    dev = tennis_tensors(G, s, dual_step_outputs(st))
    before = download(dev)
    names = td.launch_dual_step(st, dev, n)
    G.check()
    got = download(dev)
    want = td.dual_step_reference(st, s)
    assert names == want.pop("sub_rewards_names")
    DF.compare(got, {k: np.asarray(v) for k, v in want.items()}, DF.scatter("step"), what + " against the statement")
    if fixture is not None:
        DF.compare(got, fixture, DF.scatter("step"), what)
    unchanged(before, got, dual_step_writes(st), what)
    return got, want


def run_handover(st, s, what, fixture=None):
    G, n = Guarded(DEV), len(s["rb_state"])
    dev = tennis_tensors(G, s, {})
    before = download(dev)
    td.launch_handover(st, dev, n)
    G.check()
    got = download(dev)
    want = td.handover_reference(st, s)
    want.pop("table_rows")
    DF.compare(got, {k: np.asarray(v) for k, v in want.items()}, DF.scatter("hand"), what + " against the statement")
    if fixture is not None:
        DF.compare(got, fixture, DF.scatter("hand"), what)
    rea, rec = np.asarray(s["reset_reaction"]).reshape(-1, 2), np.asarray(s["reset_recovery"]).reshape(-1, 2)
    untouched = np.repeat(~(rea.any(1) | rec.any(1)), 2)
    for k, v in before.items():
        if len(v) == n and k not in E.TABLES:
            assert np.array_equal(v[untouched], got[k][untouched], equal_nan=True), "%s: a pair without a flag changed its %s" % (what, k)
    unchanged(before, got, set(want), what)
    return got, want


# ------------------------------------------------------------------------------------------------------------------ tails
@gpu
@pytest.mark.parametrize("n", [1, 3, 5, 80])
@pytest.mark.parametrize("name", F.VARIANTS)
def test_tennis_step_and_observation_at_their_tails(name, n):
    st, _ = F.settings(name)
    s = E.take(F.step_inputs(name, 0), np.arange(n))
    what = "variant %s, %d envs" % (name, n)
    got, want = run_step(st, s, what + ", step")
    if n == 80:
        F.compare(got, F.step_expected(name, 0), what + ", step against the fixture")
    run_obs(st, s, id_list(n), what + ", observation of [n - 1, n, 0, -1]")
    run_obs(st, s, [n - 1, 0, n - 1], what + ", observation of an id twice")


@gpu
@pytest.mark.parametrize("n", [2, 6, 10, 66])
@pytest.mark.parametrize("name", DF.VARIANTS)
def test_dual_step_and_handover_at_their_tails(name, n):
    st = DF.settings(name)
    what = "dual variant %s, %d envs" % (name, n)
    run_dual_step(st, DF.inputs("step", name, n), what + ", step", DF.expected("step", name, n))
    run_handover(st, DF.inputs("hand", name, n), what + ", hand-over", DF.expected("hand", name, n))


# ------------------------------------------------------------------------------------------------------------------ edge inputs
@gpu
@pytest.mark.parametrize("L", E.HISTORY_LENGTHS)
def test_history_roll_over_more_than_one_pass(L):
    st, s = E.history(L)
    n = len(s["rb_state"])
    what = "history of %d frames" % L
    got, want = run_step(st, s, what + ", step")
    assert np.array_equal(got["ball_obs"], want["ball_obs"]), what + ": the rolled history is a copy and differs in its bits"
    got, want = run_obs(st, s, id_list(n), what + ", observation")
    assert np.array_equal(got["ball_obs"][[0, n - 1]], want["ball_obs"]), what + ": the rolled history is a copy and differs in its bits"
    st, s = E.dual_history("step", L)
    run_dual_step(st, s, what + ", dual step")  # (the scatter of ball_obs is 0: bit for bit)
    st, s = E.dual_history("hand", L)
    run_handover(st, s, what + ", hand-over")


@gpu
@pytest.mark.parametrize("L", E.CURSOR_LENGTHS)
def test_cursors_at_and_past_the_windows_end(L):
    st, s = E.cursor_rows(L)
    what = "cursor edges, window of %d frames" % L
    got, _ = run_step(st, s, what + ", step")
    assert np.array_equal(got["traj_cursor"], E.cursors_after(L))
    run_obs(st, s, np.concatenate([np.arange(8), [8, -1]]), what + ", observation")
    for kind, run in (("step", run_dual_step), ("hand", run_handover)):
        st, s = E.dual_cursors(kind, L)
        run(st, s, "%s, dual %s" % (what, kind))


@gpu
def test_wrist_links():
    st, s = E.wrists()
    run_step(st, s, "wrist links, step")
    run_obs(st, s, id_list(len(E.WRISTS)), "wrist links, observation")
    given, stated = E.WRISTS_CLAMPED
    st, s = E.wrists(given)
    ref = dict(s, wrist_link=np.array(stated, np.int64))
    run_step(st, s, "wrist links below 0 and above 23, step", s_ref=ref)
    run_obs(st, s, id_list(len(given)), "wrist links below 0 and above 23, observation", s_ref=ref)
    for kind, run in (("step", run_dual_step), ("hand", run_handover)):
        st, s = E.dual_wrists(kind)
        run(st, s, "wrist links, dual %s" % kind)


@gpu
def test_out_estimator_at_every_reachable_clamp():
    st, s = E.estimator()
    got, want = run_step(st, s, "out-estimator rows")
    _, valid = E.estimator_census(st, s, want)
    for k in ("est_bounce_pos", "est_bounce_time", "est_max_height", "est_bounce_in"):
        assert np.array_equal(got[k][~valid], np.asarray(s[k])[~valid].astype(got[k].dtype)), "a row without a valid hit did not keep the bits of its %s" % k
    assert int(got["vel_x_overflow"][0]) == int(want["vel_x_overflow"]) == int(s["vel_x_overflow"][0]) + 1


@gpu
def test_dual_reset_law_over_all_sixteen_combinations():
    st, s = E.dual_flags()
    got, want = run_dual_step(st, s, "dual reset law")
    assert len(E.dual_flags_census(st, s, want)) == 16
    for k in ("reset", "reset_reaction", "reset_recovery"):  # (integers: DF.compare holds them exact; said again for the law's three outputs)
        assert np.array_equal(got[k].astype(np.int64), np.asarray(want[k]).astype(np.int64)), k


# ================================================================================================================== the motion generator
def guard_player(G, p, arrays=None):
    """`p._<name>` of every state tensor becomes a guarded slice of the same shape: the array given for it, else poison."""
    for k in mvae.STATE_NAMES:
        t = getattr(p, "_" + k)
        given = None if arrays is None else arrays.get(k)
        setattr(p, "_" + k, G.empty(k, tuple(t.shape), t.dtype) if given is None else G.of(k, np.asarray(given).reshape(tuple(t.shape)), dtype=t.dtype))


@gpu
@pytest.mark.parametrize("n", [1, 33, 70])
def test_motion_generator_reset_and_step_at_the_tile_edges(n):
    """the seeded rows of test_gpu_mvae_player.py's tile-edge case: a reset of [n - 1, n, 0, -1] on poisoned state, a reset of all, a step"""
    w, avg, std = MX.weights()
    e, g = MX.edge_inputs(), MX.golden()
    p = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, n, w, avg, std, e["init"][:n], e["bind"], False, DEV)
    G = Guarded(DEV)
    guard_player(G, p)
    before = p.state_arrays()
    ids = id_list(n)
    rows = np.clip(ids, 0, n - 1)
    p.reset(G.of("env_ids", ids), G.of("root_xy", e["xy"][rows]))
    G.check()
    got = p.state_arrays()
    named = np.unique(rows)
    pick = lambda d: {k: x[named] for k, x in d.items() if k != "phase_pred"}
    want = mvae.mvae_reset_reference(p.settings, avg, std, before, ids, e["init"][rows], e["xy"][rows], e["bind"])
    want64 = mvae.mvae_reset_reference(p.settings, avg, std, {k: (x.astype(np.float64) if x.dtype.kind == "f" else x) for k, x in before.items()}, ids, e["init"][rows],
                                       e["xy"][rows], e["bind"], dt=np.float64)
    sure = MX.well_conditioned(pick(want), pick(want64), MX.scatter_of(g, "reset"))
    assert sure.sum() >= 0.9 * len(named), "too few rows to judge: %d of %d" % (sure.sum(), len(named))
    MX.assert_state(pick(got), pick(want), MX.scatter_of(g, "reset"), "N = %d reset of %s" % (n, ids.tolist()), rows=np.nonzero(sure)[0])
    others = np.setdiff1d(np.arange(n), named)
    for k in mvae.STATE_NAMES:
        assert np.array_equal(got[k][others], before[k][others], equal_nan=True), "reset wrote %s of an env it was not given" % k
    assert np.array_equal(got["phase_pred"], before["phase_pred"], equal_nan=True), "the reset leaves the phase alone"
    # ---- all envs, then one step: what test_tile_edges_against_the_numpy_statement asserts, between guards
    p.reset(G.of("all_ids", np.arange(n)), G.of("all_xy", e["xy"][:n]))
    p._swing_type.copy_(torch.as_tensor(e["swing"][:n]))
    p._swing_type_cycle.copy_(torch.as_tensor(e["swing"][:n]))
    before = p.state_arrays()
    MP.poison(p, MP.OUTPUT_ONLY)
    z, r = G.of("latents", e["z"][:n]), G.of("residual", e["res"][:n])
    p.step(z, r)
    G.check()
    got = p.state_arrays()
    want = mvae.mvae_step_reference(p.settings, w, avg, std, before, e["z"][:n], e["res"][:n])
    sure = ~MX.near_threshold(p.settings, w, avg, std, before, e["z"][:n], e["res"][:n])
    want64 = mvae.mvae_step_reference(p.settings, w, avg, std, before, e["z"][:n], e["res"][:n], dt=np.float64)
    scatter = MX.scatter_of(g, "step")
    sure &= MX.well_conditioned(want, want64, scatter)
    assert sure.sum() >= 0.9 * n, "too few rows to judge: %d of %d" % (sure.sum(), n)
    MX.assert_state(got, want, scatter, "N = %d step" % n, rows=np.nonzero(sure)[0])
    assert all(np.isfinite(got[k]).all() for k in MX.FLOAT_STATE)
    assert np.array_equal(z.cpu().numpy(), e["z"][:n]) and np.array_equal(r.cpu().numpy(), e["res"][:n])
    for k in ("racket_pos", "racket_normal"):
        assert np.array_equal(got[k], before[k]), "the step wrote %s" % k


@gpu
@pytest.mark.parametrize("case", [(0, 2), (1, 62), (3, 66)])
def test_dual_motion_generator_step_and_reset_at_the_tile_edges(case):
    """sizes 2, 62 and 66 of test_gpu_mvae_dual.py's tile-edge case with its inputs, under both mappings of workgroups to sides; then the
    reset of the whole pairs {0, 1} and {n - 2, n - 1} on poisoned state, with the pairs {-2, -1} and {n, n + 1} in the list"""
    t, n = case
    v, g = "B", DX.golden()
    w, avg, std = DX.weights()
    p = MD.make_player(g, v, n)
    tile = lambda x: np.concatenate([x] * (n // DX.N + 1))[:n]
    before = {k: tile(x) for k, x in DX.state_before(g, v, t).items()}
    z, r = tile(g[v + "/latents"][t]), tile(g[v + "/residual"][t])
    want = mvae.mvae_dual_step_reference(p.settings, w, avg, std, before, z, r)
    for mapping in (mvae.DUAL_MAP_HALVES, mvae.DUAL_MAP_PARITY):
        G = Guarded(DEV)
        guard_player(G, p, before)
        p.dual_mapping = mapping
        p.step(G.of("latents", z), G.of("residual", r))
        G.check()
        got = p.state_arrays()
        MX.assert_state(got, want, MX.scatter_of(g, "step"), "n = %d, mapping %d: step" % (n, mapping))
        assert np.isnan(got["racket_pos"]).all() and np.isnan(got["racket_normal"]).all(), "the racket is the reset's"
    G = Guarded(DEV)
    guard_player(G, p)
    before = p.state_arrays()
    ids = np.unique([-2, -1, 0, 1, n - 2, n - 1, n, n + 1])  # (whole pairs, as reset_dual demands; the pairs outside the batch are skipped)
    reaction, recovery = ids[ids % 2 == 0], ids[ids % 2 == 1]
    listed, from_ready = mvae.dual_reset_rows(reaction, recovery)
    assert np.array_equal(listed, ids)
    feature = np.where(from_ready[:, None], g[v + "/init_ready"][ids % 2], g[v + "/init_serve"][ids % 2])
    xy = g[v + "/root_xy"][:len(ids)]
    p.reset_dual(MD.dev(reaction), MD.dev(recovery), G.of("root_xy", xy))
    G.check()
    got = p.state_arrays()
    want = mvae.mvae_dual_reset_reference(p.settings, avg, std, before, ids, feature, xy, g["joint_pos_bind_rel"])
    valid = ids[(ids >= 0) & (ids < n)]
    MX.assert_state({k: x[valid] for k, x in got.items()}, {k: np.asarray(x)[valid] for k, x in want.items() if k != "phase_pred"}, MX.scatter_of(g, "reset"),
                    "n = %d: reset of %s" % (n, ids.tolist()))
    others = np.setdiff1d(np.arange(n), valid)
    for k in mvae.STATE_NAMES:
        assert np.array_equal(got[k][others], before[k][others], equal_nan=True), "the reset wrote %s of an env it was not given" % k
    assert np.array_equal(got["phase_pred"], before["phase_pred"], equal_nan=True), "the reset leaves the phase alone"


# ================================================================================================================== the imitation target
TARGET_TABLES = ("joint_pos_bind",)


def target_tensors(G, d, n, spill=0):
    """test_gpu_mvae_target.py's step tensors (n + spill rows) replaced by guarded ones; the target is an output."""
    out = {k: None if x is None else G.of(k, x, spill=0 if k in TARGET_TABLES else spill) for k, x in d.items() if k != "target"}
    out["target"] = G.empty("target", (n, mt.ROW), f32)
    return out


@gpu
@pytest.mark.parametrize("n", [1, 3, 9, 65])
@pytest.mark.parametrize("v", TX.VARIANTS)
def test_imitation_target_step_and_reset_at_their_tails(v, n):
    g = TX.golden()
    st, shapes = TX.settings(g, v), len(g[v + "/joint_pos_bind"])
    for t in (0, TX.steps(g, v) - 1):
        plain, _, idx = TT.step_tensors(g, v, t, n)
        G = Guarded(DEV)
        d = target_tensors(G, plain, n)
        before = {k: x.cpu().numpy() for k, x in d.items() if x is not None}
        mt.launch_step(st, d, n, shapes)
        G.check()
        what = "variant %s, %d envs, step %d" % (v, n, t)
        TX.assert_row(d["target"].cpu().numpy(), g[v + "/target"][t + 1][idx], TX.scatter_of(g, "step"), what)
        for k in ("root_pos", "residual_root", "ball_state", "joint_pos_bind", "env_shape_id", "prev_target", "rb_state"):
            if k in before:
                assert np.array_equal(before[k], d[k].cpu().numpy(), equal_nan=True), "%s: the kernel wrote %s" % (what, k)
        got = d["joint_rotmat"].cpu().numpy()
        TX.assert_close(got, TX.expected_rotmat(g, v, t, st)[idx], TX.scatter_of(g, "step")["joint_rotmat"], what + ": joint_rotmat")
        others = [j for j in range(24) if not st["fix_head_orientation"] or j not in (st["smpl_head"], st["smpl_neck"])]
        assert np.array_equal(got[:, others], before["joint_rotmat"][:, others]), what + ": a joint other than Head and Neck was written"
        for k in ("hold_reset", "hold_progress", "hold_cur_time"):
            assert not d[k].cpu().numpy().any(), "%s: %s is not held" % (what, k)
    # ---- the reset of [n - 1, n, 0, -1]
    r = TX.reset_inputs(g, v)
    idx = np.arange(n) % len(r["root_pos"])
    rng = np.random.default_rng(3)
    G = Guarded(DEV)
    d = dict(root_pos=G.of("root_pos", r["root_pos"][idx]), joint_rotmat=G.of("joint_rotmat", r["joint_rotmat"][idx]), joint_pos_bind=G.of("joint_pos_bind", r["joint_pos_bind"]),
             env_shape_id=G.of("env_shape_id", r["env_shape_id"][idx], dtype=torch.int32), target=G.of("target", rng.normal(size=(n, mt.ROW)), dtype=f32),
             root_states=G.of("root_states", rng.normal(size=(n, 13)), dtype=f32), dof_state=G.of("dof_state", rng.normal(size=(n, 69, 2)), dtype=f32),
             rb_state=G.of("rb_state", rng.normal(size=(n, 24, 13)), dtype=f32))
    before = download(d)
    mt.launch_reset(st, d, n, G.of("env_ids", id_list(n)), shapes)
    G.check()
    got = download(d)
    named = np.unique([0, n - 1])
    others = np.setdiff1d(np.arange(n), named)
    for k in before:
        rows = others if k in ("target", "root_states", "dof_state", "rb_state") else slice(None)
        assert np.array_equal(before[k][rows], got[k][rows]), "variant %s, %d envs: rows of other envs (or an input) written in %s" % (v, n, k)
    TX.assert_close(got["target"][named], g[v + "/target"][0][idx[named]], TX.scatter_of(g, "reset")["target"], "variant %s, %d envs: reset rows" % (v, n))
    row, m = mt.unpack_row(got["target"][named]), len(named)
    assert np.array_equal(got["root_states"][named, 0:3], row["root_pos"]) and np.array_equal(got["root_states"][named, 3:7], row["root_rot"])
    assert not got["root_states"][named, 7:].any() and not got["dof_state"][named][..., 1].any() and not got["rb_state"][named][..., 7:].any()
    assert np.array_equal(got["dof_state"][named][..., 0], row["dof_pos"])
    assert np.array_equal(got["rb_state"][named][..., 0:3].reshape(m, 72), row["rb_pos"]) and np.array_equal(got["rb_state"][named][..., 3:7].reshape(m, 96), row["rb_rot"])


@gpu
@pytest.mark.parametrize("n", [1, 3, 7])
def test_imitation_target_actions_at_sizes_that_are_no_multiple_of_the_block(n):
    g = TX.golden()
    for base in sorted(mt.PD_TARGET_BASES):
        for no_scale in (False, True):
            st = TX.settings(g, "H", pd_target_base=base, no_scale_action=no_scale)
            G = Guarded(DEV)
            a = G.of("actions_in", g["actions/in"][:n])
            out = G.empty("actions_out", (n, 75), f32)
            d = dict(target=G.of("target", g["actions/target"][:n]), dof_state=G.of("dof_state", np.stack([g["actions/dof_pos"], np.full_like(g["actions/dof_pos"], np.nan)], -1)[:n]),
                     pd_action_scale=G.of("pd_action_scale", g["actions/pd_action_scale"]), pd_action_offset=G.of("pd_action_offset", g["actions/pd_action_offset"]))
            before = download(d)
            mt.launch_actions(st, d, n, a, out)
            G.check()
            name = "%s/%d" % (base, int(no_scale))
            TX.assert_close(out.cpu().numpy()[:, :69], g["actions/out/" + name][:n], TX.scatter_of(g, "actions")[name], "pd targets %s, %d envs" % (name, n))
            assert np.array_equal(out.cpu().numpy()[:, 69:], g["actions/in"][:n, 69:]) and np.array_equal(a.cpu().numpy(), g["actions/in"][:n])
            unchanged(before, download(d), (), "pd targets " + name)


# ================================================================================================================== the ball roll-out
ROLLOUT_NAME = "generator"
RESAMPLE = ((0.0, 3.5, 0.5), (0.0, 1.3, 0.1))  # 7 and 13 cells
UNWRITTEN = 0x5A5A5A5A5A5A5A5A
SENTINEL = -7777.0  # float outputs of a resampled run start as this: a ball without horizontal speed divides 0 by 0 there, and NaN is its result
_singles = {}


def rollout_guarded(cfg, pos, vel, vspin, frames, resample=None):
    """v2p_ball_rollout through ctypes with the three launch arrays and all six outputs between guard rows."""
    G, n = Guarded(DEV), len(pos)
    lp, lv, ls = G.of("launch_pos", pos), G.of("launch_vel", vel), G.of("launch_vspin", vspin)
    shapes = {"traj": ((n, frames, 3), f32), "bounce_pos": ((n, 3), f32), "bounce_idx": ((n,), i64), "pass_net": ((n,), u8), "peak_after_bounce": ((n,), f32),
              "final_state": ((n, 13), f32)}
    if resample is not None:
        del shapes["traj"], shapes["peak_after_bounce"]
        shapes["traj_x"], shapes["traj_y"] = ((n, ball_traj.grid_cells(resample[0])), f32), ((n, ball_traj.grid_cells(resample[1]), 2), f32)
    assert len(shapes) == 6
    out = {k: G.empty(k, shape, dt) for k, (shape, dt) in shapes.items()}
    if resample is not None:
        for x in out.values():
            if x.dtype.is_floating_point:
                x.fill_(SENTINEL)
    c = ball_traj.sim_struct(cfg, frames, resample)
    o = _lib.BallRolloutOut(**{k: x.data_ptr() for k, x in out.items()})
    dev = torch.device(DEV)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().v2p_ball_rollout(C.byref(c), n, _lib.ptr(lp), _lib.ptr(lv), _lib.ptr(ls), C.byref(o), _lib.current_stream(dev)), "v2p_ball_rollout")
    G.check()
    got = download(out)
    for k, x in got.items():  # nothing left unwritten
        if x.dtype.kind == "f":
            assert np.isfinite(x).all() if resample is None else (x != SENTINEL).all(), "%s: elements left unwritten" % k
        else:
            assert (x != (UNWRITTEN if x.dtype == np.int64 else 0x5A)).all(), "%s: elements left unwritten" % k
    for a, b in ((lp, pos), (lv, vel), (ls, vspin)):
        assert np.array_equal(a.cpu().numpy(), b), "the roll-out wrote a launch array"
    return got


def singles(cfg, frames, resample):
    """the ten fixture launches, each as a run of one ball: the reference for value, computed once per case and shared"""
    key = (frames, resample is not None)
    if key not in _singles:
        pos, vel, vspin = B.fixture_launches()
        runs = [rollout_guarded(cfg, pos[i:i + 1], vel[i:i + 1], vspin[i:i + 1], frames, resample) for i in range(len(pos))]
        _singles[key] = {k: np.concatenate([r[k] for r in runs]) for k in runs[0]}
    return _singles[key]


@gpu
@pytest.mark.parametrize("frames", [1, 15, 17, 33])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_ball_rollout_around_the_staging_area(n, frames):
    cfg = B.fixture_cfgs()[ROLLOUT_NAME]
    pos, vel, vspin = B.fixture_launches()
    idx = np.arange(n) % len(pos)
    got = rollout_guarded(cfg, pos[idx], vel[idx], vspin[idx], frames)
    one = singles(cfg, frames, None)
    for k in got:
        assert np.array_equal(got[k], one[k][idx]), "%d balls, %d frames: %s of a ball differs from its run alone" % (n, frames, k)
    if n == 63 and frames == 17:  # the float64 oracle, at the bounds of test_rollout_matches_the_oracle
        gold = B.load_golden()
        calls, sens = gold[ROLLOUT_NAME + "/calls"], gold[ROLLOUT_NAME + "/sens"].astype(np.float64)
        top = [i for i in range(len(pos)) if i != B.BACKSPIN]
        need = B.compare_with_oracle(ROLLOUT_NAME, cfg, got["traj"][top], calls[top], sens[top], cfg["control_freq_inv"], "positions per frame, 17 frames between guards")
        assert len(set(need)) <= 2, "launches %s need the conditioning term" % sorted(set(need))


@gpu
@pytest.mark.parametrize("frames", [17, 33])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_ball_rollout_resampled_on_grids_of_7_and_13_cells(n, frames):
    cfg = dict(B.fixture_cfgs()[ROLLOUT_NAME], enable_ground=0)
    pos, vel, vspin = B.fixture_launches()
    idx = np.arange(n) % len(pos)
    got = rollout_guarded(cfg, pos[idx], vel[idx], vspin[idx], frames, RESAMPLE)
    assert got["traj_x"].shape == (n, 7) and got["traj_y"].shape == (n, 13, 2)
    one = singles(cfg, frames, RESAMPLE)
    odd = sorted(set(idx[~np.isfinite(got["traj_x"]).all(1) | ~np.isfinite(got["traj_y"]).all((1, 2))].tolist()))
    print("launches with a non-finite cell: %s" % odd)
    assert odd in ([], [B.DROP]), "only the ball dropped from rest (no horizontal speed: 0 / 0 in the interpolation) may have a non-finite cell"
    for k in got:
        assert np.array_equal(got[k], one[k][idx], equal_nan=True), "%d balls, %d frames, resampled: %s of a ball differs from its run alone" % (n, frames, k)


# ================================================================================================================== one launch too wide
def named_behind(G):
    found = G.damaged()
    assert all(side == BEHIND for _, side in found), "damage in front of a tensor: %s" % found
    return {name for name, _ in found}


def changed_rows(want, s, rows):
    """names whose rows `rows` the statement changes"""
    return {k for k, w in want.items() if s.get(k) is not None and k not in E.TABLES and np.any(np.asarray(w)[rows] != np.asarray(s[k]).reshape(np.asarray(w).shape)[rows])}


@gpu
def test_a_tennis_step_one_row_too_wide_is_named():
    """n = 3 envs of variant A, tensors built for 4 valid rows with row 3 in the back guard, the guards armed on what they hold, the launch
    with 4.  Named behind: every output, and every state tensor of tests/test_gpu_tennis_controller.py's WRITTEN whose row the statement
    changes (a store of the bits already there cannot be seen); nothing outside WRITTEN, nothing in front."""
    n, (st, _) = 3, F.settings("A")
    s = E.take(F.step_inputs("A", 0), np.arange(n + 1))
    # row 3: a fresh valid hit and a bounce in the court, so that the statement changes the contact flags, est_* and bounce_in too
    s["ball_state"][n] = E.estimator()[1]["ball_state"][0]
    s["has_racket_contact"][n], s["prev_ball_vy"][n], s["est_bounce_in"][n] = False, s["ball_state"][n, 8] - 11, True
    s["tar_action"][n], s["has_bounce_now"][n], s["bounce_pos"][n], s["bounce_in"][n] = 0, True, (0.0, 5.0, 0.0), False
    G = Guarded(DEV)
    dev = tennis_tensors(G, s, single_outputs(st), spill=1)
    assert all(len(t) == n for k, t in dev.items() if k not in E.TABLES)
    G.arm()
    G.check()
    tc.launch_step(st, dev, n + 1)
    names = named_behind(G)
    want = tc.task_step_reference(st, s)
    want.pop("sub_rewards_names")
    must = set(single_outputs(st)) | changed_rows(want, s, [n])
    print("named: %s\nmust be: %s\nmay be: %s" % (sorted(names), sorted(must), sorted(TC.WRITTEN)))
    assert must >= TC.WRITTEN - {"vel_x_overflow", "ball_obs"}, "row 3 was built so that every written tensor changes: %s do not" % sorted(TC.WRITTEN - must)
    assert names >= must, "written by the statement and not named: %s" % sorted(must - names)
    assert names <= TC.WRITTEN - {"vel_x_overflow"}, "named and believed read-only: %s" % sorted(names - TC.WRITTEN)
    F.compare({k: G.wide(k, 1).cpu().numpy() for k in want if k not in E.TABLES}, {k: w for k, w in want.items() if k not in E.TABLES}, "4 rows, the last in the guard")


@gpu
def test_a_handover_one_pair_too_wide_is_named():
    """n = 6 envs of dual variant A.  A pair is the hand-over's row (n + 1 = 7 envs are the same 3 pairs), so the tensors are built for 8
    valid rows with the pair 6, 7 in the back guard - env 6 reacts, env 7 recovers - and the launch is with 8.  Named behind: what the
    statement changes in rows 6 and 7, all of it among the keys the hand-over's test compares; nothing else, nothing in front."""
    n, st = 6, DF.settings("A")
    s = DF.inputs("hand", "A", n + 2)
    s["reset_reaction"][n:], s["reset_recovery"][n:] = [True, False], [False, True]
    # (so that the statement changes every tensor the hand-over writes: a store of the bits already there cannot be seen)
    s["tar_action"][n:], s["traj_cursor"][n:], s["bounce_in"][n], s["has_bounce"][n:], s["bounce_pos"][n:] = [0, 1], [7, 3], True, True, 1.0
    s["racket_pos"][n:] += 1.0
    s["racket_normal"][n:] += 1.0
    G = Guarded(DEV)
    dev = tennis_tensors(G, s, {}, spill=2)
    G.arm()
    G.check()
    td.launch_handover(st, dev, n + 2)
    names = named_behind(G)
    want = td.handover_reference(st, s)
    want.pop("table_rows")
    must = changed_rows(want, s, [n, n + 1])
    print("named: %s\nmust be: %s\nmay be: %s" % (sorted(names), sorted(must), sorted(want)))
    assert must == set(want), "the pair was built so that every written tensor changes: %s do not" % sorted(set(want) - must)
    assert names >= must, "written by the statement and not named: %s" % sorted(must - names)
    assert names <= set(want), "named and believed read-only: %s" % sorted(names - set(want))
    DF.compare({k: G.wide(k, 2).cpu().numpy() for k in want}, {k: np.asarray(w) for k, w in want.items()}, DF.scatter("hand"), "8 rows, the last pair in the guard")


@gpu
def test_an_imitation_target_step_one_row_too_wide_is_named():
    """n = 9 envs of variant H (the head rule writes Head and Neck back), tensors for 10 valid rows, the launch with 10.  Named behind:
    target, the three held clocks, and joint_rotmat where the recorded Head / Neck of row 9 differ from the input; nothing else."""
    n, v, t = 9, "H", 0
    g = TX.golden()
    st = TX.settings(g, v)
    plain, _, idx = TT.step_tensors(g, v, t, n + 1)
    G = Guarded(DEV)
    d = target_tensors(G, plain, n, spill=1)
    G.arm()
    G.check()
    mt.launch_step(st, d, n + 1, len(g[v + "/joint_pos_bind"]))
    names = named_behind(G)
    must = {"target", "hold_reset", "hold_progress", "hold_cur_time"}
    if np.any(TX.expected_rotmat(g, v, t, st)[idx][n] != plain["joint_rotmat"].cpu().numpy()[n]):
        must.add("joint_rotmat")
    print("named: %s\nmust be: %s" % (sorted(names), sorted(must)))
    assert names >= must, "written and not named: %s" % sorted(must - names)
    assert names <= must | {"joint_rotmat"}, "named and believed read-only: %s" % sorted(names - must)
    TX.assert_row(G.wide("target", 1).cpu().numpy(), g[v + "/target"][t + 1][idx], TX.scatter_of(g, "step"), "10 rows, the last in the guard")
