"""GPU checks of `v2p_tennis_task_reset` (csrc/tennis_reset.hip): the flag-driven half of the single-player controller's `_reset_envs`,
between the guard rows of tests/guarded.py, against `task_reset_reference` - with the words supplied and with the kernel's own
generator, the statement then fed `device_rng.philox_words` -, the observation rows against `v2p_tennis_task_obs` bit for bit, the
independence of an env's draws from the rest of the launch, and `TennisControllerTask` under cfg v2p `task_reset: 'device'`.

Everything the launch writes but the observation is a copy, an integer or a single IEEE operation chain that numpy float32 evaluates in
the same order: compared bit for bit.  The observation rows are held to the tolerance of the task step's own test and to the bits of
`v2p_tennis_task_obs`."""
import numpy as np
import pytest
import torch

from tests import tennis_edges as E
from tests import tennis_fixture as F
from tests.guarded import Guarded
from vid2player3d_amd import device_rng as R
from vid2player3d_amd.tasks import tennis_controller as tc

gpu = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EEDC0FFEE123457
f32, i64 = torch.float32, torch.int64
DTYPES = {"wrist_link": i64, "swing_type": i64, "swing_type_cycle": i64, "tar_time_total": i64, "tar_action": i64, "tar_time": i64, "progress": i64, "traj_cursor": torch.int32,
          "vel_x_overflow": i64, "num_reset_reaction": i64, "sample_idx": i64}
BYTES = ("has_bounce", "has_bounce_now", "has_racket_contact", "has_racket_contact_now", "bounce_in", "est_bounce_in", "reset_reaction", "reset_recovery")
EXTRA = ("pool", "num_reset_reaction", "sample_idx")  # what the launch takes next to the names of v2p_tennis_buffers
TARGETS = {"A": False, "B": True, "C": "continuous", "D": True}  # the fixture variants' use_random_ball_target; B keeps the history
POOLS = {1: 1, 3: 100, 2500: 60}  # pool rows -> frames of a row
FLAGS = ((True, False), (False, True), (True, True), (False, False))  # the truth table of (reset_reaction, reset_recovery), env i has row i % 4


def make_pool(rows, frames, seed=1):
    """rows sorted by launch x over [-4, 4], as the reference's pool files are"""
    rng = np.random.default_rng(seed + rows)
    pool = rng.normal(0, 1, (rows, 7 + 3 * frames)).astype(np.float32)
    pool[:, 0] = np.sort(rng.uniform(-4, 4, rows))
    pool[:, 1], pool[:, 2] = rng.uniform(12, 13, rows), rng.uniform(1, 1.5, rows)
    pool[:, 3:6] = rng.normal(0, 1, (rows, 3)) * (3, 3, 2) + (0, -25, 4)
    pool[:, 6] = rng.uniform(5, 10, rows)
    if rows > 2:
        pool[1, 3:5] = 0  # a launch straight up: the spin axis is 0 / max(0, 1e-12)
    return pool


def case(name, n, rows, rule):
    st_task, _ = F.settings(name)
    st = dict(st_task, **tc.reset_settings(6, TARGETS[name], rule == "random", seed=SEED))
    s = E.take(F.step_inputs(name, 0), np.arange(n) % 80)
    rng = np.random.default_rng(7 * n + rows)
    s["reset_reaction"], s["reset_recovery"] = [np.array([FLAGS[i % 4][k] for i in range(n)]) for k in (0, 1)]
    ball = np.array(s["ball_state"], np.float32)
    # the near rule: balls on the other side (y > 0) left of the pool, right of it and inside it; balls on this side take the random row
    side = np.arange(n) // 4 % 4
    ball[:, 1] = np.where(side == 3, -np.abs(ball[:, 1]) - 0.1, np.abs(ball[:, 1]) + 0.1)
    ball[:, 0] = np.where(side == 0, -9.0, np.where(side == 1, 9.0, rng.uniform(-3.5, 3.5, n))).astype(np.float32)
    s["ball_state"] = ball
    s["pool"] = make_pool(rows, POOLS[rows])
    s["num_reset_reaction"] = rng.integers(0, 9, n)
    s["sample_idx"] = np.where(np.arange(n) % 8 == 0, rows - 1, rng.integers(0, rows, n)) if rule == "round_robin" else None
    s["obs"] = rng.normal(0, 1, (n, tc.obs_width(st))).astype(np.float32)
    s["racket_pos"], s["racket_normal"] = rng.normal(0, 1, (n, 3)).astype(np.float32), rng.normal(0, 1, (n, 3)).astype(np.float32)
    s["traj_cursor"] = rng.integers(0, 100, n).astype(np.int32)
    if st["use_history"]:
        s["ball_obs"] = rng.normal(0, 1, (n, st["L"], 3)).astype(np.float32)
    return st, s


def upload(G, s):
    t = {}
    for k, v in s.items():
        if v is None:
            continue
        a = np.ascontiguousarray(v)
        t[k] = G.of(k, a.astype(np.uint8), dtype=torch.uint8) if k in BYTES else G.of(k, a, dtype=DTYPES.get(k, f32))
    return t


def download(t):
    return {k: v.detach().cpu().numpy() for k, v in t.items()}


def statement_words(st, n, call, given=None):
    """the [n,8] words the statement is fed: the supplied ones, or what the kernel's generator makes of (seed, call)"""
    if given is not None:
        return given
    w = np.zeros((n, tc.RESET_WORDS), np.uint32)
    w[:, 0:4] = R.philox_words(st["seed"], call, R.STREAM_RESET, n, 1)
    w[:, 4:8] = R.philox_words(st["seed"], call, R.STREAM_RESET, 1, 1, envs=[R.WHOLE_CALL])
    return w


def run(st, s, call, words=None):
    """one launch between guards against the statement; returns (got, want, device tensors, Guarded)"""
    n = len(s["ball_state"])
    G = Guarded(DEV)
    dev = upload(G, s)
    w = None if words is None else G.of("words", words.view(np.int32), dtype=torch.int32)
    before = download(dev)
    tensors = {k: v for k, v in dev.items() if k not in EXTRA}
    tc.launch_reset(st, tensors, n, dev["pool"], dev["num_reset_reaction"], sample_idx=dev.get("sample_idx"), call=call, words=w)
    G.check()
    got = download(dev)
    want = tc.task_reset_reference(st, s, statement_words(st, n, call, words))
    return got, want, before, dev, G


def compare(st, s, got, want, before, what):
    n = len(s["ball_state"])
    rx, rc = np.asarray(s["reset_reaction"]), np.asarray(s["reset_recovery"])
    for k, w in want.items():
        if k == "pool_rows" or k not in got:
            continue
        g = got[k].reshape(np.asarray(w).shape)
        if k in ("obs", "racket_normal"):
            F.compare({k: g}, {k: w}, what)
        else:
            assert np.array_equal(g.astype(np.asarray(w).dtype) if g.dtype == np.uint8 else g, w, equal_nan=True), "%s: %s differs from the statement in rows %s" % (
                what, k, np.nonzero((g.reshape(n, -1) != np.asarray(w).reshape(n, -1)).any(1))[0][:8])
    untouched = ~(rx | rc)
    for k, v in before.items():
        if k in ("pool", "words") or k in E.TABLES:
            assert np.array_equal(v, got[k], equal_nan=True), "%s: the launch wrote %s" % (what, k)
        elif k not in tc.RESET_WRITES:
            assert np.array_equal(v, got[k], equal_nan=True), "%s: the launch wrote %s, which it only reads" % (what, k)
        else:
            assert np.array_equal(v[untouched], got[k][untouched], equal_nan=True), "%s: an env without a flag changed its %s" % (what, k)
    # what the statement leaves alone in flagged rows keeps its bits too (the flags themselves are read, not cleared)
    assert np.array_equal(got["reset_reaction"], before["reset_reaction"]) and np.array_equal(got["reset_recovery"], before["reset_recovery"])


def observation_bits(st, s, got, dev, what):
    """the rows the launch wrote equal `v2p_tennis_task_obs` of the same envs on the same state, bit for bit"""
    rx, rc = np.asarray(s["reset_reaction"]), np.asarray(s["reset_recovery"])
    ids = np.nonzero(rx | rc)[0]
    if not len(ids):
        return
    tensors = {k: v for k, v in dev.items() if k not in EXTRA + ("words",)}
    if "ball_obs" in tensors:  # the history as it stood before the launch's own roll: the reacting envs' fill, the others' old rows
        pre = np.array(s["ball_obs"], np.float32)
        pre[rx] = got["ball_state"][rx, None, 0:3]
        tensors["ball_obs"].copy_(torch.as_tensor(pre))
    for k in ("obs", "racket_pos", "racket_normal"):
        tensors[k][torch.as_tensor(ids, device=DEV)] = float("nan")
    tc.launch_obs(st, tensors, len(rx), torch.as_tensor(ids, device=DEV))
    again = download(tensors)
    for k in ("obs", "racket_pos", "racket_normal") + (("ball_obs",) if "ball_obs" in tensors else ()):
        assert np.array_equal(again[k], got[k], equal_nan=True), "%s: %s differs from v2p_tennis_task_obs in its bits" % (what, k)


def edge_words(n, seed):
    """supplied words: both edges of every integer law and of the uniform law in the first rows, random bits elsewhere; columns 4..7 are
    the whole call's and the same in every row"""
    w = np.random.default_rng(seed).integers(0, 2 ** 32, (n, tc.RESET_WORDS), dtype=np.uint64).astype(np.uint32)
    w[0::8, 0:4] = 0
    w[2::8, 0:4] = 0xFFFFFFFF
    w[:, 4:8] = w[0, 4:8]
    return w


@gpu
@pytest.mark.parametrize("n", [1, 3, 65, 130])
@pytest.mark.parametrize("name", sorted(TARGETS))
def test_kernel_against_the_statement(name, n):
    census = set()
    for rows in sorted(POOLS):
        for rule in ("random", "round_robin"):
            st, s = case(name, n, rows, rule)
            for words in (edge_words(n, rows), None):
                what = "variant %s, %d envs, pool of %d rows, %s, %s" % (name, n, rows, rule, "words given" if words is not None else "generator")
                got, want, before, dev, _ = run(st, s, 11 + n, words)
                compare(st, s, got, want, before, what)
                observation_bits(st, s, got, dev, what)
                picked = want["pool_rows"][want["pool_rows"] >= 0]
                assert picked.min() >= 0 and picked.max() < rows
                if rule == "random" and rows == 2500:
                    near = np.asarray(s["reset_reaction"]) & (np.asarray(s["ball_state"])[:, 1] > 0)
                    census |= {"low"} if (want["pool_rows"][near] == 0).any() else set()
                    census |= {"high"} if (want["pool_rows"][near] == rows - 1).any() else set()
                    census |= {"inside"} if ((want["pool_rows"][near] > 0) & (want["pool_rows"][near] < rows - 1)).any() else set()
                if rule == "round_robin":
                    rx = np.asarray(s["reset_reaction"])
                    assert np.array_equal(got["sample_idx"][rx], (np.asarray(s["sample_idx"])[rx] + 1) % rows)
    if n >= 65:
        assert census == {"low", "high", "inside"}, "the near rule's clamp was not reached at both ends and inside: %s" % sorted(census)
    tt = got["tar_time_total"][np.asarray(s["reset_reaction"])]
    assert tt.min() >= 1 and tt.max() <= 10


@gpu
def test_law_edges_reach_the_state():
    """w = 0 and w = 0xffffffff in every per-env word: the first and the last pool row, reaction times nframes - 5 and nframes + 4, the
    left and the right target"""
    st, s = case("B", 16, 2500, "random")
    s["reset_reaction"][:], s["reset_recovery"][:] = True, False
    s["ball_state"][:, 1] = -1.0  # this side: the random row
    words = edge_words(16, 5)
    got, want, before, dev, _ = run(st, s, 0, words)
    compare(st, s, got, want, before, "law edges")
    assert want["pool_rows"][0] == 0 and want["pool_rows"][2] == 2499
    assert np.array_equal(got["ball_state"][[0, 2], 0:3], s["pool"][[0, 2499], 0:3])
    assert got["tar_time_total"][0] == 1 and got["tar_time_total"][2] == 10
    assert got["target_bounce_pos"][0].tolist() == [-3.0, 10.0, 0.0] and got["target_bounce_pos"][2].tolist() == [3.0, 10.0, 0.0]
    assert (got["tar_action"] == 1).all() and (got["tar_time"] == 0).all() and (got["swing_type_cycle"] == -1).all() and (got["traj_cursor"] == 0).all()
    assert not got["has_bounce"].any() and not got["has_racket_contact"].any() and not got["bounce_pos"].any()
    assert np.array_equal(got["ball_traj"].reshape(16, 100, 3)[0, :60], s["pool"][0, 7:].reshape(60, 3)) and not got["ball_traj"].reshape(16, 100, 3)[:, 60:].any()
    # the continuous target is one draw for the whole call
    st, s = case("C", 16, 3, "random")
    s["reset_reaction"][:] = True
    got, want, before, dev, _ = run(st, s, 4)
    compare(st, s, got, want, before, "continuous target")
    tg = got["target_bounce_pos"]
    assert (tg == tg[0]).all() and (tg[0] >= [-3, 9, 0]).all() and (tg[0] <= [3, 11, 0]).all() and tg[0, 2] == 0
    u = R.uniform(R.philox_words(SEED, 4, R.STREAM_RESET, 1, 1, envs=[R.WHOLE_CALL])[0, :3])
    assert np.array_equal(tg[0], u * (np.float32([3, 11, 0]) - np.float32([-3, 9, 0])) + np.float32([-3, 9, 0]))


@gpu
def test_an_envs_draws_are_its_own():
    st, s = case("B", 130, 2500, "random")
    s["reset_reaction"][:], s["reset_recovery"][:] = True, False
    s["ball_state"][:, 1] = -1.0  # this side: the random row
    big, _, _, _, _ = run(st, s, 9)
    small, _, _, _, _ = run(st, E.take(s, np.arange(65)) | {"pool": s["pool"]}, 9)
    keys = ("ball_state", "ball_traj", "tar_time_total", "target_bounce_pos", "obs")
    for k in keys:
        assert np.array_equal(big[k][:65], small[k], equal_nan=True), "rows 0..64 of 130 envs and of 65 envs differ in %s" % k
    flipped = dict(s, reset_reaction=np.arange(130) % 2 == 1)
    other, _, before, _, _ = run(st, flipped, 9)
    for k in keys:
        assert np.array_equal(other[k][1::2], big[k][1::2], equal_nan=True) and np.array_equal(other[k][0::2], before[k][0::2], equal_nan=True), k  # (the fixture has NaN rows)
    nxt, _, _, _, _ = run(st, s, 10)
    assert (nxt["tar_time_total"] != big["tar_time_total"]).mean() > 0.5 and (nxt["ball_state"][:, 0] != big["ball_state"][:, 0]).mean() > 0.9


# ------------------------------------------------------------------------------------------------------------------ the controller
def make_controller(mode, n=8):
    from tests.gpu_util import synth_tables
    from vid2player3d_amd import ball_traj
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    torch.manual_seed(7)
    tg = F.golden()
    online = ball_traj.TennisBallGenerator({"num_samples": 500}, device=DEV, seed=3)
    gen = ball_traj.TennisBallGeneratorOffline(online.rows(), sample_random=True, device=DEV, seed=3)
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = dict(ball_generator=gen, restitution=1.4, ball_friction=0.2, spin_scale=5, reward_type="return_w_estimate", reward_weights={"pos": 0.5, "ball_pos": 0.5},
                      court_min=[-30.0, -30.0], court_max=[30.0, 30.0], obs_ball_traj_length=10, reset_reaction_nframes=6, ball_traj_out_x_file=tg["traj_out_x"],
                      ball_traj_out_y_file=tg["traj_out_y"], use_random_ball_target=True)
    if mode is not None:
        cfg["v2p"]["task_reset"] = mode
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)

    class SmallGrid:
        VEL_X_RANGE, VEL_Y_RANGE, VSPIN_RANGE, TRAJ_X_RANGE, TRAJ_Y_RANGE = [tuple(r) for r in tg["grids"]]

    return task, tc.TennisControllerTask(task, {"env": {"episodeLength": 300}, "v2p": cfg["v2p"]}, params=SmallGrid, seed=SEED), gen


def script(task, ctl, gen, steps=16, device_path=False):
    """16 control steps of the racket + ball batch with zero PD actions: hits and misses are forced through the task's flags, `reset(ids)`
    is called on two envs twice.  Under the device path every reset is checked against the statement run on the arrays from before it.
    Returns the state after the last step."""
    n = ctl.num_envs
    task.reset()
    resets = 0

    def checked_reset(ids):
        nonlocal resets
        before = ctl.state_arrays()
        before.update(pool=gen.data.cpu().numpy(), num_reset_reaction=ctl._num_reset_reaction.cpu().numpy().copy())
        before["num_reset_reaction"][np.asarray(ids, np.int64)] = 0  # (`_reset_env_tensors` of env_ids, in front of the launch)
        flags = before["reset_reaction"].astype(bool) | before["reset_recovery"].astype(bool)
        call = ctl._reset_calls
        ctl.reset(ids)
        torch.cuda.synchronize()
        if not device_path:
            return
        assert ctl._reset_calls == call + 1
        st = dict(ctl.settings, **ctl.reset_settings)
        ids = np.asarray(ids, np.int64)
        # the humanoid part of `reset(ids)` moves tensors the statement reads (pose, clocks): it is fed the state after that part
        after = ctl.state_arrays()
        for k in ("rb_state", "root_states", "racket_state", "progress", "reset", "terminate", "distance", "phase_pred", "swing_type"):
            before[k] = after[k]
        want = tc.task_reset_reference(st, before, statement_words(st, n, call))
        got = dict(after, num_reset_reaction=ctl._num_reset_reaction.cpu().numpy())
        want["reset_reaction"], want["reset_recovery"] = before["reset_reaction"].copy(), before["reset_recovery"].copy()
        want["reset_reaction"][ids], want["reset_recovery"][ids] = False, False  # the two flags of env_ids are cleared, the others stay
        for k, w in want.items():
            if k in ("pool_rows", "sample_idx"):
                continue
            g = got[k].reshape(np.asarray(w).shape)
            if k in ("obs", "racket_normal"):
                F.compare({k: g}, {k: w}, "controller reset %d" % call)
            else:
                assert np.array_equal(g.astype(np.asarray(w).dtype), w, equal_nan=True), "controller reset %d: %s differs from the statement" % (call, k)
        resets += int(flags.sum())

    checked_reset(np.arange(n))
    hits = misses = 0
    for k in range(steps):
        task.step(torch.zeros((n, 75), device=DEV))
        if k in (3, 9):  # a forced hit of env 1 (the flag the engine would set), a forced miss of env 2 (the ball behind the player)
            task._has_racket_ball_contact[1] = True
            task._ball_root_states[2, 1] = task._rigid_body_state.view(n, 24, 13)[2, 0, 1] - 2.0
        ctl.post_physics_step(torch.full((n,), 3.0, device=DEV), torch.zeros(n, dtype=i64, device=DEV))
        torch.cuda.synchronize()
        rec = ctl._reset_recovery_buf.cpu().numpy()
        if k in (3, 9):
            hits, misses = hits + int(rec[1]), misses + int(rec[2])
        ids = ctl.reset_buf.nonzero(as_tuple=False).flatten().cpu().numpy()
        if k in (5, 11):
            ids = np.union1d(ids, [0, n - 1])
        checked_reset(ids)
    assert hits >= 1 and misses >= 1, "the forced hit (%d) or miss (%d) did not reach the flags" % (hits, misses)
    return {k: v for k, v in ctl.state_arrays().items()}, resets


@gpu
def test_controller_resets_on_the_device():
    """`task_reset: 'device'` over 16 control steps: after every reset the controller's arrays equal the statement run on the arrays from
    before it; the engine flies the ball the kernel wrote."""
    task, ctl, gen = make_controller("device")
    final, resets = script(task, ctl, gen, device_path=True)
    assert resets >= 12, "too few flagged envs went through the launch: %d" % resets
    # the engine flies the ball the kernel wrote: one more step moves it by its launch velocity x dt, to first order
    ctl._reset_reaction_buf[:] = True
    ctl.reset([])
    torch.cuda.synchronize()
    b0 = task._ball_root_states.cpu().numpy().copy()
    rows = gen.data.cpu().numpy()
    assert all((rows[:, 0:6] == np.concatenate([b[0:3], b[7:10]])).all(1).any() for b in b0), "a ball state is no row of the pool"
    task.step(torch.zeros((ctl.num_envs, 75), device=DEV))
    torch.cuda.synchronize()
    b1 = task._ball_root_states.cpu().numpy()
    assert np.abs(b1[:, 0:2] - (b0[:, 0:2] + b0[:, 7:9] * task.dt)).max() < 0.05 and (b1[:, 1] < b0[:, 1]).all(), "the ball did not fly from the state the kernel wrote"
    assert np.isfinite(ctl.obs_buf.cpu().numpy()).all()
    task.close()


@gpu
def test_default_reset_is_the_parents_torch_path():
    """cfg without `task_reset`, and with 'torch': the parent's path - the same script gives the same bits either way, and draws from
    torch's generators as before (the launch counter of the device path stays 0).  A generator that is no offline pool on the task's
    device is refused under 'device'."""
    from vid2player3d_amd import ball_traj

    finals = []
    for mode in (None, "torch"):
        task, ctl, gen = make_controller(mode)
        final, _ = script(task, ctl, gen)
        assert ctl._reset_calls == 0
        finals.append(final)
        task.close()
    for k in finals[0]:
        assert np.array_equal(finals[0][k], finals[1][k], equal_nan=True), k
    digest = {k: float(np.nansum(np.asarray(v, dtype=np.float64))) for k, v in sorted(finals[0].items()) if k in ("ball_state", "obs", "tar_time_total", "target_bounce_pos", "rew")}
    print("default path, sums after the script: %s" % digest)
    task, ctl, gen = make_controller(None)
    task._ball_generator = ball_traj.TennisBallGenerator({"num_samples": 200}, device=DEV, seed=3)
    with pytest.raises(NotImplementedError, match="TennisBallGeneratorOffline"):
        tc.TennisControllerTask(task, dict(ctl.cfg, v2p=dict(ctl.cfg_v2p, task_reset="device")))
    with pytest.raises(ValueError, match="task_reset"):
        tc.TennisControllerTask(task, dict(ctl.cfg, v2p=dict(ctl.cfg_v2p, task_reset="kernel")))
    task.close()
