"""The match record on the device: `v2p_match_record_frame` / `v2p_match_record_select` against the numpy statement and against what the
reference's own `MVAEControllerVisDual.render_vis` left after every call (tests/golden/match_record.npz), every tensor between guard
rows; small and large batches, the overflow rule, the pose row against the evaluation's statement; and a two-player controller recorded
through `MatchPlayer` in both reset modes."""
import traceback

import numpy as np
import pytest
import torch

from tests import match_record_fixture as F
from tests import pair_reset_fixture as PX
from tests.guarded import Guarded
from vid2player3d_amd import _lib, match
from vid2player3d_amd.tasks import tennis_controller as tc

gpu = pytest.mark.gpu
DEV = "cuda:0"
ZEROS, POISON = None, {float: np.float32(np.nan), int: 0x5A5A5A5A5A5A5A5A}
STATE = tuple(k for k in _lib.MATCH_RECORD_BUFFER_NAMES if k not in _lib.MATCH_RECORD_INPUT_NAMES)  # what the entries write


def B(a):
    """the bytes of an array or tensor: NaN payloads compare like any other bits"""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def fx():
    return F.load()


class DeviceRecord:
    """The record and the inputs of the entries on the device, every tensor between guard rows; `call(s)` uploads the arrays of `s`
    and launches, `arrays()` downloads the record under the statement's names."""

    def __init__(self, st, n, fill):
        self.st, self.n, self.g = st, n, Guarded(DEV)
        rec = match.record_arrays(st, n, fill)
        self.t = {k: self.g.of(k, rec[k]) for k in STATE}
        f32, i64 = torch.float32, torch.int64
        shapes = dict(rb_state=((n, 24, 13), f32), dof_state=((n, 69, 2), f32), ball_state=((n, 13), f32), phase_pred=((n,), f32), swing_type_cycle=((n,), i64),
                      tar_action=((n,), i64), progress=((n,), i64), reset=((n,), i64), distance=((n,), f32))
        self.t.update({k: self.g.empty(k, shape, dtype) for k, (shape, dtype) in shapes.items()})
        self.structs = match.record_structs(st, n, self.t)

    def call(self, s, select=True, dof_vel=None):
        n = self.n
        dof = np.stack([np.asarray(s["dof_pos"], np.float32).reshape(n, 69), np.full((n, 69), 7.5, np.float32) if dof_vel is None else dof_vel], -1)
        for k in _lib.MATCH_RECORD_INPUT_NAMES:
            self.t[k].copy_(torch.as_tensor(dof if k == "dof_state" else s[k]).reshape(self.t[k].shape))
        match.launch_record_frame(self.structs, n, DEV)
        if select:
            match.launch_record_select(self.structs, n, DEV)
        torch.cuda.synchronize()
        self.g.check()

    def arrays(self):
        return dict(self.st, **{k: self.t[k].cpu().numpy() for k in STATE})


def assert_same_record(got, want, what):
    for k in STATE:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(B(got[k]), B(want[k])), "%s: %s differs" % (what, k)


def run_fixture(fx, fill):
    n, L, K, T = F.sizes(fx)
    st = match.record_settings(L, K, fx["body_of_smpl"])
    dev, rec = DeviceRecord(st, n, fill), match.record_arrays(st, n, fill)
    for c in range(T + 1):
        s = F.inputs(fx, c)
        dev.call(s, select=c > 0)
        rec = match.match_record_reference(rec, s, select=c > 0)
        got = dev.arrays()
        assert_same_record(got, rec, "call %d" % c)  # frames, tables, decision, kept slices; unwritten slots and unused storage at their fill
        if fill is ZEROS:
            F.compare_with_reference(fx, got, c, "call %d against the reference" % c)
        assert not got["overflow"].any()
    return got


@gpu
@pytest.mark.parametrize("fill", [ZEROS, POISON], ids=["zeros", "poison"])
def test_kernels_meet_the_fixture_and_the_statement_call_by_call(fx, fill):
    first = run_fixture(fx, fill)
    again = run_fixture(fx, fill)
    assert_same_record(again, first, "two runs")
    n, L, K, T = F.sizes(fx)
    if fill is POISON:
        written = np.zeros((n, L), bool)
        for c in range(T + 1):
            written[np.arange(n), fx["in/progress"][c]] = True
        assert np.isnan(first["phase_all"][~written]).all() and (first["swing_type_all"][~written] == POISON[int]).all() and (~written).sum() > 0
        longest = fx["best/nframes"].max()  # (what a storage slot held behind nframes stays, so the union over the run)
        assert longest < L and np.isnan(first["best_phase"][:, :, longest:]).all(), "storage no rally reached keeps its fill"


def random_script(rng, n, L, T):
    """T calls after the init call on random state: a pair finishes with probability 0.3, and always at progress L - 1; the flags of a
    finished pair are (1,1), (1,0), (0,1) or (2,-1); the distance words are halves of small integers, so that sums tie often, and grow slowly with
    the call, so that later rallies replace earlier ones."""
    calls, progress, reset = [], np.zeros(n, np.int64), np.zeros(n, np.int64)
    for c in range(T + 1):
        if c:
            progress = np.where(np.repeat((reset.reshape(-1, 2) != 0).any(1), 2), 0, progress) + 1
        rb = rng.normal(0, 1, (n, 24, 13)).astype(np.float32)
        reset = np.zeros(n, np.int64)
        if c:
            done = (rng.uniform(size=n // 2) < 0.3) | (progress[0::2] >= L - 1)
            pattern = np.array([(1, 1), (1, 0), (0, 1), (2, -1)], np.int64)[rng.integers(0, 4, n // 2)]
            reset = np.where(done[:, None], pattern, 0).reshape(-1)
        calls.append(dict(rb_state=rb, dof_pos=rng.normal(0, 1, (n, 69)).astype(np.float32), ball_state=rng.normal(0, 5, (n, 13)).astype(np.float32),
                          phase_pred=rng.uniform(0, 6.28, n).astype(np.float32), swing_type_cycle=rng.integers(-1, 4, n).astype(np.int64),
                          tar_action=rng.integers(0, 2, n).astype(np.int64), progress=progress.copy(), reset=reset,
                          distance=(rng.integers(0, 5, n) / 2.0 + c // 3).astype(np.float32)))
    return calls


@gpu
@pytest.mark.parametrize("n,L,K", [(2, 5, 1), (2, 5, 3), (6, 5, 1), (6, 5, 3), (10, 3, 16), (2060, 4, 3)])
def test_kernels_meet_the_statement_on_random_runs(n, L, K):
    """one pair, three pairs, the longest list, and more pairs (1030) than the selection's workgroup has threads, envs in more than one
    workgroup of the frame launch"""
    rng = np.random.default_rng(n * 100 + K)
    st = match.record_settings(L, K, np.concatenate([[0], 1 + rng.permutation(23)]))
    dev, rec = DeviceRecord(st, n, POISON), match.record_arrays(st, n, POISON)
    inserted = evicted = 0
    for c, s in enumerate(random_script(rng, n, L, 14)):
        if n > 2048 and c == 9:  # the maximum is reached in the second sweep of the scan alone, twice: the lower pair is taken
            s["reset"][:] = 0
            s["reset"][[2 * 1027, 2 * 1029 + 1]] = 1
            s["distance"][2 * 1027:2 * 1027 + 2] = s["distance"][2 * 1029:2 * 1029 + 2] = np.float32(50)
        full = int(rec["best_count"][0]) == K
        dev.call(s, select=c > 0)
        rec = match.match_record_reference(rec, s, select=c > 0)
        assert_same_record(dev.arrays(), rec, "n %d call %d" % (n, c))
        if n > 2048 and c == 9:
            assert rec["decision"][0] == 1027
        inserted += int(rec["decision"][0] >= 0)
        evicted += int(rec["decision"][0] >= 0 and full)
    assert inserted >= 1 and not rec["overflow"].any()
    if K < 16:
        assert evicted >= 1, "the script never replaced a kept rally"


@gpu
def test_overflow_stores_nothing_and_clips_nframes(fx):
    n, L, K, T = F.sizes(fx)
    st = match.record_settings(L, K, fx["body_of_smpl"])
    dev, rec = DeviceRecord(st, n, POISON), match.record_arrays(st, n, POISON)
    s = F.inputs(fx, 5)
    s["progress"] = np.array([L - 1, L - 1, L, L, L + 1, L + 1, -1, -1, 3, 3, 2 ** 40, -2 ** 40], np.int64)
    s["reset"][:] = 0
    s["reset"][[3, 4]] = 1
    s["distance"][:] = np.float32(1)
    s["distance"][4:6] = np.float32(2)
    dev.call(s)
    rec = match.match_record_reference(rec, s)
    got = dev.arrays()
    assert_same_record(got, rec, "progress at L - 1, L, L + 1, below zero and far outside")
    assert got["overflow"].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1] and tuple(got["decision"]) == (2, 0, L)
    assert not np.isnan(got["phase_all"][0, L - 1]) and np.isnan(got["phase_all"][2:8]).all(), "the last slot is written, then nothing"
    s["reset"][:] = 0
    s["reset"][2] = 1
    s["distance"][2:4] = np.float32(3)
    dev.call(s)
    rec = match.match_record_reference(rec, s)
    assert_same_record(dev.arrays(), rec, "a second clipped rally in front")
    assert tuple(rec["decision"]) == (1, 1, L)
    s["distance"][2] = np.float32(np.nan)
    dev.call(s)
    rec = match.match_record_reference(rec, s)
    assert_same_record(dev.arrays(), rec, "a NaN sum")
    assert tuple(rec["decision"]) == (-1, -1, 0)


@gpu
def test_pose_row_is_the_evaluations(fx):
    """`joint_rot_all[e, progress[e]]` against `eval_record_reference` - the statement the evaluation step's record is held to - on a
    scripted rigid-body / DoF state: the identity as a root rotation, w < 0, every body rotated"""
    n, L = 10, 4
    rng = np.random.default_rng(77)
    body = np.concatenate([[0], 1 + rng.permutation(23)])
    st = match.record_settings(L, 1, body)
    (s,) = random_script(rng, n, L, 0)
    q = s["rb_state"][:, 0, 3:7]
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q[1] = (0, 0, 0, 1)
    q[2, 3] = -abs(q[2, 3])
    q[3] = (0, 0, 0, -1)
    s["progress"] = rng.integers(0, L, n).astype(np.int64)
    dev = DeviceRecord(st, n, POISON)
    dev.call(s, select=False, dof_vel=rng.normal(0, 1, (n, 69)).astype(np.float32))
    want = tc.eval_record_reference(tc.eval_settings(600, body), dict(s, target_bounce_pos=np.zeros((n, 3), np.float32)))
    got = dev.arrays()
    at = (np.arange(n), s["progress"])
    assert np.array_equal(B(got["joint_rot_all"][at]), B(want["joint_rot"]))
    assert np.array_equal(B(got["root_pos_all"][at]), B(want["root_pos"])) and np.array_equal(B(got["ball_pos_all"][at]), B(want["ball_pos"]))
    assert np.array_equal(B(got["phase_all"][at]), B(want["phase"])) and np.array_equal(got["swing_type_all"][at], want["swing_type_cycle"])
    assert np.array_equal(got["tar_action_all"][at], s["tar_action"])


# ------------------------------------------------------------------------------------------------------------------ the controller
def _forced_misses(ctl, task, plan):
    """wrap `ctl.post_physics_step`: at its k-th call the envs of plan[k] (receivers: the ball flies to them) find the ball behind them -
    the dual step's law then ends the episode of their pair (as tests/test_gpu_pair_reset.py does)"""
    inner, count = ctl.post_physics_step, [0]
    index = {k: torch.as_tensor(v, dtype=torch.int64, device=DEV) for k, v in plan.items() if len(v)}  # (made here: the hook itself must not synchronise)

    def post_physics_step(*args, **kw):
        idx = index.get(count[0])
        if idx is not None:
            ctl._tar_action.index_fill_(0, idx, 1)
            root_y = task._rigid_body_state.view(ctl.num_envs, 24, 13)[:, 0, 1]
            task._ball_root_states[:, 1].index_copy_(0, idx, root_y.index_select(0, idx) - 3.0)
        count[0] += 1
        return inner(*args, **kw)

    ctl.post_physics_step = post_physics_step


N_CTL, STEPS, LENGTH = 16, 12, 16
PLAN = {1: [2], 3: [0, 6], 4: [2], 6: [10, 12], 8: [4], 10: [0, 2, 14]}  # (even envs: the receivers of a serve from 'near')


def _engine_state(ctl, task):
    n = ctl.num_envs
    t = {k: v.detach().cpu().numpy().copy() for k, v in ctl._tensors().items() if k in _lib.MATCH_RECORD_INPUT_NAMES}
    t["dof_pos"] = task._dof_state.view(n, 69, 2)[..., 0].cpu().numpy().copy()
    return t


@gpu
def test_recorded_match_flags_equals_ids_and_the_last_frame_is_the_engines():
    runs = {}
    for mode in ("ids", "flags"):
        ctl, task, player, target = PX.two_player_controller(N_CTL)
        rec = match.MatchRecorder(ctl, record_length=LENGTH, num_best=3)
        assert match.MatchRecorder(ctl, record_length=LENGTH).num_best == 1, "cfg env.num_eg, default 1"
        m = match.MatchPlayer(ctl, PX.controller_policy(ctl), mode, recorder=rec)
        _forced_misses(ctl, task, PLAN)
        pairs, distance = m.run(STEPS)
        torch.cuda.synchronize()
        best = rec.best()
        assert pairs >= sum(len(v) for v in PLAN.values()) and 1 <= len(best) <= 3
        out = {k + "_all": B(getattr(rec, k + "_all")) for k in match.FRAME_NAMES}
        out.update(overflow=B(rec.overflow), tables=np.array([(e["pair"], e["nframes"]) for e in best]), distances=np.array([e["distance"] for e in best], np.float32))
        for r, e in enumerate(best):
            assert e["joint_rot"].is_cuda and tuple(e["joint_rot"].shape) == (2, e["nframes"], 24, 3) and 1 <= e["nframes"] <= STEPS
            out.update({"best%d/%s" % (r, k): B(e[k]) for k in match.FRAME_NAMES})
            # the kept slices are the pair's slots as they stood when it finished; slot 0 is the init frame still
            assert all(np.array_equal(B(e[k][:, 0]), B(getattr(rec, k + "_all")[2 * e["pair"]:2 * e["pair"] + 2, 0])) for k in match.FRAME_NAMES)
            assert tuple(match.ball_track(e).shape) == (e["nframes"], 3)
        assert [e["distance"] for e in best] == sorted((e["distance"] for e in best), reverse=True) and not rec.overflow.any()
        # the last recorded frame against the statement on the engine's exported state
        s = _engine_state(ctl, task)
        frame = match.match_frame_reference(rec.settings, s)
        at = (np.arange(N_CTL), s["progress"])
        assert (s["progress"] >= 1).all() and (s["progress"] < LENGTH).all() and len(set(s["progress"].tolist())) >= 3
        for k in match.FRAME_NAMES:
            assert np.array_equal(B(getattr(rec, k + "_all").cpu().numpy()[at]), B(frame[k])), k
        runs[mode] = out
        task.close()
    assert runs["ids"].keys() == runs["flags"].keys()
    for k in runs["ids"]:
        assert np.array_equal(runs["flags"][k], runs["ids"][k]), "MatchPlayer with a recorder, 'flags' against 'ids': %s differs" % k


@gpu
def test_recorded_match_by_flags_makes_no_host_read():
    """the loop of `MatchPlayer` in 'flags' mode with a recorder completes under torch's sync debug mode 'error' (which
    tests/test_gpu_pair_reset.py shows to be honoured: there `reset(ids)` raises under it)"""
    ctl, task, player, target = PX.two_player_controller(N_CTL)
    rec = match.MatchRecorder(ctl, record_length=LENGTH, num_best=2)
    m = match.MatchPlayer(ctl, PX.controller_policy(ctl), "flags", recorder=rec)
    _forced_misses(ctl, task, {1: [2], 3: [0, 6]})
    torch.cuda.synchronize()
    played = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            m.play(5)
            played = ""
        except RuntimeError as e:
            played = "".join(traceback.format_exception(type(e), e, e.__traceback__))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert played == "", "the 'flags' loop of MatchPlayer with a recorder synchronised:\n" + played
    assert int(m.finished_pairs) >= 3 and len(rec.best()) >= 1 and not rec.overflow.any()
    task.close()
