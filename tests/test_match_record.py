"""The match record without a GPU: the numpy statement (`match_record_reference`) against what the reference's own
`MVAEControllerVisDual.render_vis` left after every call (tests/golden/match_record.npz), the census of cases that fixture must hold,
the overflow rule (which the reference cannot show: it raises), `ball_track`, the refusals of `MatchRecorder`, `MatchPlayer(recorder=...)`
and the two entries, and the boundary."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import match_record_fixture as F
from vid2player3d_amd import _lib, match


@pytest.fixture(scope="module")
def fx():
    return F.load()


def settings(fx, num_best=None, record_length=None):
    n, L, K, T = F.sizes(fx)
    return match.record_settings(record_length or L, num_best or K, fx["body_of_smpl"])


compare_with_reference = F.compare_with_reference


def test_the_statement_meets_the_reference_call_by_call(fx):
    n, L, K, T = F.sizes(fx)
    st = settings(fx)
    rec = match.record_arrays(st, n)
    for c in range(T + 1):
        s = F.inputs(fx, c)
        before = {k: np.array(v) for k, v in s.items()}
        new = match.match_record_reference(rec, s, select=c > 0)
        assert all(np.array_equal(s[k], before[k]) for k in s), "the statement modifies nothing it is given"
        compare_with_reference(fx, new, c, "call %d" % c)
        want = fx["inserted"][c]
        assert (new["decision"][0] >= 0) == want
        if want:
            ranks = range(int(new["best_count"][0]))
            assert any(tuple(new["decision"]) == (new["best_pair"][r], new["best_slot"][r], new["best_nframes"][r]) for r in ranks), "the decision names a kept rank"
        else:
            assert tuple(new["decision"]) == (-1, -1, 0)
        slots = new["best_slot"][:int(new["best_count"][0])]
        assert len(set(slots.tolist())) == len(slots) and ((slots >= 0) & (slots < K)).all(), "a storage slot holds one rank"
        rec = new


def test_num_best_one_keeps_the_best_rally_of_the_reference(fx):
    """the list of num_eg = 1 is not the head of the list of 3 (an insertion needs d > list[-1]): here both hold the overall best"""
    n, L, K, T = F.sizes(fx)
    rec = match.record_arrays(settings(fx, num_best=1), n)
    for c in range(T + 1):
        rec = match.match_record_reference(rec, F.inputs(fx, c), select=c > 0)
        if rec["best_count"][0]:
            assert (rec["best_slot"] == 0).all()
    (best,) = match.best_of(rec)
    dist, pair, nframes, frames = F.reference_best(fx, T)[0]
    assert np.float32(best["distance"]) == dist and best["pair"] == pair and best["nframes"] == nframes and np.array_equal(best["joint_rot"], frames["joint_rot"])


def test_the_fixture_holds_every_case(fx):
    found = F.census(fx)
    assert all(found[k] for k in F.CASES), found
    n, L, K, T = F.sizes(fx)
    assert (n, L, K) == (12, 8, 3) and fx["in/progress"].max() < L, "progress >= L is not in the fixture: the reference raises there"
    assert not fx["in/reset"][0].any() and not fx["in/progress"][0].any(), "call 0 is the init frame: after the first reset"
    # slot 0 is written by the init call alone
    for c in range(1, T + 1):
        assert all(np.array_equal(fx["all/" + k][c][:, 0], fx["all/" + k][0][:, 0]) for k in F.FRAME_NAMES)


def test_overflow_stores_nothing_and_clips_nframes(fx):
    n, L, K, T = F.sizes(fx)
    st = settings(fx)
    fill = {float: np.float32(np.nan), int: -7}
    rec = match.record_arrays(st, n, fill)
    s = F.inputs(fx, 5)
    s["progress"] = np.array([L - 1, L - 1, L, L, L + 1, L + 1, -1, -1, 3, 3, 0, 0], np.int64)
    s["reset"][:] = 0
    s["reset"][[3, 4]] = 1            # either word of a pair: pairs 1 (progress L) and 2 (progress L + 1) finish
    s["distance"][:] = np.float32(1)
    s["distance"][4:6] = np.float32(2)
    new = match.match_record_reference(rec, s)
    assert new["overflow"].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    frame = match.match_frame_reference(st, s)
    for k in F.FRAME_NAMES:
        a = new[k + "_all"]
        assert np.array_equal(a[0, L - 1], frame[k][0]) and np.array_equal(a[8, 3], frame[k][8]) and np.array_equal(a[10, 0], frame[k][10])
        untouched = np.ones(a.shape[:2], bool)
        untouched[[0, 1], L - 1] = untouched[[8, 9], 3] = untouched[[10, 11], 0] = False
        assert np.array_equal(a[untouched], rec[k + "_all"][untouched], equal_nan=True), "nothing else is written"
    assert tuple(new["decision"]) == (2, 0, L) and new["best_nframes"][0] == L, "nframes = min(progress, L)"
    s["reset"][:] = 0
    s["reset"][2] = 1
    s["distance"][2:4] = np.float32(3)
    again = match.match_record_reference(new, s)
    assert tuple(again["decision"]) == (1, 1, L) and again["best_pair"].tolist()[:2] == [1, 2]
    s["distance"][2] = np.float32(np.nan)
    assert tuple(match.match_record_reference(new, s)["decision"]) == (-1, -1, 0), "a NaN sum is no candidate"


def test_ball_track():
    ball = torch.arange(24, dtype=torch.float32).reshape(2, 4, 3) + 1
    entry = dict(ball_pos=ball, tar_action=torch.tensor([[1, 0, 1, 2], [0, 1, 0, 1]]))
    keep = ball.clone()
    track = match.ball_track(entry)
    far = ball[1] * torch.tensor([-1.0, -1.0, 1.0])
    assert torch.equal(track, torch.stack([ball[0, 0], far[1], ball[0, 2], far[3]]))
    assert torch.equal(entry["ball_pos"], keep), "on a copy"
    assert match.MatchRecorder.ball_track is match.ball_track


def test_settings_recorder_and_player_refusals(fx):
    from vid2player3d_amd.policies import ControllerPolicy
    from vid2player3d_amd.tasks import tennis_controller as tc
    from vid2player3d_amd.tasks.tennis_controller_dual import DualTennisControllerTask

    assert match.record_settings()["record_length"] == 1800 and match.MAX_BEST == 16
    for bad in (0, -1, 17):
        with pytest.raises(ValueError, match="num_best"):
            match.record_settings(8, bad)
    for bad in (0, -5, (1 << 20) + 1):
        with pytest.raises(ValueError, match="record_length"):
            match.record_settings(bad, 1)
    with pytest.raises(ValueError, match="permutation"):
        match.record_settings(8, 1, [1, 0] + list(range(2, 24)))
    with pytest.raises(ValueError, match="permutation"):
        match.record_settings(8, 1, [0, 1, 1] + list(range(3, 24)))
    for n in (0, 7, -2):
        with pytest.raises(ValueError, match="even"):
            match.record_arrays(settings(fx), n)
    with pytest.raises(ValueError, match="missing"):
        match.record_structs(settings(fx), 12, {})
    rec = match.record_arrays(settings(fx), 12)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        match.record_structs(settings(fx), 12, {k: torch.zeros(4) for k in _lib.MATCH_RECORD_BUFFER_NAMES})
    assert set(k for k, v in rec.items() if isinstance(v, np.ndarray)) | set(_lib.MATCH_RECORD_INPUT_NAMES) == set(_lib.MATCH_RECORD_BUFFER_NAMES)
    with pytest.raises(TypeError, match="DualTennisControllerTask"):
        match.MatchRecorder(tc.TennisControllerTask.__new__(tc.TennisControllerTask))
    ctl = DualTennisControllerTask.__new__(DualTennisControllerTask)
    policy = ControllerPolicy.__new__(ControllerPolicy)
    policy.ctl, ctl.device = ctl, "cpu"
    with pytest.raises(ValueError, match="MatchRecorder over the same controller"):
        match.MatchPlayer(ctl, policy, "flags", recorder=object())
    other = match.MatchRecorder.__new__(match.MatchRecorder)
    other.ctl = DualTennisControllerTask.__new__(DualTennisControllerTask)
    with pytest.raises(ValueError, match="MatchRecorder over the same controller"):
        match.MatchPlayer(ctl, policy, "flags", recorder=other)
    other.ctl = ctl
    assert match.MatchPlayer(ctl, policy, "flags", recorder=other).recorder is other and match.MatchPlayer(ctl, policy).recorder is None


def test_the_entries_are_exported_and_the_abi_stands():
    L = _lib.load()
    for name in ("v2p_match_record_frame", "v2p_match_record_select"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.v2p_abi_version() == 15
    assert C.sizeof(_lib.MatchRecordCfg) == 8 + 4 + 24 * 4 + 4 and C.sizeof(_lib.MatchRecordBuffers) == 28 * 8 == 8 * len(_lib.MATCH_RECORD_BUFFER_NAMES)


@pytest.mark.parametrize("entry", ("v2p_match_record_frame", "v2p_match_record_select"))
def test_the_entries_refuse_bad_arguments_without_a_gpu(entry):
    """every call below is refused before anything is dereferenced or launched: the pointers are placeholders"""
    L = _lib.load()
    fn = getattr(L, entry)
    one = 16

    def cfg(record_length=8, num_best=3, body=None):
        c = _lib.MatchRecordCfg(record_length=record_length, num_best=num_best)
        c.body_of_smpl[:] = list(range(24)) if body is None else body
        return c

    bufs = lambda **kw: _lib.MatchRecordBuffers(**dict({k: one for k in _lib.MATCH_RECORD_BUFFER_NAMES}, **kw))
    call = lambda c, n, b: fn(C.byref(c), n, C.byref(b), None)
    err = lambda: L.v2p_last_error().decode()
    for n in (0, -2):
        assert call(cfg(), n, bufs()) == -1 and "n %d <= 0" % n in err() and entry in err()
    assert call(cfg(), 7, bufs()) == -1 and "odd" in err()
    assert call(cfg(), 2 ** 31, bufs()) == -1 and "2^31-1" in err()
    for k in _lib.MATCH_RECORD_BUFFER_NAMES:
        assert call(cfg(), 12, bufs(**{k: None})) == -1 and "null array" in err(), k
    for bad in (0, -1, (1 << 20) + 1):
        assert call(cfg(record_length=bad), 12, bufs()) == -1 and "record_length" in err()
    for bad in (0, -1, 17):
        assert call(cfg(num_best=bad), 12, bufs()) == -1 and "num_best" in err()
    for body in ([0, 1, 1] + list(range(3, 24)), [1, 0] + list(range(2, 24)), [0, 24] + list(range(2, 24)), [0, -1] + list(range(2, 24))):
        assert call(cfg(body=body), 12, bufs()) == -1 and "permutation" in err()
    assert fn(None, 12, C.byref(bufs()), None) == -1 and "null cfg" in err()
    assert fn(C.byref(cfg()), 12, None, None) == -1 and "null cfg" in err()


def test_record_init_refuses_a_controller_whose_tensors_moved():
    """the recorder keeps the structs of its launches with the tensors they name; `record_init()` compares addresses on the host"""
    import types

    names = [k for k in _lib.MATCH_RECORD_INPUT_NAMES if k != "dof_state"]
    tensors = {k: torch.zeros(4) for k in names}
    ctl = types.SimpleNamespace(_mvae_player=object(), _tensors=lambda: tensors, task=types.SimpleNamespace(_dof_state=torch.zeros(4)))
    rec = match.MatchRecorder.__new__(match.MatchRecorder)
    rec.ctl, rec._bound = ctl, None
    rec._check_bound()  # (nothing bound yet)
    rec._bound = (None, dict(rec._sources()))
    rec._check_bound()
    tensors["phase_pred"] = torch.zeros(4)
    ctl.task._dof_state = torch.zeros(4)
    with pytest.raises(RuntimeError, match=r"dof_state, phase_pred moved .* rebind\(\)"):
        rec._check_bound()
    rec.rebind()
    rec._check_bound()
    ctl._mvae_player = None
    with pytest.raises(RuntimeError, match="no motion generator"):
        rec._sources()
