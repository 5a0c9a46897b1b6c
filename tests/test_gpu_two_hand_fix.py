"""The two-hand backhand fix on the device: `v2p_two_hand_fix` against the numpy statement `two_hand_fix_reference`, every bit of the
output, every tensor between guard rows; the cap; and the two records' hooks, `MatchRecorder.best(fix_two_hand=True)` and
`TennisControllerEval.fixed_joint_rot`."""
import numpy as np
import pytest
import torch

from tests.guarded import Guarded
from vid2player3d_amd import _lib, two_hand_fix as thf
from vid2player3d_amd.model import load_baked_model
from vid2player3d_amd.mvae_target import SMPL_JOINT_NAMES

gpu = pytest.mark.gpu
DEV = "cuda:0"
# flagged frames per track: none, one (no smoothness term), two, around a wave, and past the workgroup's 256 threads (threads 0..43 own
# two frames); track 3 is left-handed
COUNTS = (0, 1, 2, 63, 64, 65, _lib.TWO_HAND_FIX_THREADS + 44)
LEFT = 3
SLACK = 5  # slots behind the longest track, poisoned like everything behind a track's nframes


def B(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def model():
    return load_baked_model()


@pytest.fixture(scope="module")
def st(model):
    return thf.fix_settings(model.body_names, model.parents)


def bind_rows(model, shapes):
    rest = np.zeros((24, 3))
    for b in range(24):
        p = int(model.parents[b])
        rest[b] = np.asarray(model.local_pos[b], dtype=np.float64) + (rest[p] if p >= 0 else 0.0)
    rest = rest[[list(model.body_names).index(nm) for nm in SMPL_JOINT_NAMES]]
    return np.stack([rest * (1.0 + 0.07 * s) for s in range(shapes)]).astype(np.float32)


def make_tracks(counts, seed=3):
    """joint_rot [T,L,24,3], phase, swing_type [T,L], nframes, righthand [T]: track t has counts[t] flagged frames in runs with gaps
    between them (a forehand inside the window, a backhand before it, a backhand behind it, in turn); what lies behind nframes[t] is
    poison - NaN poses and phases, 0x5A swing types."""
    rng = np.random.default_rng(seed)
    tracks = []
    for t, F in enumerate(counts):
        flags, left = [], F
        while left > 0:
            run = min(left, int(rng.integers(1, 9)))
            flags += [True] * run + [False] * int(rng.integers(1, 4))
            left -= run
        flags = [False, False, False] + flags
        tracks.append(np.array(flags, bool))
    L = max(len(f) for f in tracks) + SLACK
    T = len(counts)
    jr = np.full((T, L, 24, 3), np.nan, np.float32)
    phase = np.full((T, L), np.nan, np.float32)
    swing = np.full((T, L), 0x5A5A5A5A5A5A5A5A, np.int64)
    for t, flags in enumerate(tracks):
        n = len(flags)
        base = rng.uniform(-0.4, 0.4, (24, 3))
        inc = rng.uniform(-0.01, 0.01, (24, 3))
        jr[t, :n] = base + np.arange(n)[:, None, None] * inc + rng.uniform(-0.03, 0.03, (n, 24, 3))
        phase[t, :n] = rng.uniform(2.2, 4.8, n)
        swing[t, :n] = 2
        for k in np.flatnonzero(~flags):
            if k % 3 == 0:
                swing[t, k] = 1
            elif k % 3 == 1:
                phase[t, k] = rng.uniform(0.0, 2.0)
            else:
                phase[t, k] = rng.uniform(5.0, 6.2)
        assert int(thf.need_fix_reference(phase[t, :n], swing[t, :n]).sum()) == counts[t]
    nframes = np.array([len(f) for f in tracks], np.int32)
    righthand = np.array([0 if t == LEFT else 1 for t in range(T)], np.int32)
    return dict(joint_rot=jr, phase=phase, swing_type=swing, nframes=nframes, righthand=righthand)


@pytest.fixture(scope="module")
def tracks():
    return make_tracks(COUNTS)


def launch_guarded(st, s, bind, iters):
    """the launch with every tensor between guard rows; returns (out, overflow) as numpy, `out` NaN where nothing was written"""
    g = Guarded(DEV)
    t = {k: g.of(k, s[k]) for k in ("joint_rot", "phase", "swing_type", "nframes", "righthand")}
    t["bind"] = g.of("bind", bind)
    t["out"] = g.empty("out", s["joint_rot"].shape)
    t["overflow"] = g.empty("overflow", (len(s["nframes"]),), torch.int32)
    thf.launch_fix(st, t, iters)
    torch.cuda.synchronize()
    g.check()
    return t["out"].cpu().numpy(), t["overflow"].cpu().numpy()


def statement(st, s, bind, iters):
    want = np.full(s["joint_rot"].shape, np.nan, np.float32)
    for t, n in enumerate(s["nframes"]):
        want[t, :n] = thf.two_hand_fix_reference(st, s["joint_rot"][t, :n], s["phase"][t, :n], s["swing_type"][t, :n], bool(s["righthand"][t]), bind, iters)
    return want


@gpu
@pytest.mark.parametrize("shapes,iters", [(1, 1), (2, 1), (1, 2), (2, 2), (1, 500), (2, 500)])
def test_kernel_and_statement_agree_in_every_bit(model, st, tracks, shapes, iters):
    bind = bind_rows(model, shapes)
    got, overflow = launch_guarded(st, tracks, bind, iters)
    want = statement(st, tracks, bind, iters)
    assert not overflow.any()
    for t, F in enumerate(COUNTS):
        same = (B(got[t]) == B(want[t])).reshape(got[t].shape + (4,)).all(-1)
        frames = np.flatnonzero(thf.need_fix_reference(tracks["phase"][t, :tracks["nframes"][t]], tracks["swing_type"][t, :tracks["nframes"][t]]))
        moved = float(np.abs(got[t][frames] - tracks["joint_rot"][t][frames]).max()) if F else 0.0
        assert same.all(), "track %d (F = %d, %d bind rows, %d steps): %d of %d floats differ, the first at %s; the largest difference %.3g" % (
            t, F, shapes, iters, (~same).sum(), same.size, tuple(np.argwhere(~same)[0]), np.nanmax(np.abs(got[t].astype(np.float64) - want[t])))
        assert F == 0 or moved > 1e-3, "track %d: the fix moved nothing" % t
    # behind nframes nothing is written, and the poison there was not read
    for t, n in enumerate(tracks["nframes"]):
        assert np.isnan(got[t, n:]).all() and not np.isnan(got[t, :n]).any()


@gpu
def test_public_function_returns_a_new_tensor_and_zero_steps_are_the_round_trip(model, st, tracks):
    bind = bind_rows(model, 2)
    dev = {k: torch.as_tensor(v, device=DEV) for k, v in tracks.items()}
    before = B(dev["joint_rot"])
    out = thf.fix_two_hand_backhand(dev["joint_rot"], dev["phase"], dev["swing_type"], dev["nframes"], dev["righthand"], torch.as_tensor(bind, device=DEV), num_iters=0, settings=st)
    assert out.data_ptr() != dev["joint_rot"].data_ptr() and np.array_equal(B(dev["joint_rot"]), before), "the input is not modified"
    want = np.nan_to_num(statement(st, tracks, bind, 0), nan=0.0)
    for t, n in enumerate(tracks["nframes"]):
        want[t, n:] = 0.0  # (zeros behind nframes)
    assert np.array_equal(B(out), B(want))
    with pytest.raises(RuntimeError, match="no CPU path"):
        thf.fix_two_hand_backhand(dev["joint_rot"].cpu(), dev["phase"], dev["swing_type"], dev["nframes"], dev["righthand"], torch.as_tensor(bind, device=DEV))


@gpu
def test_a_track_above_the_cap_is_copied_and_refused_by_the_message(model, st):
    s = make_tracks((2, thf.MAX_FRAMES + 1), seed=5)
    bind = bind_rows(model, 1)
    got, overflow = launch_guarded(st, s, bind, 1)
    assert list(overflow) == [0, thf.MAX_FRAMES + 1]
    n = s["nframes"][1]
    assert np.array_equal(B(got[1, :n]), B(s["joint_rot"][1, :n])) and np.isnan(got[1, n:]).all(), "the track above the cap is copied whole"
    first = {k: v[:1] for k, v in s.items()}
    assert np.array_equal(B(got[0]), B(statement(st, first, bind, 1)[0])), "the other track of the launch is fixed"
    dev = {k: torch.as_tensor(v, device=DEV) for k, v in s.items()}
    with pytest.raises(ValueError, match="%d flagged frames in one track, above the cap of %d" % (thf.MAX_FRAMES + 1, thf.MAX_FRAMES)):
        thf.fix_two_hand_backhand(dev["joint_rot"], dev["phase"], dev["swing_type"], dev["nframes"], dev["righthand"], torch.as_tensor(bind, device=DEV), num_iters=1)


def _poses(rng, shape):
    return (rng.uniform(-0.4, 0.4, shape[-2:]) + rng.uniform(-0.05, 0.05, shape)).astype(np.float32)


def _flags(rng, shape):
    """phase and swing type with runs of flagged frames"""
    phase = rng.uniform(0.0, 6.2, shape).astype(np.float32)
    swing = rng.integers(1, 3, shape).astype(np.int64)
    return phase, swing


@gpu
def test_match_recorder_best_applies_the_fix_per_side():
    from tests import pair_reset_fixture as PX
    from vid2player3d_amd import match

    n, L, K, iters = 8, 40, 2, 3
    ctl, task, player, target = PX.two_player_controller(n)
    try:
        rec = match.MatchRecorder(ctl, record_length=L, num_best=K)
        rng = np.random.default_rng(11)
        phase, swing = _flags(rng, (K, 2, L))
        rec.best_joint_rot.copy_(torch.as_tensor(_poses(rng, (K, 2, L, 24, 3))))
        rec.best_phase.copy_(torch.as_tensor(phase))
        rec.best_swing_type.copy_(torch.as_tensor(swing))
        for k, v in (("best_count", [2]), ("best_slot", [1, 0]), ("best_nframes", [31, 17]), ("best_pair", [2, 0])):
            getattr(rec, k).copy_(torch.as_tensor(v, dtype=torch.int32))
        rec.best_distance.copy_(torch.as_tensor([5.0, 3.0]))
        assert not ctl.cfg_v2p.get("fix_two_hand_backhand_post")
        plain = rec.best()
        assert [e["nframes"] for e in plain] == [31, 17]
        storage = B(rec.best_joint_rot)
        fixed = rec.best(fix_two_hand=True, num_iters=iters)
        assert np.array_equal(B(rec.best_joint_rot), storage), "the storage stays as recorded"
        sides = rec.fix_sides()
        v2p = ctl.cfg_v2p
        assert v2p.get("dual_mode") == "different" and sides == [(str(v2p["player"][j]).startswith("federer"), bool(v2p["righthand"][j])) for j in range(2)]
        assert not all(skipped for skipped, _ in sides), "no side of this fixture is fixed"
        st = thf.fix_settings(task.body_names, task.body_model.parents)
        bind = thf.bind_rows_of(target).cpu().numpy()
        assert bind.shape == (n, 24, 3)
        moved = 0
        for e, f in zip(plain, fixed):
            assert (e["pair"], e["nframes"], e["distance"]) == (f["pair"], f["nframes"], f["distance"])
            for k in match.FRAME_NAMES:
                if k != "joint_rot":
                    assert np.array_equal(B(e[k]), B(f[k])), k
            for j, (skipped, rh) in enumerate(sides):
                jr = e["joint_rot"][j].cpu().numpy()
                want = jr if skipped else thf.two_hand_fix_reference(st, jr, e["phase"][j].cpu().numpy(), e["swing_type"][j].cpu().numpy(), rh, bind, iters)
                assert np.array_equal(B(f["joint_rot"][j]), B(want)), "pair %d side %d" % (e["pair"], j)
                moved += int(not np.array_equal(want, jr))
        assert moved >= 2
        ctl.cfg_v2p["fix_two_hand_backhand_post"] = True  # None follows the cfg
        follows = rec.best(num_iters=iters)
        assert all(np.array_equal(B(a["joint_rot"]), B(b["joint_rot"])) for a, b in zip(follows, fixed))
        assert all(np.array_equal(B(a["joint_rot"]), B(b["joint_rot"])) for a, b in zip(rec.best(fix_two_hand=False), plain))
    finally:
        task.close()


@gpu
def test_controller_eval_fixed_joint_rot_is_the_statement_on_its_record():
    from tests import tennis_eval_fixture as F

    n, frames, iters = 64, 20, 3
    ctl, task, player, target, policy = F.eval_controller(n, pool=F.near_pool())
    try:
        ctl.start_record(frames)
        rng = np.random.default_rng(12)
        phase, swing = _flags(rng, (frames, n))
        ctl._record["joint_rot"].copy_(torch.as_tensor(_poses(rng, (frames, n, 24, 3))))
        ctl._record["phase"].copy_(torch.as_tensor(phase))
        ctl._record["swing_type_cycle"].copy_(torch.as_tensor(swing))
        ctl.frame_index = frames - 2  # (the record's last two frames are not written yet)
        ids = [5, 63, 0]
        record = B(ctl._record["joint_rot"])
        got = ctl.fixed_joint_rot(torch.as_tensor(ids, device=DEV), num_iters=iters)
        assert tuple(got.shape) == (3, frames - 2, 24, 3) and np.array_equal(B(ctl._record["joint_rot"]), record)
        st = thf.fix_settings(task.body_names, task.body_model.parents)
        bind = thf.bind_rows_of(target).cpu().numpy()
        rh = bool(ctl.cfg_v2p.get("righthand", True))
        for k, e in enumerate(ids):
            jr = ctl.joint_rot_all[e].cpu().numpy()
            want = thf.two_hand_fix_reference(st, jr, ctl.phase_all[e].cpu().numpy(), ctl.swing_type_all[e].cpu().numpy(), rh, bind, iters)
            assert np.array_equal(B(got[k]), B(want)) and not np.array_equal(want, jr), "env %d" % e
    finally:
        task.close()
