"""The controller's evaluation step without a GPU: the numpy statements (`eval_step_reference`, `eval_record_reference`, `select_best`)
against what the reference's own `MVAEControllerVis` recorded (tests/golden/tennis_eval.npz), the census of cases that fixture must
hold, the refusals of `TennisControllerEval`, `ControllerEvalPlayer` and `v2p_tennis_eval_step`, and the boundary."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tennis_eval_fixture as F
from vid2player3d_amd import _lib
from vid2player3d_amd.tasks import tennis_controller as tc


@pytest.mark.parametrize("name", F.VARIANTS)
def test_numpy_statements_meet_the_reference_step_by_step(name):
    st, est = F.settings(name)
    for t in range(F.steps()):
        s = F.step_inputs(name, t)
        got = tc.eval_step_reference(st, est, s)
        got["record"] = tc.eval_record_reference(est, s)
        want = F.step_expected(name, t)
        F.compare(name, got, want, "%s step %d" % (name, t))
        assert np.array_equal(got["distance"], s["distance"]), "the test-mode step does not touch _distance"
        assert got["sub_rewards_names"] == F.golden()[name + "/sub_rewards_names"].tobytes().decode()


@pytest.mark.parametrize("name", F.VARIANTS)
def test_select_best_gives_the_references_order(name):
    d = F.golden()
    root = torch.from_numpy(np.ascontiguousarray(np.swapaxes(d[name + "/rec/root_pos"], 0, 1)))  # [N,T,3], the reference's layout
    avg = d[name + "/post/meter_avg"][-1]
    ids = tc.select_best(root, torch.from_numpy(avg[tc.METER_NAMES.index("bounce_in_rate")]), torch.from_numpy(avg[tc.METER_NAMES.index("fh_ratio")]))
    assert ids.tolist() == d[name + "/best/ids"].tolist() and len(ids) >= 2
    dist = d[name + "/best/dist"][ids.numpy()]
    assert (np.diff(dist) < 0).all(), "the candidates' distances differ and descend"
    in_rate, fh = avg[2], avg[1]
    assert ((in_rate <= 0.95) & (fh < 0.6)).any() and ((in_rate > 0.95) & (fh >= 0.6)).any(), "an env fails each of the two conditions alone"


@pytest.mark.parametrize("name", F.VARIANTS)
def test_the_fixture_holds_every_case_of_the_law_and_the_meters(name):
    d, (st, est) = F.golden(), F.settings(name)
    T, EL = F.steps(), est["episode_length"]
    seen = dict.fromkeys(("react_hit_bounced", "react_hit_no_bounce", "react_miss", "recover_hit", "recover_behind", "recover_slow", "reset_over_recovery", "reset_over_reaction",
                          "at_length", "past_length", "error_skipped", "max_rises", "max_stays", "nan_kept", "out_kept"), 0)
    fh_types = set()
    post = lambda k, t: d["%s/post/%s" % (name, k)][t]
    for t in range(T):
        s, want = F.step_inputs(name, t), F.step_expected(name, t)
        hit, act0, in_time = post("has_racket_contact", t).astype(bool), s["tar_action"] == 0, post("tar_time", t) >= s["tar_time_total"]
        bounced, done = s["has_bounce"].astype(bool), post("reset", t) > 0
        root_y, ball = s["rb_state"][:, 0, 1], s["ball_state"]
        behind, slow = ball[:, 1] < root_y - np.float32(1), np.abs(ball[:, 8]) < 2
        react, recover = post("reset_reaction", t).astype(bool), post("reset_recovery", t).astype(bool)
        # every float compared with a threshold stays 1e-3 away from it
        assert np.abs(np.abs(ball[:, 8]) - 2).min() > 1e-3 and np.abs(ball[:, 1] - (root_y - 1)).min() > 1e-3
        progress = post("progress", t)
        assert np.array_equal(done, progress > EL) and np.array_equal(post("terminate", t), post("reset", t))
        seen["react_hit_bounced"] += int((hit & act0 & bounced & in_time & ~done & react).sum())
        seen["react_hit_no_bounce"] += int((hit & act0 & ~bounced & in_time & ~done & ~react).sum())
        seen["react_miss"] += int((~hit & in_time & ~done & react).sum())
        swing = ~act0 & ~done
        seen["recover_hit"] += int((swing & hit & ~behind & ~slow & recover).sum())
        seen["recover_behind"] += int((swing & ~hit & behind & ~slow & recover).sum())
        seen["recover_slow"] += int((swing & ~hit & ~behind & slow & recover).sum())
        seen["reset_over_recovery"] += int((done & ~act0 & (hit | behind | slow) & ~recover).sum())
        seen["reset_over_reaction"] += int((done & ~((hit & act0 & bounced & in_time) | (~hit & in_time)) & react).sum())
        seen["at_length"] += int(((progress == EL) & ~done).sum())
        seen["past_length"] += int(((progress == EL + 1) & done).sum())
        est_in = post("est_bounce_in", t).astype(bool)
        grown = post("meter_count", t) - s["meter_count"]
        assert np.array_equal(grown[0], recover) and np.array_equal(grown[1], recover) and np.array_equal(grown[2], recover) and np.array_equal(grown[3], recover & est_in)
        seen["error_skipped"] += int((recover & ~est_in).sum())
        rose = post("meter_max", t) > s["meter_max"]
        seen["max_rises"] += int(rose.sum())
        seen["max_stays"] += int(((grown > 0) & ~rose & (s["meter_max"] > 0)).sum())
        fh_types |= set(int(x) for x in s["swing_type_cycle"][recover])
        nan_row = np.isnan(want["obs"]).any(1)
        cmin, cmax = st["court_min"], st["court_max"]
        root = s["rb_state"][:, 0]
        outside = (root[:, 0] < cmin[0]) | (root[:, 1] < cmin[1]) | (root[:, 0] > cmax[0]) | (root[:, 1] > cmax[1])
        seen["nan_kept"] += int((nan_row & ~done).sum())
        seen["out_kept"] += int((outside & ~done).sum())
        # ---- the law is not the training law: on the rows the census marks, task_step_reference decides otherwise
        train = tc.task_step_reference(st, s)
        for rows, what in ((nan_row & ~done, "NaN row"), (outside & ~done, "out-of-court row")):
            assert (train["reset"][rows] == 1).all() and (post("reset", t)[rows] == 0).all(), what  # (nan_kept / out_kept count the rows)
        slow_only = swing & ~hit & ~behind & slow
        if slow_only.any():
            assert not train["reset_recovery"][slow_only].any() and recover[slow_only].all(), "a slow ball raises the recovery flag in the test law only"
        assert not np.array_equal(train["distance"], s["distance"]) and np.array_equal(post("distance", t), s["distance"])
    assert all(v >= 1 for v in seen.values()), seen
    assert {-1, 1, 2} <= fh_types
    counts = d[name + "/post/meter_count"][-1][0]
    assert (counts == 0).any() and (counts == 1).any() and (counts >= 3).any(), "a meter updated 0, 1 and at least 3 times on one env"
    assert np.array_equal(d[name + "/pre/meter_avg"][0], np.ones((4, len(counts)), np.float32)) and not d[name + "/pre/meter_sum"][0].any()


def test_eval_settings_and_controller_refusals():
    assert tc.eval_settings()["episode_length"] == 600
    with pytest.raises(ValueError, match="permutation"):
        tc.eval_settings(600, [1] + list(range(1, 24)))
    with pytest.raises(ValueError, match="enableEarlyTermination"):
        tc.TennisControllerEval(None, {"env": {"episodeLength": 600, "enableEarlyTermination": True}, "v2p": {}})
    with pytest.raises(ValueError, match="body_of_smpl"):
        tc.eval_record_reference(tc.eval_settings(), {})


def test_eval_player_refusals():
    from vid2player3d_amd.eval_player import ControllerEvalPlayer
    from vid2player3d_amd.tasks.tennis_controller_dual import DualTennisControllerTask

    with pytest.raises(TypeError, match="MatchPlayer"):
        ControllerEvalPlayer(DualTennisControllerTask.__new__(DualTennisControllerTask), None)
    with pytest.raises(TypeError, match="TennisControllerEval"):
        ControllerEvalPlayer(tc.TennisControllerTask.__new__(tc.TennisControllerTask), None)
    ctl = tc.TennisControllerEval.__new__(tc.TennisControllerEval)
    with pytest.raises(ValueError, match="ControllerPolicy"):
        ControllerEvalPlayer(ctl, None)


def test_the_entry_is_exported_and_the_abi_stands():
    L = _lib.load()
    assert "v2p_tennis_eval_step" in _lib.EXPORTED_SYMBOLS and hasattr(L, "v2p_tennis_eval_step")
    assert L.v2p_abi_version() == 15
    assert C.sizeof(_lib.TennisEvalCfg) == 8 + 8 + 24 * 4 and C.sizeof(_lib.TennisEvalBuffers) == 23 * 8


def test_the_entry_refuses_bad_arguments_without_a_gpu():
    """every call below is refused before anything is dereferenced or launched: the pointers are placeholders"""
    L = _lib.load()
    st, est = F.settings("V")
    one = 16
    c = tc.cfg_struct(st, (4, 4), (4, 4, 2))
    b = _lib.TennisBuffers(**{k: one for k in _lib.TENNIS_BUFFER_NAMES})

    def bufs(record=True, **kw):
        x = _lib.TennisEvalBuffers()
        for f in tc.METER_FIELDS:
            getattr(x, f)[:] = [one] * 4
        if record:
            for k in ("dof_state",) + tc.RECORD_NAMES:
                setattr(x, k, one)
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    ec = _lib.TennisEvalCfg(episode_length=600, num_frames=5)
    ec.body_of_smpl[:] = est["body_of_smpl"]
    call = lambda n, x, frame, cfg=ec: L.v2p_tennis_eval_step(C.byref(c), C.byref(cfg), n, C.byref(b), C.byref(x), frame, None, None)
    err = lambda: L.v2p_last_error().decode()
    for n in (0, -3):
        assert call(n, bufs(), 0) == -1 and "n %d <= 0" % n in err()
    for f in tc.METER_FIELDS:
        x = bufs()
        getattr(x, f)[2] = None
        assert call(8, x, 0) == -1 and "meter 2" in err()
    for frame in (-1, 5, 6):
        assert call(8, bufs(), frame) == -1 and "outside [0, 5)" in err()
    assert call(8, bufs(joint_rot=None), 0) == -1 and "6 of 7" in err()
    assert call(8, bufs(dof_state=None), 0) == -1 and "6 of 7" in err()
    bad = _lib.TennisEvalCfg(episode_length=600, num_frames=5)
    bad.body_of_smpl[:] = [0, 1, 1] + list(range(3, 24))
    assert call(8, bufs(), 0, bad) == -1 and "permutation" in err()
    assert L.v2p_tennis_eval_step(C.byref(c), None, 8, C.byref(b), C.byref(bufs()), 0, None, None) == -1 and "null eval" in err()
    b2 = _lib.TennisBuffers(**{k: one for k in _lib.TENNIS_BUFFER_NAMES if k != "swing_type_cycle"})
    assert L.v2p_tennis_eval_step(C.byref(c), C.byref(ec), 8, C.byref(b2), C.byref(bufs()), 0, None, None) == -1
    assert "v2p_tennis_eval_step" in err()
