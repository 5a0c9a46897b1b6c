"""The census of tests/tennis_edges.py: the four numpy statements run on the edge inputs, and every path the batteries were built for is
taken by at least one row - decided from the statements and the inputs, without a kernel.  tests/test_gpu_controller_guards.py runs the
same inputs on the device.  `pytest -s` prints the table (docs/NOTES.md holds it)."""
import numpy as np

from tests import tennis_edges as E
from vid2player3d_amd.tasks import tennis_controller as tc
from vid2player3d_amd.tasks import tennis_controller_dual as td

TABLE = []


def row(battery, path, count):
    TABLE.append((battery, path, count))
    print("%-28s %-58s %s" % (battery, path, count))
    assert count, "%s: no row takes the path '%s'" % (battery, path)


def test_history_rolls_over_more_than_one_pass():
    for L in E.HISTORY_LENGTHS:
        st, s = E.history(L)
        want = tc.task_step_reference(st, s)
        assert st["use_history"] and E.distinct(s["ball_obs"]) and np.array_equal(want["ball_obs"][:, :-1], s["ball_obs"][:, 1:])
        assert np.array_equal(want["ball_obs"][:, -1], s["ball_state"][:, 0:3]) and np.array_equal(tc.observation_reference(st, s, [1, 4])[1], want["ball_obs"][[1, 4]])
        row("history L=%d" % L, "step / obs: passes of %d lanes" % E.STEP_LANES, E.passes(L, E.STEP_LANES))
        for kind, ref in (("step", td.dual_step_reference), ("hand", td.handover_reference)):
            st, s = E.dual_history(kind, L)
            want = ref(st, s)
            assert st["use_history"] and E.distinct(s["ball_obs"]) and want["ball_obs"].shape == (8, L, 3)
            if kind == "step":
                assert np.array_equal(want["ball_obs"][:, :-1], s["ball_obs"][:, 1:])
                row("history L=%d" % L, "dual step: passes of %d lanes" % E.STEP_LANES, E.passes(L, E.STEP_LANES))
            else:
                ids = np.nonzero(s["reset_reaction"])[0]
                others = np.setdiff1d(np.arange(8), ids)
                assert np.array_equal(want["ball_obs"][others], s["ball_obs"][others])
                assert all((want["ball_obs"][e] == want["ball_state"][e, 0:3]).all() for e in ids), "a reacting env's history is its new ball position, L times"
                row("history L=%d" % L, "hand-over: reacting envs (fill, then roll)", len(ids))
                row("history L=%d" % L, "hand-over: pairs in which both react", int(s["reset_reaction"].reshape(-1, 2).all(1).sum()))
                row("history L=%d" % L, "hand-over: passes of %d lanes" % E.HAND_LANES, E.passes(L, E.HAND_LANES))
    assert E.passes(10, E.STEP_LANES) == 1 == E.passes(10, E.HAND_LANES), "the fixtures' length is one pass in both kernels"
    assert E.passes(22, E.STEP_LANES) == 2 and E.passes(11, E.HAND_LANES) == 2 and E.passes(100, E.STEP_LANES) == 5


def test_cursors_at_and_past_the_windows_end():
    assert E.cursors_after(10).tolist() == [1, 91, 92, 100, 100, 100, 1, 100]
    for L in E.CURSOR_LENGTHS:
        st, s = E.cursor_rows(L)
        want = tc.task_step_reference(st, s)
        assert not st["use_history"] and np.array_equal(want["traj_cursor"], E.cursors_after(L))
        rows, zeros = E.window_off_the_end(st, s, want["obs"])
        assert zeros and np.array_equal(tc.observation_reference(st, s)[0], want["obs"], equal_nan=True)
        for c in E.cursors(L):
            row("cursors L=%d" % L, "step / obs: traj_cursor %d" % c, int((s["traj_cursor"] == c).sum()))
        row("cursors L=%d" % L, "step / obs: windows past frame 99 (zeros - racket_pos)", len(rows))
        row("cursors L=%d" % L, "step / obs: windows wholly inside the row", 8 - len(rows))
        st, s = E.dual_cursors("step", L)
        want = td.dual_step_reference(st, s)
        assert np.array_equal(want["traj_cursor"][:16], np.tile(E.cursors_after(L), 2))
        rows, zeros = E.window_off_the_end(st, s, want["obs"])
        assert zeros
        row("cursors L=%d" % L, "dual step: windows past frame 99", len(rows))
        st, s = E.dual_cursors("hand", L)
        want = td.handover_reference(st, s)
        ids = np.nonzero(s["reset_reaction"])[0]
        F = s["traj_in"].shape[1]
        assert sorted(s["traj_cursor"][ids].tolist()) == sorted(E.cursors(L).tolist() + list(E.HAND_CURSORS)) and not want["traj_cursor"][ids].any()
        cur = np.clip(s["traj_cursor"].astype(np.int64), 0, 100)
        shifted = [e for e in ids if 0 < cur[e] and cur[e] + F < 100]
        emptied = [e for e in ids if cur[e] + F >= 100]
        for e in shifted:
            assert np.array_equal(want["ball_traj"][e, F:100 - cur[e]], s["ball_traj"][e, cur[e] + F:]) and not want["ball_traj"][e, 100 - cur[e]:].any()
        for e in emptied:
            assert not want["ball_traj"][e, F:].any()
        row("cursors L=%d" % L, "hand-over: reacting envs, one per cursor of the lists", len(ids))
        row("cursors L=%d" % L, "hand-over: old window shifted from a cursor > 0", len(shifted))
        row("cursors L=%d" % L, "hand-over: old window wholly past frame 99", len(emptied))


def test_wrist_links():
    st, s = E.wrists()
    want = tc.task_step_reference(st, s)
    base = tc.task_step_reference(st, dict(s, wrist_link=np.full(len(E.WRISTS), 22, np.int64)))
    for k, link in enumerate(E.WRISTS):
        differs = np.abs(want["racket_normal"][k] - base["racket_normal"][k]).max() > 1e-3
        assert differs == (link != 22), "link %d: the racket normal must be another link's than 22's" % link
        row("wrists", "wrist_link %d" % link, int((s["wrist_link"] == link).sum()))
    st, s = E.wrists(E.WRISTS_CLAMPED[0])
    row("wrists", "wrist_link below 0 / above 23 (clamped)", len(s["wrist_link"]))
    for kind in ("step", "hand"):
        st, s = E.dual_wrists(kind)
        row("wrists", "dual %s: links other than 22" % kind, int((s["wrist_link"] != 22).sum()))
        if kind == "hand":
            row("wrists", "dual hand: reacting envs with a link other than 22", int((s["reset_reaction"] & (s["wrist_link"] != 22)).sum()))


def test_out_estimator_rows_reach_every_reachable_clamp():
    st, s = E.estimator()
    want = tc.task_step_reference(st, s)
    census, valid = E.estimator_census(st, s, want)
    for path, count in census.items():
        if path in E.ESTIMATOR_UNREACHABLE:
            TABLE.append(("estimator", path + " (unreachable)", count))
            print("%-28s %-58s %s" % ("estimator", path + " (unreachable)", count))
            assert count == 0
        else:
            row("estimator", path, count)
    names = [r[0] for r in E.ESTIMATOR_ROWS]
    assert [n for n, v in zip(names, valid) if not v] == [n for n in names if n.startswith("invalid alone")]


def test_dual_reset_law_over_all_sixteen_combinations():
    st, s = E.dual_flags()
    want = td.dual_step_reference(st, s)
    seen = E.dual_flags_census(st, s, want)
    name = lambda b: "%s%s" % ("R" if b & 1 else "-", "T" if b & 2 else "-")
    for a in range(4):
        for b in range(4):
            pairs = seen.get((a, b), [])
            row("dual flags", "even env %s, odd env %s (R recovery, T terminate)" % (name(a), name(b)), len(pairs))
    row("dual flags", "pairs in waves 0-1 of a workgroup", sum(1 for ps in seen.values() for p in ps if p % 2 == 0))
    row("dual flags", "pairs in waves 2-3 of a workgroup", sum(1 for ps in seen.values() for p in ps if p % 2 == 1))
    row("dual flags", "pairs that end an episode", int(want["reset"].reshape(-1, 2).all(1).sum()))
    row("dual flags", "envs with reset_reaction", int(want["reset_reaction"].sum()))
    row("dual flags", "envs with reset_recovery", int(want["reset_recovery"].sum()))
