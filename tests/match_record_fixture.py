"""Readers of tests/golden/match_record.npz (tools/gen_golden_match_record.py) shared by the CPU and the GPU tests of the match record
and by the generator itself: the inputs of call c (0: the init frame, 1..T: the steps) as the statement takes them, what the reference's
own `MVAEControllerVisDual.render_vis` left after each call, and the census of cases the script must contain."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_record.npz")
FRAME_NAMES = ("joint_rot", "root_pos", "ball_pos", "phase", "swing_type", "tar_action")
CASES = ("no_finished", "first_insertion", "front_better", "dropped_not_full", "dropped_equal", "middle_behind_equal", "two_finish_different", "two_finish_equal",
         "eviction", "kept_twice", "nframes_one")


def load(path=GOLDEN):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def sizes(fx):
    return int(fx["N"]), int(fx["L"]), int(fx["K"]), int(fx["T"])


def rigid_bodies(root_pos, root_quat):
    """rb_state [N,24,13] with the root link's position and (x, y, z, w) set and every other link at the origin, unrotated."""
    n = len(root_pos)
    rb = np.zeros((n, 24, 13), np.float32)
    rb[:, :, 6] = 1
    rb[:, 0, 0:3], rb[:, 0, 3:7] = root_pos, root_quat
    return rb


def inputs(fx, c):
    """The arrays `match_record_reference` reads at call c."""
    n = sizes(fx)[0]
    ball = np.zeros((n, 13), np.float32)
    ball[:, 6] = 1
    ball[:, 0:3] = fx["in/ball_pos"][c]
    return dict(rb_state=rigid_bodies(fx["in/root_pos"][c], fx["in/root_quat"][c]), dof_pos=fx["in/dof_pos"][c].copy(), ball_state=ball, phase_pred=fx["in/phase"][c].copy(),
                swing_type_cycle=fx["in/swing_type"][c].copy(), tar_action=fx["in/tar_action"][c].copy(), progress=fx["in/progress"][c].copy(), reset=fx["in/reset"][c].copy(),
                distance=fx["in/distance"][c].copy())


def reference_best(fx, c):
    """The reference's lists after call c, best first: [(distance float32, pair, nframes, {name: [2,nframes,...]})]."""
    out = []
    for r in range(int(fx["best/count"][c])):
        nf = int(fx["best/nframes"][c, r])
        out.append((fx["best/distance"][c, r], int(fx["best/pair"][c, r]), nf, {k: fx["best/" + k][c, r, :, :nf] for k in FRAME_NAMES}))
    return out


def compare_with_reference(fx, rec, c, what):
    """The record `rec` after call c against the reference's arrays and lists: everything is a copy, an integer or one float32 add."""
    for k in FRAME_NAMES:
        assert rec[k + "_all"].dtype == fx["all/" + k].dtype and np.array_equal(rec[k + "_all"], fx["all/" + k][c], equal_nan=True), (what, k)
    from vid2player3d_amd import match

    got, want = match.best_of(rec), reference_best(fx, c)
    assert len(got) == len(want), what
    for g, (dist, pair, nframes, frames) in zip(got, want):
        assert np.float32(g["distance"]) == dist and g["pair"] == pair and g["nframes"] == nframes, what
        for k in FRAME_NAMES:
            assert g[k].shape == frames[k].shape and np.array_equal(g[k], frames[k]), (what, k)
    assert not rec["overflow"].any(), what


def census(fx):
    """{case: [calls]} over the stored arrays; every case of CASES must have a call."""
    n, L, K, T = sizes(fx)
    found = {k: [] for k in CASES}
    for c in range(1, T + 1):
        done = (fx["in/reset"][c].reshape(-1, 2) != 0).any(1)
        d = fx["in/distance"][c][0::2] + fx["in/distance"][c][1::2]
        before, after = reference_best(fx, c - 1), reference_best(fx, c)
        inserted = bool(fx["inserted"][c])
        if not done.any():
            found["no_finished"].append(c)
            assert not inserted
            continue
        top = d[done].max()
        reach = np.flatnonzero(done & (d == top))
        if not inserted:
            assert before and [(x[0], x[1], x[2]) for x in before] == [(x[0], x[1], x[2]) for x in after]
            if top == before[-1][0]:
                found["dropped_equal"].append(c)
            elif top < before[-1][0] and len(before) < K:
                found["dropped_not_full"].append(c)
            continue
        pos = next((i for i, x in enumerate(before) if top > x[0]), len(before))
        keys = [(x[0], x[1], x[2]) for x in before]
        pair, nframes = after[pos][1], after[pos][2]
        assert [(x[0], x[1], x[2]) for x in after] == (keys[:pos] + [(top, pair, nframes)] + keys[pos:])[:K]
        assert pair == reach[0] and nframes == fx["in/progress"][c][2 * pair]
        if not before:
            found["first_insertion"].append(c)
        elif pos == 0:
            found["front_better"].append(c)
        elif before[pos - 1][0] == top and pos < len(after) - 1:
            found["middle_behind_equal"].append(c)
        if len(before) == K:
            found["eviction"].append(c)
        if done.sum() >= 2 and len(reach) == 1 and pair != np.flatnonzero(done)[0]:
            found["two_finish_different"].append(c)
        if len(reach) >= 2:
            found["two_finish_equal"].append(c)
        if nframes == 1:
            found["nframes_one"].append(c)
        twice = [x for x in after if x[1] == pair]
        if len(twice) >= 2 and all(all(np.array_equal(x[3][k][:, 0], fx["all/" + k][0][2 * pair:2 * pair + 2, 0]) for k in FRAME_NAMES) for x in twice):
            found["kept_twice"].append(c)
    return found
