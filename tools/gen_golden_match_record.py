"""Golden data of the match record, recorded from the reference itself: tests/golden/match_record.npz.

`MVAEControllerVisDual` (vid2player/env/tasks/mvae_controller_vis_dual.py, what `run.py --test` runs for a match config) is imported on
the CPU with the shim and the inert stand-ins of tools/gen_golden_tennis_controller.py; the viewer modules it cannot have here are sunk
as tools/gen_golden_tennis_eval.py sinks them.  An object made with `__new__` gets cfg env.record true, `num_rec_frames` beyond the
script's end, `num_eg` = 3 and the arrays of `__init__` set by hand with L = 8 for N = 12 envs, and the reference's OWN `render_vis` runs
on it: once with init=True, then once per scripted step, after `_joint_rot`, `_root_pos`, `_ball_pos`, `_phase_pred`,
`_swing_type_cycle`, `_tar_action`, `progress_buf`, `reset_buf` and `_distance` have been set to the step's values.  After every call
the six `*_all` arrays and the best lists are recorded; pair and frame count of an insertion are read from the line `render_vis` prints.

`_joint_rot` is scripted as what `_update_state_from_sim` would hold for the scripted root quaternion and DoF positions (the pose row's
statement, vid2player3d_amd.tasks.tennis_controller.pose_row_reference), and those are stored too, so that the kernels can be run on the
same state.  Everything else `render_vis` does is a copy, an integer or one float32 add: the arrays are compared exactly.

The script (EVENTS below: call -> {pair: its two `_distance` words}) holds every case of tests/match_record_fixture.CASES, which the
generator asserts from the reference's results.  `progress >= L` is not in it: the reference raises there.  Only arrays are stored.
Run where the reference exists:
    python tools/gen_golden_match_record.py
"""
import contextlib
import io
import os
import re
import sys
import types

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import gen_golden_tennis_controller as base  # noqa: E402,F401  (installs the shim and the stand-ins)
from gen_golden_tennis_controller import _Sink, torch  # noqa: E402

for absent in ("smpl_visualizer.vis_scenepic", "smpl_visualizer.vis"):
    try:
        __import__(absent)
    except Exception:
        sys.modules[absent] = _Sink(absent)

import env.tasks.mvae_controller_vis_dual as ref_vis  # noqa: E402

from tests import match_record_fixture as F  # noqa: E402
from vid2player3d_amd.tasks.tennis_controller import pose_row_reference  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "match_record.npz")
N, L, K, T = 12, 8, 3, 9
# call -> {pair: (distance of env 2k, of env 2k+1)}; both flags of the pair are up in that call and the pair starts again at the next
EVENTS = {
    2: {1: (2.0, 3.0)},                      # the first insertion: [5 (1)]
    3: {2: (1.0, 2.0)},                      # 3 < 5 with one entry of three: dropped
    4: {3: (1.5, 3.5)},                      # 5 == 5: dropped
    5: {0: (4.0, 5.0)},                      # in front: [9 (0), 5 (1)]
    6: {4: (3.0, 4.0), 5: (4.5, 4.5)},       # 7 and 9: only pair 5 is seen, behind the equal entry: [9 (0), 9 (5), 5 (1)]
    7: {2: (3.0, 5.0), 3: (6.0, 2.0)},       # 8 and 8: pair 2; [9, 9, 8 (2)], the 5 leaves
    8: {0: (5.0, 5.0)},                      # pair 0 again: [10 (0), 9 (0), 9 (5)]
    9: {0: (4.75, 4.75), 1: (0.5, 0.5)},     # pair 0 one step after its reset: nframes 1; [10 (0), 9.5 (0), 9 (0)]
}
FRAME_ATTR = dict(joint_rot="joint_rot_all", root_pos="root_pos_all", ball_pos="ball_pos_all", phase="phase_all", swing_type="swing_type_all", tar_action="tar_action_all")
BEST_ATTR = dict(joint_rot="joint_rot_best_all", root_pos="root_pos_best_all", ball_pos="ball_pos_best_all", phase="phase_best_all", swing_type="swing_type_best_all",
                 tar_action="tar_action_best_all")
SHAPES = dict(joint_rot=(24, 3), root_pos=(3,), ball_pos=(3,), phase=(), swing_type=(), tar_action=())
PRINTED = re.compile(r"Update max episode length (\d+), distance \S+ from tensor\(\[\s*(\d+),\s*(\d+)\]\)")


def make_script(rng):
    s = {}
    quat = rng.normal(0, 1, (T + 1, N, 4)).astype(np.float32)
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    quat[0, 1] = np.float32([0.0, 0.0, 0.0, 1.0])  # the identity as a root rotation ...
    quat[1, 2, 3] = -abs(quat[1, 2, 3])            # ... and one with w < 0
    s["root_quat"] = quat
    s["root_pos"] = np.stack([rng.uniform(-3, 3, (T + 1, N)), rng.uniform(-14, -10, (T + 1, N)), rng.uniform(0.8, 1.0, (T + 1, N))], -1).astype(np.float32)
    s["dof_pos"] = (rng.integers(-64, 65, (T + 1, N, 69)) / 64.0).astype(np.float32)
    s["ball_pos"] = rng.uniform(-12, 12, (T + 1, N, 3)).astype(np.float32)
    s["phase"] = rng.uniform(0.0, 6.28, (T + 1, N)).astype(np.float32)
    s["swing_type"] = rng.integers(-1, 4, (T + 1, N)).astype(np.int64)
    s["tar_action"] = rng.integers(0, 2, (T + 1, N)).astype(np.int64)
    progress, reset = np.zeros((T + 1, N), np.int64), np.zeros((T + 1, N), np.int64)
    distance = np.zeros((T + 1, N), np.float32)
    for c in range(1, T + 1):
        progress[c] = np.where(reset[c - 1] != 0, 0, progress[c - 1]) + 1
        distance[c] = rng.uniform(20, 40, N).astype(np.float32)  # of pairs that go on: larger than any finished pair's, and never looked at
        for pair, (a, b) in EVENTS.get(c, {}).items():
            reset[c, 2 * pair:2 * pair + 2] = 1
            distance[c, 2 * pair:2 * pair + 2] = (a, b)
    assert progress.max() < L
    s["progress"], s["reset"], s["distance"] = progress, reset, distance
    return s


def main():
    rng = np.random.default_rng(20261021)
    body_of_smpl = np.concatenate([[0], 1 + rng.permutation(23)]).astype(np.int32)
    s = make_script(rng)

    obj = ref_vis.MVAEControllerVisDual.__new__(ref_vis.MVAEControllerVisDual)
    obj.cfg = {"env": {"record": True, "num_rec_frames": 10 ** 9, "num_eg": K}}
    obj.headless, obj.frame_index, obj.num_envs = True, 0, N
    obj.num_best = obj.cfg["env"].get("num_eg", 1)
    obj.joint_rot_all = torch.zeros((N, L, 24, 3), dtype=torch.float32)
    obj.root_pos_all = torch.zeros((N, L, 3), dtype=torch.float32)
    obj.ball_pos_all = torch.zeros((N, L, 3), dtype=torch.float32)
    obj.target_pos_all = torch.zeros((N, L, 3), dtype=torch.float32)
    obj.phase_all = torch.zeros((N, L), dtype=torch.float32)
    obj.swing_type_all = torch.zeros((N, L), dtype=torch.int64)
    obj.tar_action_all = torch.zeros((N, L), dtype=torch.int64)
    for k in ("distance_best_all",) + tuple(BEST_ATTR.values()):
        setattr(obj, k, [])
    obj._mvae_player = types.SimpleNamespace()

    out = {"N": np.int64(N), "L": np.int64(L), "K": np.int64(K), "T": np.int64(T), "body_of_smpl": body_of_smpl}
    out.update({"in/" + k: v for k, v in s.items()})
    rec = {"all/" + k: np.zeros((T + 1, N, L) + SHAPES[k], np.int64 if k in ("swing_type", "tar_action") else np.float32) for k in FRAME_ATTR}
    rec.update({"best/" + k: np.zeros((T + 1, K, 2, L) + SHAPES[k], np.int64 if k in ("swing_type", "tar_action") else np.float32) for k in BEST_ATTR})
    rec.update({"best/count": np.zeros(T + 1, np.int64), "best/distance": np.zeros((T + 1, K), np.float32), "best/nframes": np.zeros((T + 1, K), np.int64),
                "best/pair": np.full((T + 1, K), -1, np.int64), "inserted": np.zeros(T + 1, bool)})
    pairs = []  # the pair of every entry of the reference's lists, kept in step with them
    for c in range(T + 1):
        rb = F.rigid_bodies(s["root_pos"][c], s["root_quat"][c])
        obj._joint_rot = torch.from_numpy(pose_row_reference(body_of_smpl, rb, s["dof_pos"][c]))
        obj._root_pos, obj._ball_pos = torch.from_numpy(s["root_pos"][c].copy()), torch.from_numpy(s["ball_pos"][c].copy())
        obj._mvae_player._phase_pred, obj._mvae_player._swing_type_cycle = torch.from_numpy(s["phase"][c].copy()), torch.from_numpy(s["swing_type"][c].copy())
        obj._tar_action, obj.progress_buf = torch.from_numpy(s["tar_action"][c].copy()), torch.from_numpy(s["progress"][c].copy())
        obj.reset_buf, obj._distance = torch.from_numpy(s["reset"][c].copy()), torch.from_numpy(s["distance"][c].copy())
        before = [float(x) for x in obj.distance_best_all]
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            obj.render_vis(init=(c == 0))
        m = PRINTED.search(said.getvalue())
        if m:
            nframes, even, odd = (int(x) for x in m.groups())
            assert even % 2 == 0 and odd == even + 1
            # where the reference's list changed first: an insertion goes behind its equals, so that is the new entry's rank
            pos = next(i for i, x in enumerate(obj.distance_best_all) if i >= len(before) or float(x) != before[i])
            assert obj.phase_best_all[pos].shape[1] == nframes
            pairs.insert(pos, even // 2)
            del pairs[K:]
            rec["inserted"][c] = True
        assert len(pairs) == len(obj.distance_best_all) <= K
        for k, attr in FRAME_ATTR.items():
            rec["all/" + k][c] = getattr(obj, attr).numpy()
        rec["best/count"][c] = len(obj.distance_best_all)
        for r, dist in enumerate(obj.distance_best_all):
            nf = obj.phase_best_all[r].shape[1]
            rec["best/distance"][c, r], rec["best/nframes"][c, r], rec["best/pair"][c, r] = np.float32(dist), nf, pairs[r]
            for k, attr in BEST_ATTR.items():
                rec["best/" + k][c, r, :, :nf] = getattr(obj, attr)[r].numpy()
    assert not obj.target_pos_all.any()  # (allocated, never written by the dual class)
    out.update(rec)
    found = F.census(out)
    missing = [k for k in F.CASES if not found[k]]
    assert not missing, "the script lacks: %s" % ", ".join(missing)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes); census: %s" % (OUT, os.path.getsize(OUT), ", ".join("%s @ %s" % (k, found[k]) for k in F.CASES)))


if __name__ == "__main__":
    main()
