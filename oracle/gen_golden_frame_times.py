#!/usr/bin/env python
"""Generate tests/golden/frame_times.npz by RUNNING THE REFERENCE'S OWN PYTHON (test infrastructure only).

Every fixture so far queries the sampler and steps the task at random clip times.  Evaluation (StateInit.Start, 30 fps clips, a control
step of 1/30 s) sits on a frame boundary at every step.  This records the reference there, in three parts:

  S   MotionLib.get_motion_state and _calc_frame_blend on every frame time of nine clips, in nine float32 forms each
      (oracle/golden_inputs.py::frame_time_queries)
  R   get_motion_state on two-frame clips whose lrs / grs rows are overwritten by key-frame pairs at the branch points of slerp and
      quat_to_exp_map (oracle/golden_inputs.py::rotation_branch_pairs)
  E   two epochs of the gym-less HumanoidSMPLIM in StateInit.Start, physics teacher-forced, stepped until every reset flag is up

The file has to stay under 1 MiB, so outputs that are copies of other outputs or of table rows are CHECKED here and not stored:
velocities are the table rows of frame_idx0 (stored: frame_idx0), root_pos / root_rot / key_pos are rows of rb_pos / rb_rot, the outputs
without adjust_height differ from those with it in the z of the positions only, the task's observation is the forced state.  The
helper tests/frame_times_fixture.py puts them together again.  Rigid-body rows and dof_pos are stored for a subset of the queries.

Runs only where the reference is installed.    Usage:  PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_frame_times.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import gen_golden as GG  # noqa: E402  (installs the shim, imports the reference)
import torch  # noqa: E402

from oracle import golden_inputs as GI  # noqa: E402
from vid2player3d_amd.model import load_baked_model  # noqa: E402

him, BaseTask, npf = GG.him, GG.BaseTask, GG.npf
T = torch.from_numpy
NAMES = ("root_pos", "root_rot", "dof_pos", "root_vel", "root_ang_vel", "dof_vel", "key_pos", "rb_pos", "rb_rot")
TABLE_KEYS = ("gts", "grs", "lrs", "grvs", "gravs", "dvs")
CLIP_KEYS = ("motion_lengths", "motion_num_frames", "motion_dt", "motion_fps", "motion_weights", "motion_bodies", "motion_min_verts_h")
KEY = list(GG.KEY_BODY_IDS)


def tables_of(mlib):
    tabs = {k: npf(getattr(mlib, k)).copy() for k in TABLE_KEYS}
    tabs.update({k: npf(getattr(mlib, "_" + k)).copy() for k in CLIP_KEYS})
    tabs["length_starts"] = npf(mlib.length_starts).copy()
    return tabs


def same(a, b):
    """bit for bit (NaN == NaN, -0.0 != 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def query(mlib, tabs, ids, times, what):
    """The reference on (ids, times): frame indices, blend, the nine outputs with adjust_height, rb_pos z without; the redundancies checked."""
    ti, tt = torch.tensor(ids, dtype=torch.long), torch.tensor(times, dtype=torch.float32)
    f0, f1, blend = mlib._calc_frame_blend(tt, mlib._motion_lengths[ti], mlib._motion_num_frames[ti], mlib._motion_dt[ti])
    adj = dict(zip(NAMES, [npf(r) for r in mlib.get_motion_state(ti, tt, return_rigid_body=True, adjust_height=True, ground_tolerance=0.0)]))
    raw = dict(zip(NAMES, [npf(r) for r in mlib.get_motion_state(ti, tt, return_rigid_body=True, adjust_height=False)]))
    f0l = npf(f0) + tabs["length_starts"][ids]
    for o in (adj, raw):
        assert same(o["root_vel"], tabs["grvs"][f0l]) and same(o["root_ang_vel"], tabs["gravs"][f0l]) and same(o["dof_vel"], tabs["dvs"][f0l]), what
        assert same(o["root_pos"], o["rb_pos"][:, 0]) and same(o["root_rot"], o["rb_rot"][:, 0]) and same(o["key_pos"], o["rb_pos"][:, KEY]), what
    for k in ("root_rot", "dof_pos", "rb_rot"):
        assert same(adj[k], raw[k]), (what, k)
    assert same(adj["rb_pos"][..., :2], raw["rb_pos"][..., :2]), what
    return npf(f0), npf(f1), npf(blend), adj, raw["rb_pos"][..., 2].copy()


def gen_sampler(mlib, tabs, out):
    ids, times, ks, forms = GI.frame_time_queries(tabs["motion_dt"], tabs["motion_lengths"], tabs["motion_num_frames"])
    f0, f1, blend, adj, raw_z = query(mlib, tabs, ids, times, "S")
    nf = tabs["motion_num_frames"][ids]
    exact = (forms & 0b001001001) != 0
    full = (ks < 0) | (exact & ((ks % 3 == 0) | (ks >= nf - 1) | (nf <= 3)))
    rows = np.nonzero(full)[0]
    out.update(s_ids=ids.astype(np.int16), s_times=times, s_k=ks.astype(np.int16), s_forms=forms.astype(np.uint16), s_f0=f0.astype(np.int16),
               s_f1=f1.astype(np.int16), s_blend=blend, s_root_pos=adj["root_pos"], s_root_rot=adj["root_rot"], s_root_z_noadj=raw_z[:, 0],
               s_rows=rows.astype(np.int32), s_dof_pos=adj["dof_pos"][rows], s_rb_pos=adj["rb_pos"][rows], s_rb_rot=adj["rb_rot"][rows],
               s_rb_z_noadj=raw_z[rows])
    print("S: %d queries (%d with all outputs), NaN in the outputs: %d" % (len(ids), len(rows), sum(int(np.isnan(v).sum()) for v in adj.values())))


def gen_rotations(body_model, out):
    clips = [GI.synth.make_clip(np.random.default_rng(9200 + c), 2) for c in range(GI.FT_ROT_CLIPS)]
    mlib = GG.build_reference_motion_lib(clips)
    q0, q1, labels = GI.rotation_branch_pairs()
    lp, gp = GI.rotation_branch_slots(len(labels))
    for c in range(GI.FT_ROT_CLIPS):   # data, not code: the key frames of the reference's own tables
        s = int(mlib.length_starts[c])
        mlib.lrs[s], mlib.lrs[s + 1] = T(q0[lp[c]]), T(q1[lp[c]])
        mlib.grs[s], mlib.grs[s + 1] = T(q0[gp[c]]), T(q1[gp[c]])
    tabs = tables_of(mlib)
    ids = np.repeat(np.arange(GI.FT_ROT_CLIPS), len(GI.FT_BLENDS)).astype(np.int64)
    times = (np.tile(np.array(GI.FT_BLENDS, np.float32), GI.FT_ROT_CLIPS) * tabs["motion_dt"][ids]).astype(np.float32)
    f0, f1, blend, adj, raw_z = query(mlib, tabs, ids, times, "R")
    out.update({"r_tab_" + k: v for k, v in tabs.items()})
    out.update(r_ids=ids.astype(np.int16), r_times=times, r_f0=f0.astype(np.int16), r_f1=f1.astype(np.int16), r_blend=blend, r_dof_pos=adj["dof_pos"],
               r_rb_pos=adj["rb_pos"], r_rb_rot=adj["rb_rot"], r_rb_z_noadj=raw_z, r_labels=np.array(labels))
    print("R: %d pairs, %d queries, NaN in the outputs: %d" % (len(labels), len(ids), sum(int(np.isnan(v).sum()) for v in adj.values())))


def gen_epochs(mlib, tabs, body_model, out):
    torch.manual_seed(7)
    n = len(GI.FT_EPOCH_MOTION_IDS)
    ids = GI.FT_EPOCH_MOTION_IDS
    task = GG.make_gymless_task(mlib, n, ids, body_model)
    task._state_init = him.HumanoidSMPLIM.StateInit.Start
    forced = {}

    def teacher_forced_physics(self):
        s = forced["cur"]
        self._dof_pos[:] = T(s["dof_pos"])
        self._dof_vel[:] = T(s["dof_vel"])
        self._rigid_body_state.view(n, 24, 13)[:] = T(s["rb_state"])
        self._humanoid_root_states[:] = T(s["rb_state"][:, 0, :])

    task._physics_step = types.MethodType(teacher_forced_physics, task)
    nf = tabs["motion_num_frames"][ids]
    sample_envs = (0, 2, 4, 6)

    def target_rows():
        return np.concatenate([npf(getattr(task, "_target_" + k)).reshape(n, -1) for k in NAMES], axis=1)

    def target_frames(what):
        """frame_idx0 / blend of the target query (cur_time + dt), and the check that the target's velocities are that frame's rows"""
        t = task._cur_ref_motion_times + task.dt
        ti = torch.tensor(ids, dtype=torch.long)
        f0, _, blend = mlib._calc_frame_blend(t, mlib._motion_lengths[ti], mlib._motion_num_frames[ti], mlib._motion_dt[ti])
        f0l = npf(f0) + tabs["length_starts"][ids]
        assert same(npf(task._target_dof_vel), tabs["dvs"][f0l]) and same(npf(task._target_root_vel), tabs["grvs"][f0l]), what
        assert same(npf(task._target_root_ang_vel), tabs["gravs"][f0l]), what
        return npf(f0).astype(np.int16), npf(blend)

    def record_reset(tag, envs):
        e = list(envs)
        out[tag + "cur_time"] = npf(task._cur_ref_motion_times).copy()
        out[tag + "root_states"] = npf(task._humanoid_root_states)[e].copy()
        out[tag + "dof_pos"] = npf(task._dof_pos)[e].copy()
        out[tag + "dof_vel"] = npf(task._dof_vel)[e].copy()
        out[tag + "rb_state"] = npf(task._rigid_body_state.view(n, 24, 13))[e].copy()
        out[tag + "obs"] = npf(task.obs_buf)[e].copy()
        out[tag + "target"] = target_rows()[e]
        out[tag + "flags"] = np.stack([npf(task.reset_buf), npf(task._terminate_buf), npf(task.progress_buf)]).astype(np.int16)

    def run_epoch(tag, partial):
        task.reset()
        assert not npf(task._reset_ref_motion_times).any()
        record_reset(tag + "reset_", range(n))
        feat = npf(task.context_feat)
        assert same(feat[..., 0:72], feat[..., 237:309]) and same(feat[..., 168:237], feat[..., 309:378])   # body_pos_gt, dof_pos_gt
        out[tag + "context_feat"] = feat[[0, 4], :, :237].copy()   # envs 0 and 4 (17 and 45 frames): body_pos, body_rot, dof_pos
        out[tag + "context_mask"] = npf(task.context_mask).astype(np.uint8)
        per = {k: [] for k in ("rew", "sub_rewards", "reset", "terminate", "progress", "cur_time", "target_f0", "target_blend", "actions_masked_rows")}
        trow, tstep, tenv = [], [], []
        start = np.zeros(n, np.float32)   # the time that the forced state follows: clip time 0 at this step
        left, i = None, 0
        while i < GI.FT_MAX_STEPS and (left is None or left > 0):
            if partial and i == GI.FT_PARTIAL_AT:
                pe = torch.tensor(GI.FT_PARTIAL_ENVS, dtype=torch.long)
                try:
                    task.reset(pe)
                    skipped = 0
                except RuntimeError as err:   # _init_context views its rows as [num_envs, ...]: it cannot take a subset of the envs
                    print("E: the reference's _init_context refuses a partial reset (%s): recorded without it" % str(err).splitlines()[0][:80])
                    keep, task._init_context = task._init_context, lambda motion_ids, motion_times: None
                    task.reset(pe)
                    task._init_context = keep
                    skipped = 1
                out[tag + "partial_context_skipped"] = np.int64(skipped)
                record_reset(tag + "partial_", GI.FT_PARTIAL_ENVS)
                start[GI.FT_PARTIAL_ENVS] = -np.float32(i) * np.float32(GI.DT)
            s = GI.env_trace_step_inputs(tabs, ids, start, i, seed=GI.FT_EPOCH_SEED)
            forced["cur"] = s
            a = T(s["actions"].copy())
            BaseTask.step(task, a)
            want_obs = np.concatenate([s["rb_state"][..., 0:3].reshape(n, -1), s["rb_state"][..., 3:7].reshape(n, -1), s["dof_pos"], s["dof_vel"],
                                       s["rb_state"][..., 7:10].reshape(n, -1), s["rb_state"][..., 10:13].reshape(n, -1), tabs["motion_bodies"][ids]], axis=1)
            assert same(npf(task.obs_buf), want_obs.astype(np.float32)), "obs is not the forced state"
            per["rew"].append(npf(task.rew_buf).copy())
            per["sub_rewards"].append(npf(task._sub_rewards).copy())
            per["reset"].append(npf(task.reset_buf).astype(np.uint8))
            per["terminate"].append(npf(task._terminate_buf).astype(np.uint8))
            per["progress"].append(npf(task.progress_buf).astype(np.int16))
            per["cur_time"].append(npf(task._cur_ref_motion_times).copy())
            f0, blend = target_frames("%sstep %d" % (tag, i))
            per["target_f0"].append(f0)
            per["target_blend"].append(blend)
            per["actions_masked_rows"].append((npf(a) == 0).all(axis=1).astype(np.uint8))
            prog = npf(task.progress_buf)
            rows = target_rows()
            for e in sample_envs:   # whole target rows at the first steps and around the clip's end
                if prog[e] <= 2 or nf[e] - 3 <= prog[e] <= nf[e] + 1:
                    trow.append(rows[e])
                    tstep.append(i)
                    tenv.append(e)
            if left is None and npf(task.reset_buf).all():
                left = 4
            if left is not None:
                left -= 1
            i += 1
        for k, v in per.items():
            out[tag + k] = np.stack(v)
        out[tag + "steps"] = np.int64(i)
        out[tag + "target_rows"], out[tag + "target_step"], out[tag + "target_env"] = np.stack(trow), np.array(tstep, np.int16), np.array(tenv, np.int16)
        rise = np.argmax(out[tag + "reset"], axis=0) + 1
        print("E %s: %d steps; control steps until the reset flag is up, per env: %s (frames %s); terminated %s"
              % (tag, i, rise.tolist(), nf.tolist(), out[tag + "terminate"][-1].tolist()))

    run_epoch("a_", False)
    run_epoch("b_", True)


def main():
    body_model = load_baked_model()
    mlib = GG.build_reference_motion_lib(GI.frame_time_clips())
    tabs = tables_of(mlib)
    assert [int(x) for x in tabs["motion_num_frames"]] == [c[0] for c in GI.FT_CLIPS] and np.allclose(tabs["motion_fps"], [c[1] for c in GI.FT_CLIPS])
    out = {"tab_" + k: v for k, v in tabs.items()}
    gen_sampler(mlib, tabs, out)
    gen_rotations(body_model, out)
    gen_epochs(mlib, tabs, body_model, out)
    path = os.path.join(GG.OUT, "frame_times.npz")
    np.savez_compressed(path, **out)
    print("%-24s %8.1f KB" % ("frame_times.npz", os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
