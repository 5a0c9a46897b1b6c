"""The controller's evaluation step on the device: `v2p_tennis_eval_step` against its numpy statement and against what the reference's
own `MVAEControllerVis` recorded (tests/golden/tennis_eval.npz), step by step, every tensor between guard rows; the record's frames; and
`TennisControllerEval` / `ControllerEvalPlayer` on the racket + ball controller, reset by ids against reset by flags."""
import numpy as np
import pytest
import torch

from tests import tennis_eval_fixture as F
from tests import tennis_fixture as TF
from tests.guarded import Guarded
from vid2player3d_amd.tasks import tennis_controller as tc

gpu = pytest.mark.gpu
DEV = F.DEV
DTYPES = {"wrist_link": torch.int64, "swing_type": torch.int64, "swing_type_cycle": torch.int64, "tar_time_total": torch.int64, "tar_action": torch.int64,
          "tar_time": torch.int64, "progress": torch.int64, "traj_cursor": torch.int32, "vel_x_overflow": torch.int64, "meter_count": torch.int64}
BYTES = ("has_bounce", "has_bounce_now", "has_racket_contact", "has_racket_contact_now", "bounce_in", "est_bounce_in")
PER_ENV = ("rb_state", "root_states", "racket_state", "ball_state", "wrist_link", "has_bounce", "has_bounce_now", "bounce_pos", "phase_pred", "swing_type", "swing_type_cycle",
           "tar_time_total", "tar_action", "target_bounce_pos", "ball_traj", "has_racket_contact", "has_racket_contact_now", "tar_time", "progress", "prev_ball_vy",
           "traj_cursor", "ball_obs", "bounce_in", "est_bounce_pos", "est_bounce_time", "est_max_height", "est_bounce_in", "distance", "dof_pos")
FRAMES = 3  # of the record in the kernel tests


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype != want.dtype:  # (flags: bytes on the device, bools in the statement)
        got, want = got.astype(np.int64), want.astype(np.int64)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r != %r" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def first_rows(s, n):
    """the fixture step's arrays for its first n envs (the meters are [4,N]: their columns)"""
    out = {}
    for k, v in s.items():
        if v is None:
            out[k] = None
        elif k in PER_ENV:
            out[k] = np.ascontiguousarray(v[:n])
        elif k in tc.METER_FIELDS:
            out[k] = np.ascontiguousarray(v[:, :n])
        else:
            out[k] = v
    return out


def upload(st, s, record):
    """(guard, step tensors, meter tensors [4,n], record tensors or None, dof_state): the arrays of a step between guard rows, outputs
    poisoned - whatever survives was not written."""
    g = Guarded(DEV)
    n = len(s["rb_state"])
    t = {}
    for k, v in s.items():
        if v is None or k in tc.METER_FIELDS or k == "dof_pos":
            continue
        dt = torch.uint8 if k in BYTES else DTYPES.get(k, torch.float32)
        t[k] = g.of(k, np.ascontiguousarray(v).astype(np.uint8 if k in BYTES else v.dtype), dtype=dt)
    for k, shape in (("racket_pos", (n, 3)), ("racket_normal", (n, 3)), ("obs", (n, tc.obs_width(st))), ("rew", (n,)), ("sub_rewards", (n, tc.num_sub_rewards(st)))):
        t[k] = g.empty(k, shape)
    for k in ("reset", "terminate"):
        t[k] = g.empty(k, (n,), torch.int64)
    for k in ("reset_reaction", "reset_recovery"):
        t[k] = g.empty(k, (n,), torch.uint8)
    # a meter array is [4,n] with its rows handed to the kernel one by one: guard rows around the whole, as [4 n] elements
    meters = {k: g.of(k, np.ascontiguousarray(s[k]).reshape(-1), dtype=DTYPES.get(k, torch.float32)).view(4, n) for k in tc.METER_FIELDS}
    dof = np.zeros((n * 69, 2), np.float32)
    dof[:, 0], dof[:, 1] = s["dof_pos"].reshape(-1), 7.0  # (the velocities: never read)
    dof_state = g.of("dof_state", dof)
    rec = None
    if record:
        rec = dict(joint_rot=g.empty("joint_rot", (FRAMES, n, 24, 3)), root_pos=g.empty("root_pos", (FRAMES, n, 3)), ball_pos=g.empty("ball_pos", (FRAMES, n, 3)),
                   target_pos=g.empty("target_pos", (FRAMES, n, 3)), phase=g.empty("phase", (FRAMES * n,)).view(FRAMES, n),
                   swing_type_cycle=g.empty("rec_swing", (FRAMES * n,), torch.int64).view(FRAMES, n))
    return g, t, meters, rec, dof_state


def download(t, meters, rec):
    out = {k: v.detach().cpu().numpy() for k, v in t.items()}
    out.update({k: v.detach().cpu().numpy() for k, v in meters.items()})
    if rec is not None:
        out["record_all"] = {k: v.detach().cpu().numpy() for k, v in rec.items()}
    return out


def run_step(st, est, s, frame=0, record=True):
    g, t, meters, rec, dof_state = upload(st, s, record)
    names = tc.launch_eval_step(st, est, t, len(s["rb_state"]), meters, rec, dof_state if record else None, frame)
    g.check()
    got = download(t, meters, rec)
    got["names"] = names
    if rec is not None:
        got["record"] = {k: v[frame] for k, v in got["record_all"].items()}
    return got


EXACT = TF.EXACT + tc.METER_FIELDS + ("distance",)


def against_statement(st, est, s, got, frame, what):
    """bit for bit, except the step's exp / sqrt-derived floats: those within the bounds of the step's own test (tests/tennis_fixture.py).
    The record's frame is bit for bit throughout, joint 0 included: kernel and statement round its one arctangent once, from double."""
    want = tc.eval_step_reference(st, est, s)
    assert got["names"] == want.pop("sub_rewards_names")
    for k in EXACT:
        if k in want and k in got:
            assert_bits(got[k].reshape(-1), np.asarray(want[k]).reshape(-1), "%s: %s" % (what, k))
    TF.compare(got, {k: v for k, v in want.items() if k in TF.FLOATS and k in got}, what)
    assert_bits(got["distance"], s["distance"], what + ": distance is not touched")
    rec = tc.eval_record_reference(est, s)
    for k in tc.RECORD_NAMES:
        for f in range(FRAMES):  # frames not yet written hold their pre-fill
            if f != frame:
                rest = got["record_all"][k][f]
                assert np.isnan(rest).all() if rest.dtype.kind == "f" else (rest == 0x5A5A5A5A5A5A5A5A).all(), "%s: record %s, frame %d was written" % (what, k, f)
        assert_bits(got["record"][k], rec[k], "%s: record %s, frame %d" % (what, k, frame))


@gpu
@pytest.mark.parametrize("n", [None, 1, 3, 4, 5])
@pytest.mark.parametrize("name", F.VARIANTS)
def test_eval_step_kernel_matches_its_statement_step_by_step(name, n):
    """at the fixture's N and on its first n rows, n around the 4 envs of a workgroup"""
    st, est = F.settings(name)
    for t in range(F.steps()):
        s = F.step_inputs(name, t)
        s = s if n is None else first_rows(s, n)
        got = run_step(st, est, s, frame=t % FRAMES)
        against_statement(st, est, s, got, t % FRAMES, "%s step %d n %s" % (name, t, n))
        if t in (0, F.steps() - 1):  # two runs give the same bits
            again = run_step(st, est, s, frame=t % FRAMES)
            for k, v in got.items():
                if isinstance(v, np.ndarray):
                    assert_bits(again[k], v, "%s step %d, second run: %s" % (name, t, k))
            for k in tc.RECORD_NAMES:
                assert_bits(again["record_all"][k], got["record_all"][k], "%s step %d, second run: record %s" % (name, t, k))


@gpu
@pytest.mark.parametrize("name", F.VARIANTS)
def test_eval_step_kernel_matches_the_reference_step_by_step(name):
    st, est = F.settings(name)
    for t in range(F.steps()):
        s = F.step_inputs(name, t)
        got = run_step(st, est, s, frame=t % FRAMES)
        F.compare(name, got, F.step_expected(name, t), "%s step %d" % (name, t))
        assert got["names"] == F.golden()[name + "/sub_rewards_names"].tobytes().decode()


@gpu
def test_record_frames_and_the_step_without_a_record():
    st, est = F.settings("V")
    s = F.step_inputs("V", 4)
    plain = run_step(st, est, s, record=False)
    for frame in (0, FRAMES - 1):
        got = run_step(st, est, s, frame=frame)
        against_statement(st, est, s, got, frame, "frame %d" % frame)
        for k, v in plain.items():  # with NULL record pointers the step's own outputs are the same bits
            if isinstance(v, np.ndarray):
                assert_bits(v, got[k], "without a record: %s" % k)
    for frame in (FRAMES, -1):
        g, t, meters, rec, dof_state = upload(st, s, True)
        before = download(t, meters, rec)
        with pytest.raises(RuntimeError, match=r"frame -?\d+ outside \[0, %d\)" % FRAMES):
            tc.launch_eval_step(st, est, t, len(s["rb_state"]), meters, rec, dof_state, frame)
        g.check()
        after = download(t, meters, rec)
        for k, v in before.items():
            if isinstance(v, np.ndarray):
                assert_bits(after[k], v, "a refused frame launched nothing: %s" % k)


# ------------------------------------------------------------------------------------------------------------------ the controller
def B(t):
    return t.detach().contiguous().view(torch.uint8).cpu().numpy().copy()


def _state_bytes(ctl, task, player):
    from vid2player3d_amd import mvae

    out = {"ctl/" + k: B(v) for k, v in ctl._tensors().items()}
    out.update({"player/" + k: B(getattr(player, "_" + k)) for k in mvae.STATE_NAMES})
    out.update({"meters/" + k: B(v) for k, v in ctl._meters.items()})
    out.update({"record/" + k: B(v) for k, v in ctl._record.items()})
    out.update({"task/_dof_state": B(task._dof_state), "task/_rigid_body_state": B(task._rigid_body_state), "task/_ball_root_states": B(task._ball_root_states),
                "ctl/_num_reset": B(ctl._num_reset)})
    return out


@gpu
def test_controller_eval_by_ids_equals_by_flags_and_plays_without_a_host_read():
    from vid2player3d_amd.eval_player import ControllerEvalPlayer

    n, steps = 64, 12
    runs = {}
    for mode in ("ids", "flags"):
        ctl, task, player, target, policy = F.eval_controller(n, pool=F.near_pool())
        assert not player._is_train and ctl.eval_settings["episode_length"] == F.EPISODE_LENGTH
        assert ctl.eval_settings["body_of_smpl"] == tuple(int(b) for b in F.golden()["body_of_smpl"])
        ctl.progress_buf.copy_(torch.arange(n, device=DEV) % (F.EPISODE_LENGTH + 1))
        ctl.start_record(steps)
        ev = ControllerEvalPlayer(ctl, policy, reset_mode=mode)
        assert ControllerEvalPlayer(ctl, policy).reset_mode == "ids"
        if mode == "flags":  # nothing in play waits for the device
            torch.cuda.synchronize()
            was = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                ev.play(steps)
            finally:
                torch.cuda.set_sync_debug_mode(was)
        else:
            ev.play(steps)
        torch.cuda.synchronize()
        assert ctl.frame_index == steps and ctl.joint_rot_all.shape == (n, steps, 24, 3) and ctl.swing_type_all.shape == (n, steps)
        # the last frame's joints: the statement on the engine's exported state of that step (no reset has followed it)
        arrays = dict(ctl.state_arrays(), dof_pos=task._dof_pos.detach().cpu().numpy())
        want = tc.eval_record_reference(ctl.eval_settings, arrays)
        for k, view in (("joint_rot", ctl.joint_rot_all), ("root_pos", ctl.root_pos_all), ("ball_pos", ctl.ball_pos_all), ("target_pos", ctl.target_pos_all),
                        ("phase", ctl.phase_all), ("swing_type_cycle", ctl.swing_type_all)):
            last = view[:, -1].cpu().numpy()
            assert_bits(last, want[k], "%s: the record's last frame, %s" % (mode, k))
        assert int(ctl._num_reset.sum()) > n, "no env was reset after the first reset"
        assert int(ctl._meters["meter_count"].sum()) > 0, "no meter was updated"
        assert bool((ctl._distance == 0).all()), "the test-mode step does not touch _distance"
        runs[mode] = dict(state=_state_bytes(ctl, task, player), best=ctl.select_best().cpu().numpy(), summary=ctl.summary())
        with pytest.raises(RuntimeError, match="all are written"):
            ctl.post_physics_step()
        if hasattr(task, "check"):
            task.check()
        task.close()
    a, b = runs["ids"], runs["flags"]
    for k, v in a["state"].items():
        assert np.array_equal(b["state"][k], v), "reset by flags against reset by ids: %s differs" % k
    assert np.array_equal(a["best"], b["best"])
    assert a["summary"].keys() == b["summary"].keys() and all(np.array_equal(a["summary"][k], b["summary"][k], equal_nan=True) for k in a["summary"])
    assert set(a["summary"]) == set(tc.METER_NAMES) | {m + "_envs" for m in tc.METER_NAMES} and a["summary"]["hit_rate_envs"] > 0
