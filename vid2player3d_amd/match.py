"""Playing a match: `V2PPlayer.run` (vid2player/players/v2p_player.py:133-156) for the two-player controller of the match configs
(`nadal_federer`, `federer_djokovic`: `dual_mode: different`, network `vid2player_dual`, two single-player checkpoints through
`dual_model_cp`).  Every step of that loop resets the pairs that are done, computes the deterministic action and steps the controller.

`MatchPlayer(ctl, policy, reset_mode)`: ctl a `DualTennisControllerTask` with its generator, target and low-level policy attached, policy
a `policies.ControllerPolicy` over it.  reset_mode 'ids' is the reference's form - `done.nonzero()` (the host waits for the device), then
`ctl.reset(ids)`; 'flags' is `ctl.reset_pairs_by_flags()`, the same launches every step and no host read.  Both give the same bits when
`ctl._reset_root_xy` [N,2] and `ctl._reset_serve_draws` [N/2,3] stand in for the draws; without them 'ids' draws from torch's stream and
'flags' from the kernels' own.

`run(steps)` keeps on the device, and returns after the run, the number of pairs that finished and the sum of `_distance` over both
players of the finished pairs - what the reference ranks matches by (mvae_controller_vis_dual.py:167).

The record of a match run - what `run.py --test` produces for a match config, `MVAEControllerVisDual.render_vis` with cfg env.record
(mvae_controller_vis_dual.py:156-195) - is `MatchRecorder(ctl, record_length, num_best)`: every control step each env's frame (SMPL
pose, root, ball, phase, swing type, `_tar_action`) goes to slot `progress_buf` of the env's own `record_length` slots, and when pairs
finish the `num_best` rallies with the largest summed `_distance` are kept, on the device (`v2p_match_record_frame`,
`v2p_match_record_select`, csrc/match_record.hip) - no `.cpu()`, no `nonzero()`, no host list.  `match_record_reference(rec, s)` states
the law once in numpy; `MatchPlayer(..., recorder=...)` records a run; `MatchRecorder.best()` is the one host read and
`ball_track(entry)` the ball a viewer would show (render_one_result:278-285).  `target_pos_all`, which the reference allocates and the
dual class never writes, is left out.  `best(fix_two_hand=...)` applies the two-hand backhand fix of cfg v2p `fix_two_hand_backhand_post`
(two_hand_fix.py).  Not built: the SMPL mesh, video / HTML output and the on-screen viewer branch of `render_vis`."""
import ctypes as C

import numpy as np
import torch

from . import _lib

RESET_MODES = ("ids", "flags")
FRAME_NAMES = _lib.MATCH_RECORD_FRAME_NAMES  # joint_rot, root_pos, ball_pos, phase, swing_type, tar_action
FRAME_SHAPES = dict(joint_rot=(24, 3), root_pos=(3,), ball_pos=(3,), phase=(), swing_type=(), tar_action=())
FRAME_DTYPES = dict(joint_rot=np.float32, root_pos=np.float32, ball_pos=np.float32, phase=np.float32, swing_type=np.int64, tar_action=np.int64)
TABLE_DTYPES = dict(best_distance=np.float32, best_pair=np.int32, best_nframes=np.int32, best_slot=np.int32)
MAX_BEST = _lib.MATCH_RECORD_MAX_BEST  # the cap of num_best: the selection's insertion is one thread's loop over the list
RECORD_LENGTH = 1800  # the reference's hard-coded length (mvae_controller_vis_dual.py:52)


# ------------------------------------------------------------------------------------------------------------------ the statement
def record_settings(record_length=RECORD_LENGTH, num_best=1, body_of_smpl=None):
    """The settings of the record as a plain dict; what the entries refuse is refused here with the same words."""
    L, K = int(record_length), int(num_best)
    if not 1 <= L <= _lib.MATCH_RECORD_MAX_LENGTH:
        raise ValueError("match record: record_length %d outside 1..%d" % (L, _lib.MATCH_RECORD_MAX_LENGTH))
    if not 1 <= K <= MAX_BEST:
        raise ValueError("match record: num_best %d outside 1..%d" % (K, MAX_BEST))
    body = tuple(int(b) for b in (range(24) if body_of_smpl is None else body_of_smpl))
    if sorted(body) != list(range(24)) or body[0] != 0:
        raise ValueError("match record: body_of_smpl must be a permutation of 0..23 with the root first")
    return dict(record_length=L, num_best=K, body_of_smpl=body)


def record_arrays(st, n, fill=None):
    """The record before the first frame as numpy arrays: the six `*_all` [n,L,...], `overflow` [n], the tables by rank, `best_count`,
    `decision` and the storage `best_*` [K,2,L,...].  fill None: zeros, as the reference allocates; else {float: v, int: w} for the
    `*_all` and storage arrays (the tests' poison)."""
    n, L, K = int(n), st["record_length"], st["num_best"]
    if n <= 0 or n % 2:
        raise ValueError("match record: n %d is not a positive even number (envs 2k and 2k+1 are a pair)" % n)
    val = lambda k: 0 if fill is None else fill[float if FRAME_DTYPES[k] == np.float32 else int]
    rec = dict(st)
    for k in FRAME_NAMES:
        rec[k + "_all"] = np.full((n, L) + FRAME_SHAPES[k], val(k), FRAME_DTYPES[k])
        rec["best_" + k] = np.full((K, 2, L) + FRAME_SHAPES[k], val(k), FRAME_DTYPES[k])
    rec["overflow"] = np.zeros(n, np.int32)
    for k, dt in TABLE_DTYPES.items():
        rec[k] = np.zeros(K, dt)
    rec["best_count"] = np.zeros(1, np.int32)
    rec["decision"] = np.array([-1, -1, 0], np.int32)
    return rec


def match_frame_reference(st, s):
    """The frame of every env (mvae_controller_vis_dual.py:157-162) from the arrays of `s`, under FRAME_NAMES: `rb_state` [n,24,13],
    `dof_pos` [n,69], `ball_state` [n,13], `phase_pred`, `swing_type_cycle`, `tar_action`.  The pose row is the evaluation's statement."""
    from .tasks.tennis_controller import pose_row_reference

    rb = np.asarray(s["rb_state"], dtype=np.float32).reshape(-1, 24, 13)
    return dict(joint_rot=pose_row_reference(st["body_of_smpl"], rb, s["dof_pos"]), root_pos=rb[:, 0, 0:3].copy(), ball_pos=np.array(s["ball_state"], dtype=np.float32)[:, 0:3],
                phase=np.array(s["phase_pred"], dtype=np.float32), swing_type=np.array(s["swing_type_cycle"], dtype=np.int64), tar_action=np.array(s["tar_action"], dtype=np.int64))


def match_record_reference(rec, s, select=True):
    """One `render_vis` on arrays.  rec: record_arrays(...) as the previous call left it; s: the arrays of `match_frame_reference` plus
    `progress`, `reset` [n] int64 and `distance` [n] float32, as they stand after the control step.  Returns the record after; nothing in
    `rec` or `s` is modified.  select False: the frames alone (`v2p_match_record_frame`).

    1. env e's frame goes to slot p = progress[e]; p outside [0, L) stores nothing and raises overflow[e].
    2. a pair is finished when either `reset` word is up; d = distance[2k] + distance[2k+1] in float32; the candidate is the lowest
       finished pair that reaches the maximum of d (a NaN d is no candidate).  It is inserted iff the list is empty or d > list[-1], in
       front of the first entry with d > entry, and the list is cut to num_best.  The tables are by rank; best_slot[rank] names the
       storage slot: the next free one, or the evicted entry's.  nframes = min(progress[2k], L).
    3. slots [0, nframes) of both envs are copied to the storage slot; what it held behind nframes stays."""
    L, K = rec["record_length"], rec["num_best"]
    o = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in rec.items()}
    progress = np.asarray(s["progress"], dtype=np.int64)
    frame = match_frame_reference(rec, s)
    inside = (progress >= 0) & (progress < L)
    ids = np.flatnonzero(inside)
    for k in FRAME_NAMES:
        o[k + "_all"][ids, progress[ids]] = frame[k][ids]
    o["overflow"][~inside] = 1
    if not select:
        return o
    o["decision"] = np.array([-1, -1, 0], np.int32)
    done = (np.asarray(s["reset"]).reshape(-1, 2) != 0).any(1)
    dist = np.asarray(s["distance"], dtype=np.float32)
    d = dist[0::2] + dist[1::2]
    cand = done & ~np.isnan(d)
    if not cand.any():
        return o
    max_dist = d[cand].max()
    pair = int(np.flatnonzero(cand & (d == max_dist))[0])
    count = int(o["best_count"][0])
    if count and not max_dist > o["best_distance"][count - 1]:
        return o
    pos = 0
    while pos < count and not max_dist > o["best_distance"][pos]:
        pos += 1
    nframes = int(min(max(progress[2 * pair], 0), L))
    slot = count if count < K else int(o["best_slot"][K - 1])
    kept = min(count + 1, K)
    for k, new in (("best_distance", max_dist), ("best_pair", pair), ("best_nframes", nframes), ("best_slot", slot)):
        o[k][pos + 1:kept] = o[k][pos:kept - 1].copy()
        o[k][pos] = new
    o["best_count"][0] = kept
    o["decision"] = np.array([pair, slot, nframes], np.int32)
    for k in FRAME_NAMES:
        o["best_" + k][slot, :, :nframes] = o[k + "_all"][2 * pair:2 * pair + 2, :nframes]
    return o


def best_of(rec):
    """The kept rallies of a record (numpy or torch arrays under the statement's names, the tables on the host), best first: dicts
    {pair, distance, nframes, joint_rot [2,nframes,24,3], root_pos, ball_pos, phase, swing_type, tar_action}."""
    out = []
    for r in range(int(rec["best_count"][0])):
        slot, nframes = int(rec["best_slot"][r]), int(rec["best_nframes"][r])
        e = dict(pair=int(rec["best_pair"][r]), distance=float(rec["best_distance"][r]), nframes=nframes)
        e.update({k: rec["best_" + k][slot, :, :nframes] for k in FRAME_NAMES})
        out.append(e)
    return out


def ball_track(entry):
    """The ball a viewer shows for a kept rally (render_one_result:278-285), [nframes,3]: per frame env 0's ball where
    `tar_action[0, i] == 1`, else env 1's with x and y negated (the far side's frame).  On a copy: the entry is not modified."""
    ball, tar = torch.as_tensor(entry["ball_pos"]).clone(), torch.as_tensor(entry["tar_action"])
    far = ball[1] * torch.tensor([-1.0, -1.0, 1.0], dtype=ball.dtype, device=ball.device)
    return torch.where((tar[0] == 1).unsqueeze(-1), ball[0], far)


# ------------------------------------------------------------------------------------------------------------------ the launches
def record_structs(st, n, tensors):
    """(v2p_match_record_cfg, v2p_match_record_buffers) of record_settings(...) and a dict of device tensors under
    _lib.MATCH_RECORD_BUFFER_NAMES.  Every size is checked against n, L and num_best here: the kernels trust them."""
    n, L, K = int(n), st["record_length"], st["num_best"]
    if n <= 0 or n % 2:
        raise ValueError("match record: n %d is not a positive even number (envs 2k and 2k+1 are a pair)" % n)
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    want = dict(rb_state=(n * 24 * 13, f32), dof_state=(n * 69 * 2, f32), ball_state=(n * 13, f32), phase_pred=(n, f32), swing_type_cycle=(n, i64), tar_action=(n, i64),
                progress=(n, i64), reset=(n, i64), distance=(n, f32), overflow=(n, i32), best_distance=(K, f32), best_pair=(K, i32), best_nframes=(K, i32),
                best_slot=(K, i32), best_count=(1, i32), decision=(3, i32))
    for k in FRAME_NAMES:
        dtype = i64 if FRAME_DTYPES[k] == np.int64 else f32
        width = int(np.prod(FRAME_SHAPES[k], dtype=np.int64))
        want[k + "_all"], want["best_" + k] = (n * L * width, dtype), (K * 2 * L * width, dtype)
    b = _lib.MatchRecordBuffers()
    for k in _lib.MATCH_RECORD_BUFFER_NAMES:
        t = tensors.get(k)
        if t is None:
            raise ValueError("match record: array %s is missing" % k)
        if not torch.is_tensor(t) or not t.is_cuda or not t.is_contiguous() or t.dtype != want[k][1] or t.numel() != want[k][0]:
            raise RuntimeError("match record: %s must be a contiguous %s GPU tensor of %d elements (there is no CPU path)" % (k, str(want[k][1]).replace("torch.", ""), want[k][0]))
        setattr(b, k, t.data_ptr())
    c = _lib.MatchRecordCfg(record_length=L, num_best=K)
    c.body_of_smpl[:] = st["body_of_smpl"]
    return c, b


def launch_record_frame(structs, n, device):
    with torch.cuda.device(device):
        _lib.check(_lib.load().v2p_match_record_frame(C.byref(structs[0]), int(n), C.byref(structs[1]), _lib.current_stream(device)), "v2p_match_record_frame")


def launch_record_select(structs, n, device):
    with torch.cuda.device(device):
        _lib.check(_lib.load().v2p_match_record_select(C.byref(structs[0]), int(n), C.byref(structs[1]), _lib.current_stream(device)), "v2p_match_record_select")


class MatchRecorder:
    """The record of a match run over `ctl`, a `DualTennisControllerTask` with its motion generator attached.  record_length: the slots
    of an env (the reference: 1800; 10240 envs at 1800 slots are 6.1 GB, mostly `joint_rot_all`); num_best None: cfg env.num_eg,
    default 1, at most MAX_BEST.  It owns the six `*_all` arrays [N,L,...] (zeros before a frame is written, as the reference's),
    `overflow` [N] and the best list.  `record_init()` after the first reset and `record_step()` after every `ctl.step` are the
    launches - nothing in them waits for the device; `best()` is the one host read."""

    def __init__(self, ctl, record_length=RECORD_LENGTH, num_best=None):
        from .mvae_target import tree_from_model
        from .tasks.tennis_controller_dual import DualTennisControllerTask

        if not isinstance(ctl, DualTennisControllerTask):
            raise TypeError("MatchRecorder records a DualTennisControllerTask (a match has two players)")
        if num_best is None:
            num_best = (ctl.cfg.get("env") or {}).get("num_eg", 1)
        smpl_of_body = tree_from_model(ctl.task.body_names, ctl.task.body_model.parents)[1]
        self.settings = record_settings(record_length, num_best, [smpl_of_body.index(j) for j in range(24)])
        self.ctl, self.device, self.num_envs = ctl, ctl.device, ctl.num_envs
        self.record_length, self.num_best = self.settings["record_length"], self.settings["num_best"]
        self._arrays = {k: torch.as_tensor(v, device=self.device) for k, v in record_arrays(self.settings, self.num_envs).items() if isinstance(v, np.ndarray)}
        for k, v in self._arrays.items():
            setattr(self, k, v)
        self._bound = None

    def _sources(self):
        ctl = self.ctl
        if ctl._mvae_player is None:
            raise RuntimeError("MatchRecorder: the controller has no motion generator attached (phase and swing type are its)")
        t = ctl._tensors()
        return dict(dof_state=ctl.task._dof_state, **{k: t[k] for k in _lib.MATCH_RECORD_INPUT_NAMES if k != "dof_state"})

    def _bind(self):
        """The structs of the launches, made at the first launch from the controller's tensors as they stand and kept with those
        tensors (so that no address outlives its memory): a step's two launches then cost no host work beyond the calls."""
        if self._bound is None:
            held = dict(self._arrays, **self._sources())
            self._bound = (record_structs(self.settings, self.num_envs, held), held)
        return self._bound[0]

    def rebind(self):
        """Make the structs anew at the next launch (after another generator or task was attached to the controller)."""
        self._bound = None

    def _check_bound(self):
        """once per run, in `record_init()`: the controller's tensors are still the ones the structs name - a generator or task
        attached since would otherwise be recorded from its predecessor's tensors.  Host pointers only, no device read."""
        if self._bound is not None:
            held = self._bound[1]
            moved = [k for k, t in self._sources().items() if t.data_ptr() != held[k].data_ptr()]
            if moved:
                raise RuntimeError("MatchRecorder: the controller's %s moved since the recorder bound them (a generator or task was attached): call rebind()" % ", ".join(moved))

    def record_init(self):
        """`render_vis(init=True)` (v2p_player.py:142): every env's slot `progress_buf` - 0 after the first reset - gets the frame of
        the engine's state as it stands.  No later step writes slot 0, so it holds this frame for the whole run."""
        self._check_bound()
        launch_record_frame(self._bind(), self.num_envs, self.device)

    def record_step(self):
        """`render_vis()` after a control step: the frames, then the selection and the copy of the kept pair."""
        structs = self._bind()
        launch_record_frame(structs, self.num_envs, self.device)
        launch_record_select(structs, self.num_envs, self.device)

    def best(self, fix_two_hand=None, num_iters=None):
        """The kept rallies, best first, as dicts {pair, distance, nframes, joint_rot [2,nframes,24,3], root_pos, ball_pos, phase,
        swing_type, tar_action} of device tensors (views of the storage).  The one host read: the four tables and the count.
        fix_two_hand: the two-hand backhand fix of `render_one_result` (mvae_controller_vis_dual.py:213-231) on `joint_rot`, one launch
        for every kept rally and side (`two_hand_fix.fix_two_hand_backhand`, num_iters None: its 500); None follows cfg v2p
        `fix_two_hand_backhand_post`.  A fixed `joint_rot` is a new tensor, the storage stays as recorded."""
        names = tuple(TABLE_DTYPES)
        host = torch.cat([self._arrays[k].view(torch.int32) for k in names] + [self.best_count]).cpu().numpy()
        K = self.num_best
        tables = {k: host[i * K:(i + 1) * K].view(TABLE_DTYPES[k]) for i, k in enumerate(names)}
        entries = best_of(dict(self._arrays, best_count=host[4 * K:], **tables))
        if fix_two_hand is None:
            fix_two_hand = bool(self.ctl.cfg_v2p.get("fix_two_hand_backhand_post"))
        if fix_two_hand and entries:
            self._fix_two_hand(entries, [int(tables["best_slot"][r]) for r in range(len(entries))], num_iters)
        return entries

    def fix_sides(self):
        """[(skipped, righthand)] of the two sides, the reference's rule (mvae_controller_vis_dual.py:217-224): with `dual_mode:
        different` cfg v2p `player[j]` and `righthand[j]`, else `player` and `righthand` (default True) for both; a side whose player
        name starts with `federer` is skipped."""
        from .two_hand_fix import skips_fix

        v2p = self.ctl.cfg_v2p
        sides = []
        for j in range(2):
            if v2p.get("dual_mode") == "different":
                player, righthand = v2p["player"][j], v2p["righthand"][j]
            else:
                player, righthand = v2p.get("player"), v2p.get("righthand", True)
            sides.append((skips_fix(player), bool(righthand)))
        return sides

    def fix_bind_rows(self):
        """The reference's `_smpl.joint_pos_bind` [N,24,3], a row per env, from the attached imitation target."""
        target = self.ctl._imitation_target
        if target is None:
            raise RuntimeError("MatchRecorder: the two-hand fix reads joint_pos_bind of the controller's imitation target, and none is attached")
        from .two_hand_fix import bind_rows_of

        return bind_rows_of(target)

    def _fix_two_hand(self, entries, slots, num_iters):
        from . import two_hand_fix as thf

        K, L, sides = self.num_best, self.record_length, self.fix_sides()
        nframes, righthand = np.zeros(2 * K, np.int32), np.zeros(2 * K, np.int32)
        for e, slot in zip(entries, slots):
            for j, (skipped, rh) in enumerate(sides):
                nframes[2 * slot + j], righthand[2 * slot + j] = (0 if skipped else e["nframes"]), int(rh)
        st = thf.fix_settings(self.ctl.task.body_names, self.ctl.task.body_model.parents)
        dev = lambda a: torch.as_tensor(a, device=self.device)
        out = thf.fix_two_hand_backhand(self.best_joint_rot.view(2 * K, L, 24, 3), self.best_phase.view(2 * K, L), self.best_swing_type.view(2 * K, L), dev(nframes),
                                        dev(righthand), self.fix_bind_rows(), thf.NUM_ITERS if num_iters is None else num_iters, settings=st)
        for e, slot in zip(entries, slots):
            e["joint_rot"] = torch.stack([e["joint_rot"][j].clone() if skipped else out[2 * slot + j, :e["nframes"]] for j, (skipped, _) in enumerate(sides)])

    ball_track = staticmethod(ball_track)


class MatchPlayer:
    def __init__(self, ctl, policy, reset_mode="ids", recorder=None):
        from .policies import ControllerPolicy
        from .tasks.tennis_controller_dual import DualTennisControllerTask

        if not isinstance(ctl, DualTennisControllerTask):
            raise TypeError("MatchPlayer plays a DualTennisControllerTask (a match has two players)")
        if not isinstance(policy, ControllerPolicy) or policy.ctl is not ctl:
            raise ValueError("MatchPlayer: policy must be a ControllerPolicy over the same controller")
        if reset_mode not in RESET_MODES:
            raise ValueError("MatchPlayer: reset_mode %r is neither 'ids' nor 'flags'" % (reset_mode,))
        if recorder is not None and (not isinstance(recorder, MatchRecorder) or recorder.ctl is not ctl):
            raise ValueError("MatchPlayer: recorder must be a MatchRecorder over the same controller")
        self.ctl, self.policy, self.reset_mode, self.device, self.recorder = ctl, policy, reset_mode, ctl.device, recorder
        self.finished_pairs = torch.zeros((), dtype=torch.int64, device=self.device)
        self.finished_distance = torch.zeros((), dtype=torch.float64, device=self.device)

    def _reset_done(self):
        ctl = self.ctl
        if self.reset_mode == "flags":
            ctl.reset_pairs_by_flags()
            return
        ids = ctl.reset_buf.nonzero(as_tuple=False).flatten()  # (the host read of the reference's loop)
        xy, draws = ctl._reset_root_xy, ctl._reset_serve_draws
        ctl.reset(ids, root_xy=None if xy is None or ids.numel() == 0 else xy[ids], serve_vel_draws=None if draws is None or ids.numel() == 0 else draws[ids[::2] >> 1])

    def _count_finished(self):
        """(the dual step's law raises both flags of a pair; either one counts, as in `reset_pairs_by_flags`)"""
        ctl = self.ctl
        done = (ctl.reset_buf.view(-1, 2) != 0).any(1)
        self.finished_pairs += done.sum()
        self.finished_distance += (ctl._distance.view(-1, 2).sum(1).double() * done).sum()

    @torch.no_grad()
    def play(self, steps):
        """The loop of `run` without its closing host read: returns the two device scalars (`finished_pairs` int64, `finished_distance`
        float64) of this run.  With reset_mode 'flags' nothing in it waits for the device, with a recorder or without: the recorder
        gets `record_init()` after the reset and `record_step()` after every step, as `V2PPlayer.run` calls `render_vis`."""
        ctl, recorder = self.ctl, self.recorder
        ctl.reset()
        if recorder is not None:
            recorder.record_init()
        self.finished_pairs.zero_()
        self.finished_distance.zero_()
        for _ in range(int(steps)):
            self._reset_done()
            ctl.step(self.policy.act())
            if recorder is not None:
                recorder.record_step()
            self._count_finished()
        return self.finished_pairs, self.finished_distance

    def run(self, steps):
        """`steps` control steps; returns (finished pairs, the summed distance of the finished pairs) of this run as Python numbers - the
        one host read, after the last step."""
        pairs, distance = self.play(steps)
        return int(pairs), float(distance)
