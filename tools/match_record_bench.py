"""What recording a match costs per control step, on the device (`match.MatchRecorder`: `v2p_match_record_frame`, then
`v2p_match_record_select` = selection + copy, no host read) against the reference's form in torch
(`MVAEControllerVisDual.render_vis`, mvae_controller_vis_dual.py:156-195: six `.cpu()` copies into host arrays - a seventh for
`progress_buf`, which indexes them -, `reset_buf.sum() > 0` and `nonzero()` with their host reads, and the host-side lists), on one GPU
on the two-player controller (`dual_mode: different`) with generator, target, low-level policy (units 1024 / 1024 / 512) and a
`ControllerPolicy` attached, at 10240 envs and record_length 600 - about 2 GB of record on the device (`joint_rot_all` alone 1.77 GB),
and as much on the host for the reference's form.  Everything runs in the same process on one controller.

  (a) the launches alone, device events around `--iters` repetitions and the wall clock around the same loop, closed by a
      synchronisation: `frame` (the frame launch), `select_none` (selection + copy on a step with no finished pair), `select_insert`
      (selection + copy on a step that inserts a rally of record_length - 1 frames; `best_count` is zeroed before every repetition so
      that every one inserts, and `zero_alone` is that fill by itself), `reference_none` / `reference_some` (the reference's form on a
      step with no finished pair / with 1 % of the pairs finished; its lists are emptied before every repetition of the latter, so
      that every one clones a rally).
  (b) `MatchPlayer.play(steps)` per step in 'flags' mode with a recorder and without one, wall clock and device events; after every
      step `reset_buf` is set to the next of `--rotate` patterns with 1 % of the pairs finished (as tools/pair_reset_bench.py does).

The launches of (a) go through the recorder's kept structs (`MatchRecorder._bind()`), as `record_step()` does, so that a figure is the
launch and not the making of its arguments.  The reference's form clamps `progress_buf` to record_length - 1 where the reference would
raise: `reference_*` is its cost on a step inside the record, not its behaviour at overflow (the runs here stay inside).

`--rounds` rounds alternate the forms; one JSON line per figure and a summary line (medians, min - max) at the end.
    python tools/match_record_bench.py [--envs 10240] [--length 600] [--steps 64] [--iters 50] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from pair_reset_bench import DEV, SetFlags, make, timed  # noqa: E402
from vid2player3d_amd import match  # noqa: E402


class ReferenceForm:
    """`render_vis` with cfg env.record on the controller's device tensors: host arrays, host lists."""

    def __init__(self, ctl, length, num_best):
        n = ctl.num_envs
        self.ctl, self.n, self.num_best = ctl, n, num_best
        self.joint_rot = torch.randn((n, 24, 3), device=DEV)  # (`_joint_rot`, which the reference's state update has formed before)
        self.joint_rot_all = torch.zeros((n, length, 24, 3))
        self.root_pos_all, self.ball_pos_all = torch.zeros((n, length, 3)), torch.zeros((n, length, 3))
        self.phase_all = torch.zeros((n, length))
        self.swing_type_all, self.tar_action_all = torch.zeros((n, length), dtype=torch.int64), torch.zeros((n, length), dtype=torch.int64)
        self.length = length
        self.clear()

    def clear(self):
        self.distance_best_all, self.best = [], []

    def __call__(self):
        ctl, t = self.ctl, self.ctl._tensors()
        env_ids = torch.arange(self.n)
        progress = ctl.progress_buf.cpu().clamp_(0, self.length - 1)
        self.joint_rot_all[env_ids, progress] = self.joint_rot.cpu()
        self.root_pos_all[env_ids, progress] = t["rb_state"].view(self.n, 24, 13)[:, 0, 0:3].cpu()
        self.ball_pos_all[env_ids, progress] = t["ball_state"][:, 0:3].cpu()
        self.phase_all[env_ids, progress] = t["phase_pred"].cpu()
        self.swing_type_all[env_ids, progress] = t["swing_type_cycle"].cpu()
        self.tar_action_all[env_ids, progress] = t["tar_action"].cpu()
        if ctl.reset_buf.sum() > 0:
            reset_env_ids = ctl.reset_buf.nonzero(as_tuple=False).flatten()
            distance = ctl._distance[reset_env_ids[::2]] + ctl._distance[reset_env_ids[1::2]]
            max_dist = distance.max()
            if len(self.distance_best_all) == 0 or max_dist > self.distance_best_all[-1]:
                best_env_id = reset_env_ids[::2][torch.argmax(distance)]
                nframes = progress[best_env_id.cpu()]
                ids = torch.LongTensor([best_env_id, best_env_id + 1])
                insert_id = 0
                for dist in self.distance_best_all:
                    if max_dist > dist:
                        break
                    insert_id += 1
                self.distance_best_all.insert(insert_id, max_dist)
                self.best.insert(insert_id, [a[ids, :nframes].clone() for a in (self.joint_rot_all, self.root_pos_all, self.ball_pos_all, self.phase_all,
                                                                               self.swing_type_all, self.tar_action_all)])
        self.distance_best_all, self.best = self.distance_best_all[:self.num_best], self.best[:self.num_best]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=10240)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--best", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--share", type=float, default=0.01, help="share of pairs finished per step")
    ap.add_argument("--rotate", type=int, default=8, help="number of patterns taken in turn")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("match_record_bench measures on a GPU; there is none here")
    n, L = args.envs, args.length
    plain, hook = make(n, "flags")
    ctl = plain.ctl
    rec = match.MatchRecorder(ctl, record_length=L, num_best=args.best)
    recorded = match.MatchPlayer(ctl, plain.policy, "flags", recorder=rec)
    record_bytes = sum(v.numel() * v.element_size() for v in rec._arrays.values())
    rng = np.random.default_rng(1)
    count = max(1, int(round(args.share * (n // 2))))
    some = []
    for _ in range(args.rotate):
        f = np.zeros(n // 2, np.int64)
        f[rng.choice(n // 2, count, replace=False)] = 1
        some.append(torch.as_tensor(np.repeat(f, 2), device=DEV))
    out = {}

    def note(k, v, **kw):
        out.setdefault(k, []).append(v)
        print(json.dumps(dict({"figure": k, "value": round(v, 5)}, **kw)), flush=True)

    # (b) whole runs first (they warm up code objects and GEMM algorithms, and leave the controller in a played state)
    forms = (("plain", plain), ("recorded", recorded))
    for _, m in forms:
        m.play(4)
    torch.cuda.synchronize()
    hook.patterns = some
    for r in range(args.rounds):
        for tag, m in forms:
            hook.k = 0
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            pairs, _ = m.play(args.steps)
            b.record()
            torch.cuda.synchronize()
            note("play_wall_ms_per_step_%s" % tag, (time.perf_counter() - t0) * 1e3 / args.steps, round=r)
            note("play_device_ms_per_step_%s" % tag, a.elapsed_time(b) / args.steps, round=r)
            note("play_pairs_per_step_%s" % tag, float(pairs) / args.steps, round=r)
    kept = rec.best()
    overflow = int(rec.overflow.sum())

    # (a) the launches alone, on the controller's state as the runs left it
    hook.patterns = None
    ref = ReferenceForm(ctl, L, args.best)
    none = torch.zeros(n, dtype=torch.int64, device=DEV)
    pair = n // 4  # the pair of the long rally: its progress is record_length - 1, its distance above every other

    def frame():
        match.launch_record_frame(rec._bind(), n, DEV)

    def select():
        match.launch_record_select(rec._bind(), n, DEV)

    def select_insert():
        rec.best_count.zero_()
        select()

    def reference_some():
        ref.clear()
        ref()

    def long_rally():
        ctl.reset_buf.copy_(some[0])
        ctl.reset_buf[2 * pair:2 * pair + 2] = 1
        ctl.progress_buf[2 * pair:2 * pair + 2] = L - 1
        ctl._distance[2 * pair:2 * pair + 2] = 1e6

    ctl.progress_buf.clamp_(max=L - 1)
    for r in range(args.rounds):
        for tag, fn, prepare in (("frame", frame, lambda: ctl.reset_buf.copy_(none)), ("select_none", select, lambda: ctl.reset_buf.copy_(none)),
                                 ("reference_none", ref, lambda: ctl.reset_buf.copy_(none)), ("select_insert", select_insert, long_rally),
                                 ("zero_alone", rec.best_count.zero_, long_rally), ("reference_some", reference_some, long_rally)):
            prepare()
            dev_ms, wall_ms = timed(fn, args.iters, args.warmup)
            note("%s_device_ms" % tag, dev_ms, round=r, iters=args.iters)
            note("%s_wall_ms" % tag, wall_ms, round=r, iters=args.iters)
    decision = rec.decision.cpu().tolist()
    med = {k: float(np.median(v)) for k, v in out.items()}
    summary = {"summary": "match record on the device against the reference's form, %d envs, record_length %d (%.2f GB of record on the device), num_best %d, %d steps, "
                          "%d of %d pairs finished per step" % (n, L, record_bytes / 1e9, args.best, args.steps, count, n // 2),
               **{k: round(v, 5) for k, v in med.items()}, "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()},
               "kept_after_the_runs": [(e["pair"], round(e["distance"], 3), e["nframes"]) for e in kept], "overflow_envs_after_the_runs": overflow,
               "last_decision": decision, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
