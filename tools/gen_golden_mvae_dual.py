"""Golden data of the two-player motion generator, recorded from the reference itself: tests/golden/mvae_dual.npz.

Built like tools/gen_golden_mvae_player.py: `MVAEPlayer` (vid2player/players/mvae_player.py) with `_is_dual` and two `MotionVAEModel`s
(`_mvae1`, `_mvae2`) are made with `__new__` on the CPU through oracle/ref_shim; the two decoders are the reference's own `PoseMixtureVAE`
with the seeded weights of tests/mvae_fixture.py under two seeds (so avg and std differ between the sides); the reference's OWN
`reset_dual` and `step` run: one reset of all envs, T steps, then a reset of four ids (tests/mvae_dual_fixture.py names the keys).

12 envs, env 2k side 0 and env 2k+1 side 1; three variants (tests/mvae_dual_fixture.VARIANTS).  Every side's six envs walk the script of
the single fixture's first six: on each side every window of that side's player rule (variants with residuals) and every swing-type
transition occur - asserted below.  Latents are chosen env by env and step by step as in the single fixture.

Scatter: `scatter/step`, `scatter/free`, `scatter/reset` = max |float32 - float64| of the reference's own code, as in the single fixture.
Asserted: every branch-picking float (from the numpy statement in float32 and float64, per side) stays 100 x its scatter away from its
threshold, a draw that does not is drawn again; and the root columns of the even rows' condition - which the reference normalises with
side 1's statistics - differ from their own-statistics normalisation by more than 100 x the allowance, so the fixture tells that quirk
from its absence.  Only arrays are stored.  Run where the reference exists:
    python tools/gen_golden_mvae_dual.py
"""
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_mvae_player as G1  # noqa: E402  (installs the shim and imports the reference's modules)

torch, ref_base, ref_model, ref_player, Racket = G1.torch, G1.ref_base, G1.ref_model, G1.ref_player, G1.Racket

from tests import mvae_dual_fixture as DX  # noqa: E402
from tests import mvae_fixture as FX  # noqa: E402
from vid2player3d_amd import mvae  # noqa: E402

N, T, MARGIN = DX.N, DX.T, G1.MARGIN
HALF = N // 2
WINDOWS, CANDIDATES = G1.WINDOWS, G1.CANDIDATES
PRESET, SCRIPTS = G1.PRESET[:HALF], G1.SCRIPTS[:HALF]  # per side: swing types -1, 1, 2, 0, 3, -1
WRIST_SIGN = (1.0, 1.0, -1.0, 1.0, -1.0, -1.0)  # the preferred sign of the right wrist's x of a side's envs (both transitions out of -1)
STATE = DX.STATE


def make_model(sd, avg, std, dtype):
    model = ref_model.PoseMixtureVAE(FX.FRAME, FX.FRAME, FX.FRAME + 2, FX.LATENT, FX.HIDDEN, 1, 1, FX.EXPERTS)
    missing = model.load_state_dict({k: torch.from_numpy(x) for k, x in sd.items()}, strict=False)
    assert all(k.startswith("encoder.") for k in missing.missing_keys) and not missing.unexpected_keys
    model = (model.double() if dtype == torch.float64 else model).eval()
    opt = types.SimpleNamespace(frame_size=FX.FRAME, latent_size=FX.LATENT, num_condition_frames=1, num_future_predictions=1, predict_phase=True,
                                condition_root_x_only=False, no_condition_root_y=False, pose_feature=["root_pos", "root_velo", "joint_pos", "joint_velo", "joint_rotmat"])
    m = ref_base.MotionVAEModel.__new__(ref_base.MotionVAEModel)
    m.opt, m.device, m.model = opt, "cpu", model
    m.avg, m.std = torch.from_numpy(avg).to(dtype), torch.from_numpy(std).to(dtype)
    if dtype == torch.float64:
        def forward(action, condition):  # `MotionVAEModel.forward` (base.py:390-407) without its casts to float32
            output = model.sample(action, condition).view(-1, 1, FX.FRAME + 2)
            return output[:, :, :-2][:, 0], output[:, :, -2:][:, 0]
        m.forward = forward
    return m


def make_player(v, sets, ready, serve, bind, dtype):
    """A reference `MVAEPlayer` in `dual_mode: different` around two reference `MotionVAEModel`s, all made with `__new__`."""
    s = DX.VARIANTS[v]
    p = ref_player.MVAEPlayer.__new__(ref_player.MVAEPlayer)
    p.cfg = dict(DX.cfg(v), test_mode="random")
    p.num_envs, p._is_train, p._enable_physics, p.device, p._is_dual, p._predict_phase = N, s["is_train"], True, "cpu", True, True
    p._mvae1, p._mvae2 = (make_model(sd, avg, std, dtype) for sd, avg, std in sets)
    z = lambda *shape, dt=dtype: torch.zeros(shape, dtype=dt)
    p._root_pos, p._root_vel, p._joint_rot6d, p._joint_rotmat = z(N, 3), z(N, 3), z(N, 24, 6), z(N, 24, 3, 3)
    p._racket_pos, p._racket_normal, p._joint_rot, p._joint_rot_ori = z(N, 3), z(N, 3), z(N, 24, 3), z(N, 24, 3)
    server = 0 if p.cfg.get("serve_from", "near") != "near" else 1  # (mvae_player.py:56-57)
    p._racket = Racket("tennis", "cpu", grip=p.cfg["grip"][server], righthand=p.cfg["righthand"][server])
    mine = mvae.player_settings(p.cfg, s["is_train"], N)["racket"]
    assert mine["righthand"] == bool(p.cfg["righthand"][server]) and list(mine["direction"]) == p._racket.vectors[1].tolist() and list(mine["normal"]) == p._racket.vectors[2].tolist()
    if dtype == torch.float64:
        p._racket.vectors = tuple(x.double() for x in p._racket.vectors)
    p._phase_pred, p._swing_type = z(N), z(N, dt=torch.int64) - 1
    p._swing_type_cycle = p._swing_type.clone()
    p._smpl = types.SimpleNamespace(joint_pos_bind_rel=torch.from_numpy(bind).to(dtype))
    p._conditions = z(N, 1, FX.FRAME)
    p._root_pos_inds = torch.arange(0, 3)
    p._root_vel_inds, p._joint_pos_inds, p._joint_rot6d_inds = torch.arange(3, 6), torch.arange(6, 75), torch.arange(144, 288)
    P = ref_player.SMPLPose
    p._residual_joint_inds = [torch.LongTensor([P.RElbow, P.RWrist] if rh else [P.LElbow, P.LWrist]) for rh in p.cfg["righthand"]]
    # (init_states :113-121)
    p._init_data_ready = torch.from_numpy(ready).to(dtype).view(2, 1, FX.FRAME).repeat(HALF, 1, 1)
    p._init_data_serve = torch.from_numpy(serve).to(dtype).view(2, 1, FX.FRAME).repeat(HALF, 1, 1)
    return p


def ref_reset_dual(p, reaction, recovery, xy, dtype):
    """the reference's `reset_dual` with root positions xy [len(ids),2] (ids ascending): its two draws (:232, side 0's ids then side
    1's) are made to give them - in float64 to 1e-15"""
    xy = torch.from_numpy(np.asarray(xy)).to(dtype)
    draws = [(xy[i::2] - torch.tensor([0.0, -13.0], dtype=dtype)) / torch.tensor([2.0, 1.5], dtype=dtype) + 0.5 for i in (0, 1)]
    real = torch.rand
    torch.rand = lambda shape, device=None: draws.pop(0).clone()
    try:
        p.reset_dual(torch.as_tensor(reaction, dtype=torch.long), torch.as_tensor(recovery, dtype=torch.long))
    finally:
        torch.rand = real
    assert not draws


def state_of(p):
    return {k: getattr(p, "_" + k).detach().clone().numpy() for k in DX.RESET_STATE}


def in64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


def serve_wrist_tie():
    """m00 - m22 of federer's serve-window wrist as the evaluation mode stores it, in float64.  Not training, the residual of a serve is
    zeroed and the wrist's angle-axis is the rule's constant (-0.5, 0.1, -0.5) pi: a rotation with m00 = m22 but for the 1e-6 that
    angle_axis_to_rotation_matrix adds to theta, which leaves -9.5e-7 after rot6d's Gram-Schmidt."""
    m = mvae.angle_axis_to_rotmat_reference(np.array([[-0.5, 0.1, -0.5]]) * math.pi, np.float64)
    m = mvae.rot6d_to_rotmat_reference(np.concatenate([m[..., 0], m[..., 1]], -1), np.float64)
    return float(m[0, 0, 0] - m[0, 2, 2])


def check_margins(p32, p64, what):
    """the single fixture's margins, per side.  One float is left out, recognised by its float64 value: serve_wrist_tie().  It is a
    constant of the rule, no draw moves it, it lies 4 x its own scatter below zero, and what it picks is which of two branches of
    rotation_matrix_to_quaternion computes the SAME quaternion from elements of the same size (m00 and m22 are the two largest): the
    stored angle-axis is continuous across the pick, and no integer hangs on it."""
    tie = serve_wrist_tie()
    for i in (0, 1):
        a, b = G1.with_diagonal(p32[i]), G1.with_diagonal(p64[i])
        if "diagonal" in a:
            x, y = (np.concatenate([np.ravel(u) for u in d["diagonal"]]) for d in (a, b))
            assert x.shape == y.shape, "%s side %d: a trace changes sign between float32 and float64" % (what, i)
            keep = np.abs(y - tie) > 1e-12
            a["diagonal"], b["diagonal"] = [x[keep]], [y[keep]]
        G1.check_margins(a, b, "%s side %d" % (what, i))


def run_variant(v, sets, ws, avgs, stds, bind, rng, total):
    spec = DX.VARIANTS[v]
    st = mvae.player_settings(DX.cfg(v), spec["is_train"], N)
    zero = {k: np.zeros((N,) + shape, dt) for k, shape, dt in (("conditions", (1, FX.FRAME), np.float32), ("root_pos", (3,), np.float32), ("root_vel", (3,), np.float32),
            ("joint_rot6d", (24, 6), np.float32), ("joint_rotmat", (24, 3, 3), np.float32), ("joint_rot", (24, 3), np.float32), ("racket_pos", (3,), np.float32),
            ("racket_normal", (3,), np.float32), ("phase_pred", (), np.float32), ("swing_type", (), np.int64), ("swing_type_cycle", (), np.int64))}
    # the reset of all envs: even pairs receive (ready frame), odd pairs serve; the second reset: DX.PART_*
    reaction = [e for e in range(N) if (e // 2) % 2 == 0]
    recovery = [e for e in range(N) if (e // 2) % 2 == 1]
    for attempt in range(60):  # (initial frames whose rotations come too near a branch of the conversions are drawn again)
        ready, serve = (np.stack([avgs[i] + stds[i] * rng.normal(0, 0.8, FX.FRAME) for i in (0, 1)]).astype(np.float32) for _ in (0, 1))
        out = {"%s/init_ready" % v: ready, "%s/init_serve" % v: serve}
        ids, feature = DX.reset_inputs(out, v, reaction, recovery)
        pr32, pr64 = ({}, {}), ({}, {})
        mvae.mvae_dual_reset_reference(st, avgs, stds, zero, ids, feature, np.zeros((N, 2), np.float32), bind, np.float32, pr32)
        mvae.mvae_dual_reset_reference(st, avgs, stds, zero, ids, feature, np.zeros((N, 2), np.float32), bind, np.float64, pr64)
        try:
            check_margins(pr32, pr64, v + " reset")
            break
        except AssertionError as err:
            failure = err
    else:
        raise failure
    p = make_player(v, sets, ready, serve, bind, torch.float32)
    q = in64(lambda: make_player(v, sets, ready, serve, bind, torch.float64))
    scat = {"step": {}, "free": {}, "reset": {}}

    def worse(kind, a, b):
        for k in a:
            if a[k].dtype.kind == "f":
                scat[kind][k] = max(scat[kind].get(k, 0.0), float(np.abs(a[k].astype(np.float64) - b[k]).max()))
            else:
                assert np.array_equal(a[k], b[k]), "%s: %s differs between float32 and float64" % (kind, k)

    def set_state(pl, s):
        for k, x in s.items():
            getattr(pl, "_" + k)[:] = torch.from_numpy(np.asarray(x)).to(getattr(pl, "_" + k).dtype)

    # ---- the reset of all envs
    root_xy = ((rng.uniform(size=(N, 2)).astype(np.float32) - np.float32(0.5)) * np.array([2.0, 1.5], np.float32) + np.array([0.0, -13.0], np.float32)).astype(np.float32)
    ref_reset_dual(p, reaction, recovery, root_xy, torch.float32)
    root_xy = p._root_pos[:, :2].clone().numpy()  # (the float32 result of the reference's own expression: what the kernel is given)
    in64(lambda: ref_reset_dual(q, reaction, recovery, root_xy, torch.float64))
    worse("reset", state_of(p), state_of(q))
    mine = mvae.mvae_dual_reset_reference(st, avgs, stds, zero, ids, feature, root_xy, bind, np.float32)
    for k, x in state_of(p).items():
        out["%s/reset/%s" % (v, k)] = x
        if x.dtype.kind == "f":
            print("  %s reset %-14s reference - numpy statement %.3g (scatter %.3g)" % (v, k, float(np.abs(x - mine[k].reshape(x.shape)).max()), scat["reset"][k]))
    out["%s/reaction_ids" % v], out["%s/recovery_ids" % v], out["%s/root_xy" % v] = np.array(reaction, np.int64), np.array(recovery, np.int64), root_xy
    preset = np.array([PRESET[e // 2] for e in range(N)], np.int64)
    for pl in (p, q):
        pl._swing_type[:] = torch.from_numpy(preset)
        pl._swing_type_cycle[:] = torch.from_numpy(preset)
    # ---- T steps
    step_keys = ("conditions", "root_pos", "swing_type", "swing_type_cycle")
    traj = {k: [state_of(p)[k]] for k in step_keys}
    post = {k: [] for k in ("root_vel", "joint_rot6d", "joint_rotmat", "phase_pred") + (() if spec["is_train"] else ("joint_rot",))}
    latents, residuals = [], []
    cover = total.setdefault(v, dict(windows=set(), to1=[0, 0], to2=[0, 0], back=[0, 0], kept=[0, 0], quirk=np.inf))
    for t in range(T):
        s = state_of(p)

        def choose():
            res = rng.uniform(-2.0, 2.0, (N, 3)).astype(np.float32)
            z = np.zeros((N, FX.LATENT), np.float32)
            centre = np.zeros((N, 1, FX.LATENT), np.float32)
            lo, hi = (np.array([WINDOWS[SCRIPTS[e // 2][t]][k] for e in range(N)]) for k in (0, 1))
            sign = np.array([WRIST_SIGN[e // 2] for e in range(N)])
            for width in (1.5, 1.0, 0.7, 0.5, 0.35, 0.25, 0.15, 0.1, 0.05, 0.03):  # a search that narrows around the best candidate so far
                cand = np.clip(centre + width * rng.normal(0, 1, (N, CANDIDATES, FX.LATENT)), -3, 3).astype(np.float32)
                cand[:, 0] = centre[:, 0]
                phase, wrist, ph = (np.zeros((N, CANDIDATES)) for _ in range(3))
                for i in (0, 1):
                    o = mvae.decoder_reference(ws[i], cand[i::2].reshape(-1, FX.LATENT), np.repeat(s["conditions"][i::2].reshape(HALF, FX.FRAME), CANDIDATES, 0))
                    ph[i::2] = np.arctan2(o[:, FX.FRAME], o[:, FX.FRAME + 1]).reshape(HALF, CANDIDATES)
                    wrist[i::2] = (o[:, 6 + 20 * 3] * stds[i][6 + 20 * 3] + avgs[i][6 + 20 * 3]).reshape(HALF, CANDIDATES)
                phase = np.where(ph < 0, ph + 2 * math.pi, ph)
                ok = (phase > lo[:, None] + 0.02) & (phase < hi[:, None] - 0.02) & (np.abs(ph) > 0.02) & (np.abs(wrist) > 0.02)
                cost = np.abs(phase - (lo + hi)[:, None] / 2) + np.where(wrist * sign[:, None] > 0, 0, 0.5) + np.where(ok, 0, 1.0)  # (the wrist's sign: wanted more than the window's centre, less than the window)
                best = np.argmin(cost, 1)
                centre = cand[np.arange(N), best][:, None]
                if ok[np.arange(N), best].all():
                    break
            for e in range(N):
                assert ok[e, best[e]], "variant %s env %d step %d: no candidate latent puts the phase into (%g, %g)" % (v, e, t, lo[e], hi[e])
                z[e] = cand[e, best[e]]
            return z, res

        for attempt in range(60):  # (a draw whose floats come too near a threshold inside the rotation conversions is drawn again)
            z, res = choose()
            r_in = res if spec["residual"] else None
            p32, p64 = ({}, {}), ({}, {})
            mine = mvae.mvae_dual_step_reference(st, ws, avgs, stds, s, z, r_in, np.float32, p32)
            mvae.mvae_dual_step_reference(st, ws, avgs, stds, s, z, r_in, np.float64, p64)
            try:
                check_margins(p32, p64, "%s step %d" % (v, t))
                break
            except AssertionError as err:
                failure = err
        else:
            raise failure
        latents.append(z)
        residuals.append(res)
        T64 = lambda x: None if x is None else torch.from_numpy(x).double()
        T32 = lambda x: None if x is None else torch.from_numpy(x)
        # one teacher-forced step in float64 from the recorded float32 state, then the free-running float64 sequence
        free64 = state_of(q)
        set_state(q, s)
        in64(lambda: q.step(T64(z), T64(r_in)))
        forced64 = state_of(q)
        set_state(q, free64)
        in64(lambda: q.step(T64(z), T64(r_in)))
        p.step(T32(z), T32(r_in))
        a = state_of(p)
        drop = ("racket_pos", "racket_normal") + (("joint_rot",) if spec["is_train"] else ())
        worse("step", {k: x for k, x in a.items() if k not in drop}, forced64)
        worse("free", {k: x for k, x in a.items() if k not in drop}, state_of(q))
        for k in traj:
            traj[k].append(a[k])
        for k in post:
            post[k].append(a[k])
        # ---- the numpy statement, the quirk's visibility, coverage
        for k in ("conditions", "joint_rot6d", "joint_rotmat", "phase_pred"):
            total["statement"] = max(total.get("statement", 0.0), float(np.abs(mine[k].reshape(a[k].shape) - a[k]).max()))
        assert np.array_equal(mine["swing_type"], a["swing_type"]) and np.array_equal(mine["swing_type_cycle"], a["swing_type_cycle"])
        own = (a["root_pos"][0::2] - avgs[0][:3]) / stds[0][:3]
        cover["quirk"] = min(cover["quirk"], float(np.abs(a["conditions"][0::2, 0, :3] - own).max(1).min()))
        before, after = s["swing_type"], a["swing_type"]
        for i in (0, 1):
            b_, a_, c_ = before[i::2], after[i::2], a["swing_type_cycle"][i::2]
            cover["to1"][i] += int(((b_ == -1) & (a_ == 1)).sum())
            cover["to2"][i] += int(((b_ == -1) & (a_ == 2)).sum())
            cover["back"][i] += int(((b_ != -1) & (a_ == -1)).sum())
            cover["kept"][i] += int(((a_ == -1) & (c_ != -1)).sum())
            ph = a["phase_pred"][i::2]
            for r, (sw, lo, hi, ge, _) in enumerate(mvae.RESIDUAL_RULES[spec["player"][i]]["rows"]):
                if ((a_ == sw) & ((ph >= np.float32(lo)) if ge else (ph > np.float32(lo))) & (ph < np.float32(hi))).any():
                    cover["windows"].add((i, r))
    for k, x in traj.items():
        out["%s/traj/%s" % (v, k)] = np.stack(x)
    for k, x in post.items():
        out["%s/post/%s" % (v, k)] = np.stack(x)
    out["%s/latents" % v], out["%s/preset_swing" % v] = np.stack(latents), preset
    if spec["residual"]:
        out["%s/residual" % v] = np.stack(residuals)
    # ---- the second reset: four ids, from the state after the last step
    part_xy = ((rng.uniform(size=(len(DX.PART_IDS), 2)).astype(np.float32) - np.float32(0.5)) * np.array([2.0, 1.5], np.float32) + np.array([0.0, -13.0], np.float32)).astype(np.float32)
    before = state_of(p)
    expect_before = DX.state_before_part(out, v)
    assert all(np.array_equal(before[k], expect_before[k]) for k in before), "the state before the second reset is not what the fixture's keys give"
    ref_reset_dual(p, DX.PART_REACTION, DX.PART_RECOVERY, part_xy, torch.float32)
    rows = list(DX.PART_IDS)
    part_xy = p._root_pos[rows, :2].clone().numpy()
    set_state(q, before)
    in64(lambda: ref_reset_dual(q, DX.PART_REACTION, DX.PART_RECOVERY, part_xy, torch.float64))
    after = state_of(p)
    others = [e for e in range(N) if e not in rows]
    assert all(np.array_equal(after[k][others], before[k][others]) for k in after)
    worse("reset", {k: x[rows] for k, x in after.items()}, {k: x[rows] for k, x in state_of(q).items()})
    out["%s/part/root_xy" % v] = part_xy
    for k, x in after.items():
        out["%s/part/%s" % (v, k)] = x[rows]
    return out, scat


def main():
    rng = np.random.default_rng(2047)
    sets = [FX.seeded_state_dict(seed) for seed in DX.WEIGHT_SEEDS]
    ws = tuple(mvae.weights_from_state_dict(sd) for sd, _, _ in sets)
    avgs, stds = tuple(a for _, a, _ in sets), tuple(s for _, _, s in sets)
    bind = rng.uniform(-0.3, 0.3, (N, 24, 3)).astype(np.float32)
    out = {"joint_pos_bind_rel": bind}
    for i, (sd, avg, std) in enumerate(sets):
        out["weights_sha256_%d" % i] = np.frombuffer(FX.weights_sha256(sd, avg, std).encode(), dtype=np.uint8).copy()
    total = {}
    scatter = {"step": {}, "free": {}, "reset": {}}
    for v in DX.VARIANTS:
        o, sc = run_variant(v, sets, ws, avgs, stds, bind, rng, total)
        out.update(o)
        for kind in sc:
            for k, x in sc[kind].items():
                scatter[kind][k] = max(scatter[kind].get(k, 0.0), x)
    for kind in scatter:
        for k, x in scatter[kind].items():
            out["scatter/%s/%s" % (kind, k)] = np.float64(x)
            print("scatter %-5s %-16s %.3g" % (kind, k, x))
    print("numpy statement - reference: %.3g" % total.pop("statement"))
    allowance = FX.ORDER_ALLOWANCE * max(scatter["step"]["conditions"], scatter["free"]["conditions"])
    for v, c in total.items():
        print(v, c)
        spec = DX.VARIANTS[v]
        for i in (0, 1):
            assert c["to1"][i] and c["to2"][i] and c["back"][i] and c["kept"][i], "variant %s side %d: a swing-type transition is missing" % (v, i)
            if spec["residual"]:
                for r in range(len(mvae.RESIDUAL_RULES[spec["player"][i]]["rows"])):
                    assert (i, r) in c["windows"], "variant %s side %d: window %d of %s never occurs" % (v, i, r, spec["player"][i])
        assert c["quirk"] > MARGIN * allowance, "variant %s: the even rows' root columns come within %.3g of their own-statistics normalisation (allowance %.3g)" % (v, c["quirk"], allowance)
    np.savez_compressed(DX.GOLDEN, **out)
    print("wrote", os.path.relpath(DX.GOLDEN, G1.REPO), "%.2f MB" % (os.path.getsize(DX.GOLDEN) / 1e6))


if __name__ == "__main__":
    main()
