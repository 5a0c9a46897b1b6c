"""Golden data of the MotionVAE motion generator, recorded from the reference itself: tests/golden/mvae_player.npz.

`MVAEPlayer` (vid2player/players/mvae_player.py) and `MotionVAEModel` (vid2player/motion_vae/base.py) are imported on the CPU through
oracle/ref_shim, with inert stand-ins for the modules they cannot have here (the SMPL visualizer, tensorboard).  Objects made with
`__new__` get their attributes set by hand; the decoder is the reference's own `PoseMixtureVAE` with the seeded weights of
tests/mvae_fixture.py loaded into it, and the reference's OWN `reset` and `step` run: one reset of all envs, then T consecutive steps.

Four variants, one per player, one of them left-handed, one in evaluation mode.  Recorded: the inputs (init feature, root draw, latents,
residuals, the swing types preset after the reset - types 0 and 3 can be reached in no other way), the state after the reset, the
trajectory of the tensors a step reads (`traj/`, T + 1 states) and what every step writes besides (`post/`).  The weights are not
stored; the fixture carries their sha256.

The latents are CHOSEN, env by env and step by step, among candidates drawn from N(0, 1): the one that puts the predicted phase into
the window the env's script asks for, away from every threshold.  The script walks every env through the phase windows of the residual
rule, so that every window of every player, every swing-type transition and both signs of the clamp occur.

Scatter.  The same steps are run with the reference's model and inputs in float64 (torch's default dtype set to float64; the model's
`forward`, which casts to float32, restated in double).  `scatter/step/<name>`: max |float32 - float64| of one step from the recorded
float32 state; `scatter/free/<name>`: of the free-running sequences; `scatter/reset/<name>`: of the reset.  The tests allow the kernel
8 x these.  Every float that is compared with a threshold or picks a branch - taken from the float32 and the float64 evaluation of the
numpy statement, vid2player3d_amd/mvae.py - stays 100 x its own scatter away from it, so integers must match exactly whatever the
order of summation.  Only arrays are stored.  Run where the reference exists:
    python tools/gen_golden_mvae_player.py
"""
import math
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True  # never leave __pycache__ in the read-only reference mount

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)

from ref_shim.install import REFERENCE_ROOT, _Sink, install  # noqa: E402

install()
for absent in ("smpl_visualizer", "smpl_visualizer.smpl", "torch.utils.tensorboard", "tqdm"):
    try:
        __import__(absent)
    except Exception:
        sys.modules[absent] = _Sink(absent)
sys.path.insert(0, os.path.join(REFERENCE_ROOT, "vid2player"))

import torch  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

import motion_vae.base as ref_base  # noqa: E402
import motion_vae.model as ref_model  # noqa: E402
import players.mvae_player as ref_player  # noqa: E402
from utils.racket import Racket  # noqa: E402

from tests import mvae_fixture as FX  # noqa: E402
from vid2player3d_amd import mvae  # noqa: E402

OUT = FX.GOLDEN
N, T, CANDIDATES, MARGIN = 10, 6, 512, 100.0
VARIANT_SETTINGS = {"A": ("djokovic", True, True), "B": ("federer", True, True), "C": ("nadal", False, True), "D": ("djokovic", True, False)}
THRESHOLDS = (2.0, 2.5, 3.0, 3.1, 3.2, 3.3, 3.5)
# the phase windows an env's script names: between two neighbouring thresholds, 0.02 inside
WINDOWS = [(1.0, 2.0), (2.0, 2.5), (2.5, 3.0), (3.0, 3.1), (3.1, 3.2), (3.2, 3.3), (3.3, 3.5), (3.5, 4.5)]
# env e: the swing type preset after the reset and the windows of its T steps
PRESET = (-1, 1, 2, 0, 3, -1, 1, 2, 0, -1)
SCRIPTS = ((1, 2, 3, 4, 5, 7), (1, 2, 3, 4, 6, 7), (1, 2, 3, 4, 5, 7), (1, 2, 3, 5, 6, 7), (1, 2, 4, 6, 7, 1), (0, 2, 3, 4, 7, 1), (2, 3, 4, 5, 6, 7), (1, 2, 4, 5, 6, 7),
           (2, 3, 4, 5, 6, 7), (0, 1, 7, 2, 4, 7))
STATE = FX.FLOAT_STATE + FX.INT_STATE


def make_player(name, righthand, is_train, model, avg, std, init, bind, dtype):
    """A reference `MVAEPlayer` around a reference `MotionVAEModel`, both made with `__new__`."""
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
    p = ref_player.MVAEPlayer.__new__(ref_player.MVAEPlayer)
    p.cfg = {"player": name, "righthand": righthand, "add_residual_dof": "euler", "test_mode": "random"}
    p.num_envs, p._is_train, p._enable_physics, p.device, p._is_dual, p._mvae, p._predict_phase = N, is_train, True, "cpu", False, m, True
    z = lambda *shape, dt=dtype: torch.zeros(shape, dtype=dt)
    p._root_pos, p._root_vel, p._joint_rot6d, p._joint_rotmat = z(N, 3), z(N, 3), z(N, 24, 6), z(N, 24, 3, 3)
    p._racket_pos, p._racket_normal, p._joint_rot, p._joint_rot_ori = z(N, 3), z(N, 3), z(N, 24, 3), z(N, 24, 3)
    p._racket = Racket("tennis", "cpu", righthand=righthand)
    if dtype == torch.float64:
        p._racket.vectors = tuple(v.double() for v in p._racket.vectors)
    p._phase_pred, p._swing_type = z(N), z(N, dt=torch.int64) - 1
    p._swing_type_cycle = p._swing_type.clone()
    p._smpl = types.SimpleNamespace(joint_pos_bind_rel=torch.from_numpy(bind).to(dtype)[None].repeat(N, 1, 1))
    p._conditions = z(N, 1, FX.FRAME)
    p._root_pos_inds = torch.arange(0, 3)
    p._root_vel_inds, p._joint_pos_inds, p._joint_rot6d_inds = torch.arange(3, 6), torch.arange(6, 75), torch.arange(144, 288)
    P = ref_player.SMPLPose
    p._residual_joint_inds = torch.LongTensor([P.RElbow, P.RWrist] if righthand else [P.LElbow, P.LWrist])
    p._init_data = torch.from_numpy(init).to(dtype).view(N, 1, FX.FRAME)
    return p


def ref_reset(p, draw):
    """the reference's `reset` of all envs with `draw` [N,2] as what its torch.rand returns (:232)"""
    real = torch.rand
    torch.rand = lambda shape, device=None: draw.clone()
    try:
        p.reset(torch.arange(N))
    finally:
        torch.rand = real


def state_of(p):
    return {k: getattr(p, "_" + k).detach().clone().numpy() for k in STATE + ("racket_pos", "racket_normal")}


def set_state(p, s):
    for k, v in s.items():
        getattr(p, "_" + k)[:] = torch.from_numpy(np.asarray(v)).to(getattr(p, "_" + k).dtype)


def near(values, thresholds):
    """distance of every value to its nearest threshold"""
    v = np.asarray(values, dtype=np.float64).ravel()
    return np.min(np.abs(v[:, None] - np.asarray(thresholds, dtype=np.float64)[None]), axis=1) if v.size else np.zeros(0)


def with_diagonal(p):
    """the probes with `diagonal`: the three differences of the diagonal where they can decide, that is where the trace is not positive"""
    if "trace" not in p or "diagonal" in p:
        return p
    pick = [np.concatenate([d[t <= 0] for d in ds]) for t, *ds in zip(p["trace"], p["diag01"], p["diag02"], p["diag12"])]
    return dict(p, diagonal=pick)


def check_margins(p32, p64, what):
    """every float that picks a branch stays MARGIN x its scatter (float32 against float64 evaluation of the same statement) away"""
    p32, p64 = with_diagonal(p32), with_diagonal(p64)
    for name, thresholds in (("phase", THRESHOLDS), ("atan2", (0.0,)), ("wrist_x", (0.0,)), ("rot6d_norm", (1e-8,)), ("trace", (0.0,)), ("diagonal", (0.0,)), ("quat_w", (0.0,)), ("sin2", (0.0,)), ("theta2", (1e-6,))):
        if name not in p32:
            continue
        a, b = (np.concatenate([np.ravel(x) for x in (d[name] if isinstance(d[name], list) else [d[name]])]) for d in (p32, p64))
        keep = a != 0 if name in ("sin2", "theta2") else np.ones(len(a), bool)  # (exact zeros - a joint the rule sets to no rotation - are exact everywhere)
        a, b = a[keep], b[keep]
        if not a.size:
            continue
        scatter = float(np.abs(a.astype(np.float64) - b).max())
        dist = float(near(a, thresholds).min())
        if name in ("sin2", "theta2"):  # (squares that span decades: every value against its own scatter, at least an ulp)
            own = np.maximum(np.abs(a.astype(np.float64) - b), 1.2e-7 * np.abs(a))
            worst = int(np.argmin(near(a, thresholds) / own))
            scatter, dist = float(own[worst]), float(near(a, thresholds)[worst])
        assert dist >= MARGIN * scatter, "%s: %s comes within %.3g of a threshold, scatter %.3g" % (what, name, dist, scatter)


def run_variant(v, sd, w, avg, std, bind, rng, total):
    name, righthand, is_train = VARIANT_SETTINGS[v]
    st = mvae.player_settings({"player": name, "righthand": righthand, "add_residual_dof": "euler"}, is_train)
    model = ref_model.PoseMixtureVAE(FX.FRAME, FX.FRAME, FX.FRAME + 2, FX.LATENT, FX.HIDDEN, 1, 1, FX.EXPERTS)
    missing = model.load_state_dict({k: torch.from_numpy(x) for k, x in sd.items()}, strict=False)
    assert all(k.startswith("encoder.") for k in missing.missing_keys) and not missing.unexpected_keys
    model.eval()
    model64 = ref_model.PoseMixtureVAE(FX.FRAME, FX.FRAME, FX.FRAME + 2, FX.LATENT, FX.HIDDEN, 1, 1, FX.EXPERTS)
    model64.load_state_dict(model.state_dict())
    model64 = model64.double().eval()
    for attempt in range(40):  # (an init feature whose rotations come too near a branch of the conversions is drawn again)
        init = (avg + std * rng.normal(0, 0.8, (N, FX.FRAME))).astype(np.float32)
        zero = {k: np.zeros((N,) + shape, dt) for k, shape, dt in (("conditions", (1, FX.FRAME), np.float32), ("root_pos", (3,), np.float32), ("root_vel", (3,), np.float32),
                ("joint_rot6d", (24, 6), np.float32), ("joint_rotmat", (24, 3, 3), np.float32), ("joint_rot", (24, 3), np.float32), ("racket_pos", (3,), np.float32),
                ("racket_normal", (3,), np.float32), ("phase_pred", (), np.float32), ("swing_type", (), np.int64), ("swing_type_cycle", (), np.int64))}
        pr32, pr64 = {}, {}
        mvae.mvae_reset_reference(st, avg, std, zero, np.arange(N), init, np.zeros((N, 2), np.float32), bind, np.float32, pr32)
        mvae.mvae_reset_reference(st, avg, std, zero, np.arange(N), init, np.zeros((N, 2), np.float32), bind, np.float64, pr64)
        try:
            check_margins(pr32, pr64, v + " reset")
            break
        except AssertionError as err:
            failure = err
    else:
        raise failure
    draw = torch.from_numpy(rng.uniform(size=(N, 2)).astype(np.float32))
    p = make_player(name, righthand, is_train, model, avg, std, init, bind, torch.float32)
    torch.set_default_dtype(torch.float64)
    q = make_player(name, righthand, is_train, model64, avg, std, init, bind, torch.float64)
    torch.set_default_dtype(torch.float32)
    out, scat = {}, {"step": {}, "free": {}, "reset": {}}

    def worse(kind, a, b):
        for k in a:
            if a[k].dtype.kind == "f":
                scat[kind][k] = max(scat[kind].get(k, 0.0), float(np.abs(a[k].astype(np.float64) - b[k]).max()))
            else:
                assert np.array_equal(a[k], b[k]), "%s: %s differs between float32 and float64" % (kind, k)

    def in64(fn):
        torch.set_default_dtype(torch.float64)
        try:
            return fn()
        finally:
            torch.set_default_dtype(torch.float32)

    # ---- the reset
    ref_reset(p, draw)
    root_xy = p._root_pos[:, :2].clone().numpy()  # (the float32 result of the reference's own expression: what the kernel is given)
    # (in float64 the draw that gives the same xy to 1e-15)
    in64(lambda: ref_reset(q, (torch.from_numpy(root_xy).double() - torch.tensor([0.0, -13.0])) / torch.tensor([2.0, 1.5]) + 0.5))
    worse("reset", state_of(p), state_of(q))
    mine = mvae.mvae_reset_reference(st, avg, std, zero, np.arange(N), init, root_xy, bind, np.float32)
    for k, x in state_of(p).items():
        out["%s/reset/%s" % (v, k)] = x
        if x.dtype.kind == "f":
            print("  %s reset %-14s reference - numpy statement %.3g (scatter %.3g)" % (v, k, float(np.abs(x - mine[k].reshape(x.shape)).max()), scat["reset"][k]))
    preset = np.array(PRESET, np.int64)
    for pl in (p, q):
        pl._swing_type[:] = torch.from_numpy(preset)
        pl._swing_type_cycle[:] = torch.from_numpy(preset)
    # ---- T steps
    traj = {k: [state_of(p)[k]] for k in ("conditions", "root_pos", "swing_type", "swing_type_cycle")}
    post = {k: [] for k in ("root_vel", "joint_rot6d", "joint_rotmat", "phase_pred") + (() if is_train else ("joint_rot",))}
    latents, residuals = [], []
    for t in range(T):
        s = state_of(p)
        def choose():
            res = rng.uniform(-2.0, 2.0, (N, 3)).astype(np.float32)
            # choose every env's latent among candidates: phase inside the scripted window, everything away from its thresholds
            z = np.zeros((N, FX.LATENT), np.float32)
            centre = np.zeros((N, 1, FX.LATENT), np.float32)
            lo, hi = (np.array([WINDOWS[SCRIPTS[e][t]][k] for e in range(N)]) for k in (0, 1))
            sign = np.array([1.0 if (e + t) % 2 else -1.0 for e in range(N)])
            for width in (1.5, 1.0, 0.7, 0.5, 0.35, 0.25, 0.15, 0.1, 0.05, 0.03):  # a search that narrows around the best candidate so far
                cand = np.clip(centre + width * rng.normal(0, 1, (N, CANDIDATES, FX.LATENT)), -3, 3).astype(np.float32)
                cand[:, 0] = centre[:, 0]
                o = mvae.decoder_reference(w, cand.reshape(-1, FX.LATENT), np.repeat(s["conditions"].reshape(N, FX.FRAME), CANDIDATES, 0))
                ph = np.arctan2(o[:, FX.FRAME], o[:, FX.FRAME + 1]).reshape(N, CANDIDATES)
                phase = np.where(ph < 0, ph + 2 * math.pi, ph)
                wrist = (o[:, 6 + 20 * 3] * std[6 + 20 * 3] + avg[6 + 20 * 3]).reshape(N, CANDIDATES)
                ok = (phase > lo[:, None] + 0.02) & (phase < hi[:, None] - 0.02) & (np.abs(ph) > 0.02) & (np.abs(wrist) > 0.02)
                cost = np.abs(phase - (lo + hi)[:, None] / 2) + np.where(wrist * sign[:, None] > 0, 0, 0.01) + np.where(ok, 0, 1.0)  # (the wrist's sign: a preference)
                best = np.argmin(cost, 1)
                centre = cand[np.arange(N), best][:, None]
                if ok[np.arange(N), best].all():
                    break
            for e in range(N):
                assert ok[e, best[e]], "variant %s env %d step %d: no candidate latent puts the phase into (%g, %g)" % (v, e, t, lo[e], hi[e])
                z[e] = cand[e, best[e]]
            return z, res

        # (a draw whose floats come too near a threshold inside the rotation conversions is drawn again)
        for attempt in range(40):
            z, res = choose()
            p32, p64 = {}, {}
            mine = mvae.mvae_step_reference(st, w, avg, std, s, z, res, np.float32, p32)
            mvae.mvae_step_reference(st, w, avg, std, s, z, res, np.float64, p64)
            try:
                check_margins(p32, p64, "%s step %d" % (v, t))
                break
            except AssertionError as err:
                failure = err
        else:
            raise failure
        latents.append(z)
        residuals.append(res)
        # one teacher-forced step in float64 from the recorded float32 state, then the free-running float64 sequence
        free64 = state_of(q)
        set_state(q, s)
        in64(lambda: q.step(torch.from_numpy(z).double(), torch.from_numpy(res).double()))
        forced64 = state_of(q)
        set_state(q, free64)
        in64(lambda: q.step(torch.from_numpy(z).double(), torch.from_numpy(res).double()))
        p.step(torch.from_numpy(z), torch.from_numpy(res))
        a = state_of(p)
        drop = ("racket_pos", "racket_normal") + (("joint_rot",) if is_train else ())
        worse("step", {k: x for k, x in a.items() if k not in drop}, forced64)
        worse("free", {k: x for k, x in a.items() if k not in drop}, state_of(q))
        for k in traj:
            traj[k].append(a[k])
        for k in post:
            post[k].append(a[k])
        # ---- margins and coverage, from the numpy statement in float32 and float64
        for k in ("conditions", "joint_rot6d", "joint_rotmat", "phase_pred"):
            total["statement"] = max(total.get("statement", 0.0), float(np.abs(mine[k].reshape(a[k].shape) - a[k]).max()))
        assert np.array_equal(mine["swing_type"], a["swing_type"]) and np.array_equal(mine["swing_type_cycle"], a["swing_type_cycle"])
        coef = p32["coef"]
        total["winners"] |= set(np.argmax(coef, 1).tolist())
        total["rows"] += len(coef)
        total["peaked"] += int((coef.max(1) > 0.5).sum())
        for i in range(2):  # both ELU branches in both layers that have one
            assert (p32["pre%d" % i] > 0).any() and (p32["pre%d" % i] <= 0).any()
        total["spread"].append([float(p32["pre%d" % i].std()) for i in range(3)])
        before, after = s["swing_type"], a["swing_type"]
        total["to1"] += int(((before == -1) & (after == 1)).sum())
        total["to2"] += int(((before == -1) & (after == 2)).sum())
        total["back"] += int(((before != -1) & (after == -1)).sum())
        total["kept"] += int(((after == -1) & (a["swing_type_cycle"] != -1)).sum())
        rule = mvae.RESIDUAL_RULES[name]
        for i, (sw, lo, hi, ge, _) in enumerate(rule["rows"]):
            m = (after == sw) & ((a["phase_pred"] >= np.float32(lo)) if ge else (a["phase_pred"] > np.float32(lo))) & (a["phase_pred"] < np.float32(hi))
            if m.any():
                total["windows"].add((name, i))
                if (res[m] > 1).any():
                    total["clamp"].add((name, i, 1))
                if (res[m] < -1).any():
                    total["clamp"].add((name, i, -1))
    for k, x in traj.items():
        out["%s/traj/%s" % (v, k)] = np.stack(x)
    for k, x in post.items():
        out["%s/post/%s" % (v, k)] = np.stack(x)
    out["%s/latents" % v], out["%s/residual" % v] = np.stack(latents), np.stack(residuals)
    out["%s/init_feature" % v], out["%s/root_xy" % v], out["%s/preset_swing" % v] = init, root_xy, preset
    out["%s/settings" % v] = np.array([FX.PLAYER_NAMES.index(name), int(righthand), int(is_train)], np.int64)
    return out, scat


def main():
    rng = np.random.default_rng(2031)
    sd, avg, std = FX.seeded_state_dict()
    w = mvae.weights_from_state_dict(sd)
    bind = rng.uniform(-0.3, 0.3, (24, 3)).astype(np.float32)
    out = {"joint_pos_bind_rel": bind, "weights_sha256": np.frombuffer(FX.weights_sha256(sd, avg, std).encode(), dtype=np.uint8).copy()}
    total = dict(winners=set(), rows=0, peaked=0, elu=[set(), set(), set()], spread=[], to1=0, to2=0, back=0, kept=0, windows=set(), clamp=set())
    scatter = {"step": {}, "free": {}, "reset": {}}
    for v in FX.VARIANTS:
        o, sc = run_variant(v, sd, w, avg, std, bind, rng, total)
        out.update(o)
        for kind in sc:
            for k, x in sc[kind].items():
                scatter[kind][k] = max(scatter[kind].get(k, 0.0), x)
    for kind in scatter:
        for k, x in scatter[kind].items():
            out["scatter/%s/%s" % (kind, k)] = np.float64(x)
            print("scatter %-5s %-16s %.3g" % (kind, k, x))
    print("spread of the pre-activations per layer:", np.mean(total["spread"], 0), " numpy statement - reference: %.3g" % total["statement"])
    print({k: x for k, x in total.items() if k not in ("spread", "elu")})
    assert total["winners"] == set(range(FX.EXPERTS)), "not every expert has the largest coefficient in some row: %s" % total["winners"]
    assert total["peaked"] * 4 >= total["rows"], "the largest coefficient exceeds 0.5 in %d of %d rows only" % (total["peaked"], total["rows"])
    assert total["to1"] and total["to2"] and total["back"] and total["kept"], "a swing-type transition is missing"
    for name, rule in mvae.RESIDUAL_RULES.items():
        for i in range(len(rule["rows"])):
            assert (name, i) in total["windows"], "window %d of %s never occurs" % (i, name)
            assert (name, i, 1) in total["clamp"] and (name, i, -1) in total["clamp"], "window %d of %s lacks a sign of the clamp" % (i, name)
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.relpath(OUT, REPO), "%.2f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
