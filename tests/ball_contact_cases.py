"""Designed ball launches for tests/test_gpu_ball_contacts.py: the generation rule of the ball's contacts stated in numpy, the cases
(one env each) and the batches of 3 and 34 envs.  CPU only: numpy, scipy and the C oracle's point x hull distance.

The humanoid floats upright in its T-pose with the root at 3 m (no link near the ground), with small joint rates
and a small root spin from a generator seeded by the CASE (an env holds the same state wherever its case is put).  Every launch is
computed in float64 from the rigid-body state of that pose and rounded to float32; what a case "is" is then judged on the rounded launch
by `classify`, the numpy statement of the rule (oracle/phys/v2p_phys_oracle.c, substep_impl):

  cylinder j of the racket   closest point of the solid cylinder; normal from it to the ball centre, +-axis by the sign of t when the
                             centre lies inside; gap = distance - R; row when gap < contact_offset + h max(0, -v_rel)
  hull of link b != racket's distance of the centre from the hull (body frame); normal from the closest point, from the centre of the
                             bounding box when the centre lies inside, +z at that centre itself; same activation test; the kernel
                             looks at a hull only inside the reach of its bounding box, R + contact_offset + h v_max
  selection                  the three candidates with the smallest gaps, nearest first, ties to the lower link
"""
import functools
import zlib

import numpy as np
from scipy.spatial import ConvexHull
from scipy.spatial.transform import Rotation

H = 1.0 / 120.0   # substep
COFF = 0.02       # contact offset (oracle.default_params)
RB = 0.032        # ball radius
MARGIN = 1e-4     # metres: every decision of a designed case is at least this far from flipping
BASE = [0.5, 0.5, 0.5, 0.5]
SPIN = np.array([20.0, -30.0, 10.0])
CENTRE_EPS = 1e-5  # a centre this close to the bounding-box centre leaves along +z


@functools.lru_cache(maxsize=None)
def models(player):
    from vid2player3d_amd import racket as R
    from vid2player3d_amd.model import load_baked_model

    return R.with_racket(load_baked_model(), player=player)


@functools.lru_cache(maxsize=None)
def _hull_planes(model, b):
    """Outward face planes [m, 4] (unit normal, offset) of link b's hull."""
    return ConvexHull(hull_of(model, b)).equations


def hull_of(model, b):
    off = np.asarray(model.hull_offsets)
    return np.asarray(model.hull_verts, dtype=np.float64)[off[b]:off[b + 1]]


# ------------------------------------------------------------------------------------------------ the rule, in numpy
def cyl_rule(rb, geom, j, ball):
    """Ball x solid cylinder j of the racket (closed form)."""
    b = geom["racket_link"]
    c = geom["cylinders"][j]
    Rw = Rotation.from_quat(rb[b, 3:7]).as_matrix()
    x, xd, w = rb[b, 0:3], rb[b, 7:10], rb[b, 10:13]
    cw, aw, hl, rc = x + Rw @ np.asarray(c["center"]), Rw @ np.asarray(c["axis"]), float(c["half_len"]), float(c["radius"])
    s = ball[0:3]
    d = s - cw
    t = d @ aw
    q = d - t * aw
    rho = np.linalg.norm(q)
    inside = abs(t) <= hl and rho <= rc
    pt = cw + np.clip(t, -hl, hl) * aw + (rc / rho if rho > rc else 1.0) * q
    dist = 0.0 if inside else np.linalg.norm(s - pt)
    n = (1.0 if t >= 0 else -1.0) * aw if inside else (s - pt) / dist
    vrel = (ball[7:10] - xd - np.cross(w, pt - x)) @ n
    gap, thr = dist - RB, COFF + H * max(0.0, -vrel)
    region = "inside" if inside else ("side" if abs(t) < hl else ("rim" if rho > rc else "face")) + ("" if abs(t) < hl else "+" if t > 0 else "-")
    if inside:
        region += "+" if t >= 0 else "-"
        bound = min(hl - abs(t), rc - rho, abs(t))  # (|t|: the sign of t picks the cap)
    else:
        bound = min(abs(abs(t) - hl), abs(rho - rc))
    return {"region": region, "t": t, "rho": rho, "pt": pt, "n": n, "gap": gap, "vrel": vrel, "thr": thr, "row": bool(gap < thr), "act_margin": abs(gap - thr), "region_margin": bound}


def hull_rule(rb, model, b, ball, want_feature=False):
    """Ball x the hull of link b: box reach, distance (the oracle's GJK; `feature` = vertices that carry the closest point, from the
    quadratic program of tests/test_oracle_ball_hull.py), normal, activation."""
    from oracle.phys_oracle import hull_closest

    V = hull_of(model, b)
    Rw = Rotation.from_quat(rb[b, 3:7]).as_matrix()
    x, xd, w = rb[b, 0:3], rb[b, 7:10], rb[b, 10:13]
    cb = Rw.T @ (ball[0:3] - x)
    lo, hi = V.min(0), V.max(0)
    ac, ae = 0.5 * (lo + hi), 0.5 * (hi - lo)
    ex = np.maximum(np.abs(cb - ac) - ae, 0.0)
    vmax = np.linalg.norm(ball[7:10] - xd) + np.linalg.norm(w) * (np.linalg.norm(ac) + np.linalg.norm(ae))
    reach = RB + COFF + H * vmax
    dist, pb = hull_closest(V, cb)
    out = {"link": b, "box_dist": float(np.linalg.norm(ex)), "reach": reach, "in_box": bool(np.linalg.norm(ex) < reach), "centre_dist": float(np.linalg.norm(cb - ac))}
    inside = dist <= 1e-6
    if inside:
        out["depth"] = float(-(_hull_planes(model, b) @ np.concatenate([cb, [1.0]])).max())  # how far inside: distance to the nearest face
        e = cb - ac
        nb = e / np.linalg.norm(e) if np.linalg.norm(e) > CENTRE_EPS else np.array([0.0, 0.0, 1.0])
        dist, pb = 0.0, cb
    else:
        nb = (cb - pb) / dist
    nw, rl = Rw @ nb, Rw @ pb
    vrel = (ball[7:10] - xd - np.cross(w, rl)) @ nw
    gap, thr = dist - RB, COFF + H * max(0.0, -vrel)
    out.update(inside=bool(inside), dist=dist, n=nw, gap=gap, vrel=vrel, thr=thr, row=bool(gap < thr), act_margin=abs(gap - thr))
    if not inside:
        # the feature that carries the closest point: the vertices within 1e-7 m of the supporting plane there (1 vertex, 2 edge, 3 face),
        # its barycentric weights, and how far below that plane the next vertex lies
        depth = -((V - pb) @ nb)
        on = np.nonzero(depth < 1e-7)[0]
        A = np.concatenate([V[on].T, np.ones((1, len(on)))])
        wts = np.linalg.lstsq(A, np.concatenate([pb, [1.0]]), rcond=None)[0]
        out.update(feature=len(on), feature_slack=float(np.sort(depth)[len(on)]), feature_weight=float(wts.min()), feature_fit=float(np.abs(A @ wts - np.concatenate([pb, [1.0]])).max()))
    if want_feature and not inside:  # the same distance from a quadratic program that is neither the oracle nor the kernel
        from tests.test_oracle_ball_hull import qp_closest

        d2, _ = qp_closest(V, cb)
        out["qp_err"] = abs(d2 - dist)
    return out


def classify(rb, model, geom, ball, want_feature=()):
    """Everything the rule decides for one env: both cylinders, every hull, the selection."""
    cyl = [cyl_rule(rb, geom, j, ball) for j in range(len(geom["cylinders"]))]
    hulls = [hull_rule(rb, model, b, ball, want_feature=b in want_feature) for b in range(24) if b != geom["racket_link"]]
    for hr in hulls:
        assert hr["in_box"] or not hr["row"], "the box reach covers every active hull"
    cand = sorted((hr for hr in hulls if hr["row"]), key=lambda hr: (hr["gap"], hr["link"]))
    own = hull_rule(rb, model, geom["racket_link"], ball)
    return {"cyl": cyl, "hulls": {hr["link"]: hr for hr in hulls}, "cand": [hr["link"] for hr in cand], "cand_gaps": [hr["gap"] for hr in cand], "racket_hull": own,
            "boxes": [hr["link"] for hr in hulls if hr["in_box"]]}


def decisive_margin(cl, at_centre=None):
    """Smallest distance of any decision of this env from flipping: activation of every cylinder and hull, region of a cylinder with a
    row, centre inside or outside of every hull (1e-6 m of distance on one side, the depth below the nearest face on the other), gaps of
    competing candidates, and for a centre inside a hull its distance from the bounding-box centre against CENTRE_EPS.  at_centre: the
    link whose box centre the launch is meant to sit on - that one decision cannot have room of its own (it is a statement about
    float32 resolution: the test asserts the centre within CENTRE_EPS / 10 instead)."""
    m = min(c["act_margin"] for c in cl["cyl"])
    m = min([m] + [c["region_margin"] for c in cl["cyl"] if c["row"]])
    for hr in list(cl["hulls"].values()):
        m = min(m, hr["act_margin"], hr["depth"] if hr["inside"] else hr["dist"] - 1e-6)
        if hr["inside"] and hr["link"] != at_centre:
            m = min(m, hr["centre_dist"] - CENTRE_EPS)
    g = np.asarray(cl["cand_gaps"])
    if len(g) > 1:
        m = min(m, float(np.diff(g).min()))
    return m


# ------------------------------------------------------------------------------------------------ poses and states
def state_of(case):
    """(root [13], dof_pos [69], dof_vel [69]) float32, a function of the case's name alone."""
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    root = np.zeros(13)
    root[2] = 3.0
    root[3:7] = BASE
    root[7:10] = rng.normal(0, 0.1, 3)
    root[10:13] = rng.normal(0, 0.2, 3)
    return root.astype(np.float32), np.zeros(69, dtype=np.float32), rng.normal(0, 0.3, 69).astype(np.float32)


def oracle_for(player, solver, state, without=()):
    """A PhysOracle in `state` with the ball attached; without: links whose hulls are taken away (the ball cannot touch them)."""
    from oracle.phys_oracle import PhysOracle, _dptr, default_params

    model, geom = models(player)
    o = PhysOracle(model, default_params(solver_type={"pgs": 0, "tgs": 1}[solver]), kp=model.kp.astype(np.float32), kd=model.kd.astype(np.float32))
    if without:
        off = np.asarray(model.hull_offsets).copy()
        keep = np.ones(off[-1], dtype=bool)
        for b in without:
            keep[off[b]:off[b + 1]] = False
        cnt = np.diff(off)
        cnt[list(without)] = 0
        o._hv = np.ascontiguousarray(np.asarray(model.hull_verts, dtype=np.float64)[keep])
        o.model.hull_verts = _dptr(o._hv)
        o.model.hull_offsets[:] = [0] + np.cumsum(cnt).tolist()
    o.set_state(*state)
    o.attach_ball(geom)
    return o


# ------------------------------------------------------------------------------------------------ launches
def _ball(pos, vel):
    ball = np.zeros(13)
    ball[0:3], ball[6], ball[7:10], ball[10:13] = pos, 1.0, vel, SPIN
    return ball.astype(np.float32).astype(np.float64)


def _link_vel_at(rb, b, p):
    return rb[b, 7:10] + np.cross(rb[b, 10:13], p - rb[b, 0:3])


def _approach(rb, b, point, normal, gap, speed):
    """Ball `gap` off the surface point `point` of link b along `normal`, closing at `speed` along it (receding when negative)."""
    normal = normal / np.linalg.norm(normal)
    return _ball(point + (RB + gap) * normal, _link_vel_at(rb, b, point) - speed * normal)


def _cyl_frame(rb, geom, j):
    b = geom["racket_link"]
    Rw = Rotation.from_quat(rb[b, 3:7]).as_matrix()
    c = geom["cylinders"][j]
    cw, aw = rb[b, 0:3] + Rw @ np.asarray(c["center"]), Rw @ np.asarray(c["axis"])
    away = Rw @ (np.asarray(geom["cylinders"][1]["center"]) / np.linalg.norm(geom["cylinders"][1]["center"]))  # from the wrist along the handle to the head
    return b, cw, aw, float(c["half_len"]), float(c["radius"]), away


def launch_cyl(kind):
    def make(ctx):
        rb, geom = ctx["rb"], ctx["geom"]
        b, c1, a1, hl1, r1, away = _cyl_frame(rb, geom, 1)
        _, c0, a0, hl0, r0, _ = _cyl_frame(rb, geom, 0)
        inplane = np.cross(a1, away)  # in the plane of the head, across the handle
        if kind == "face+":    # beyond the 0.11 m the scenario tests reach
            return _approach(rb, b, c1 + hl1 * a1 + 0.13 * inplane, a1, 0.01, 10.0)
        if kind == "face-":
            return _approach(rb, b, c1 - hl1 * a1 + 0.05 * away - 0.04 * inplane, -a1, 0.01, 10.0)
        if kind == "side":
            return _approach(rb, b, c1 + 0.006 * a1 + r1 * away, away, 0.01, 10.0)
        if kind == "rim":
            u = (away + 0.3 * inplane) / np.linalg.norm(away + 0.3 * inplane)
            return _approach(rb, b, c1 + hl1 * a1 + r1 * u, a1 + u, 0.015, 4.0)  # (the normal turns with the position here: slower, for the conditioning)
        if kind in ("inside+", "inside-"):  # centre inside the solid head, 1 cm off its middle plane
            p = c1 + (0.01 if kind == "inside+" else -0.01) * a1 + 0.06 * away + 0.03 * inplane
            return _ball(p, _link_vel_at(rb, b, p) + 0.3 * inplane)
        if kind == "handle side":  # between the hand and the throat, from out of the racket's plane
            p = c0 + 0.045 * (a0 @ away) * a0
            return _approach(rb, b, p + r0 * a1, a1, 0.008, 5.0)  # (a thin cylinder: the normal turns quickly with the position)
        if kind == "handle cap":   # the end at the wrist
            e = -(a0 @ away) * a0
            return _approach(rb, b, c0 + hl0 * e + 0.004 * a1, e, 0.01, 6.0)
        if kind == "throat":       # on the handle's side, 2 cm before the head's rim: both cylinders
            p = c0 + (hl0 - 0.02) * (a0 @ away) * a0
            return _approach(rb, b, p + r0 * a1, a1, 0.005, 5.0)
        if kind == "racket link":  # beside the handle IN the racket's plane: inside the hull of the racket's link (wrist + rims)
            p = c0 + 0.03 * (a0 @ away) * a0
            return _approach(rb, b, p + r0 * inplane, inplane, 0.008, 5.0)
        if kind == "spec closing":   # 6 cm off the face: beyond the contact offset, within reach of a 10 m/s ball
            return _approach(rb, b, c1 + hl1 * a1 - 0.03 * inplane, a1, 0.06, 10.0)
        if kind == "spec receding":
            return _approach(rb, b, c1 + hl1 * a1 - 0.03 * inplane, a1, 0.06, -10.0)
        raise KeyError(kind)
    return make


@functools.lru_cache(maxsize=None)
def _hull_features(player, b):
    """Faces (merged coplanar triangles are not needed: baked hulls are in general position), edges and vertices of link b's hull with
    their outward normals, body frame."""
    V = hull_of(models(player)[0], b)
    ch = ConvexHull(V)
    faces = [(tuple(sorted(s)), eq[:3]) for s, eq in zip(ch.simplices, ch.equations)]
    edges, verts = {}, {}
    for s, nrm in faces:
        for i in range(3):
            edges.setdefault(tuple(sorted((s[i], s[(i + 1) % 3]))), []).append(nrm)
            verts.setdefault(s[i], []).append(nrm)
    return V, faces, edges, verts


def launch_hull(b, feature, direction, gap=0.01, speed=8.0):
    """Towards the vertex / edge / face of link b whose outward normal points most along the world `direction`."""
    def make(ctx):
        rb = ctx["rb"]
        V, faces, edges, verts = _hull_features(ctx["player"], b)
        Rw = Rotation.from_quat(rb[b, 3:7]).as_matrix()
        want = Rw.T @ (np.asarray(direction, dtype=np.float64) / np.linalg.norm(direction))
        cands = []
        if feature == 3:
            for s, nrm in faces:
                a, bb, c = V[list(s)]
                cands.append((nrm @ want, (a + bb + c) / 3.0, nrm))
        elif feature == 2:
            for (i, j), ns in edges.items():
                nrm = (ns[0] + ns[1]) / np.linalg.norm(ns[0] + ns[1])
                cands.append((nrm @ want, 0.5 * (V[i] + V[j]), nrm))
        else:
            for i, ns in verts.items():
                nrm = np.mean(ns, axis=0)
                cands.append((nrm @ want / np.linalg.norm(nrm), V[i], nrm / np.linalg.norm(nrm)))
        # the best-aligned one that the rule itself classifies as designed, well inside the feature (a pointed vertex, a sharp edge, a
        # face with room around its centroid)
        for _, p, nrm in sorted(cands, key=lambda c: -c[0]):
            ball = _approach(rb, b, rb[b, 0:3] + Rw @ p, Rw @ nrm, gap, speed)
            hr = hull_rule(rb, ctx["model"], b, ball)
            if not hr["inside"] and hr["feature"] == feature and hr["feature_slack"] >= 5 * MARGIN and hr["feature_weight"] >= 0.2 and abs(hr["gap"] - gap) < 1e-6:
                return ball
        raise AssertionError("no such feature")
    return make


def launch_inside(b, where):
    """Centre inside the hull of link b: at the hull's centroid, or at the centre of its bounding box."""
    def make(ctx):
        rb = ctx["rb"]
        V = hull_of(ctx["model"], b)
        Rw = Rotation.from_quat(rb[b, 3:7]).as_matrix()
        p = rb[b, 0:3] + Rw @ (V.mean(0) if where == "centroid" else 0.5 * (V.min(0) + V.max(0)))
        return _ball(p, _link_vel_at(rb, b, p) + np.array([0.2, 0.1, -0.1]))
    return make


def launch_far(ctx):
    return _ball(ctx["rb"][0, 0:3] + np.array([2.5, 1.0, 0.5]), np.array([-8.0, 1.0, 2.0]))


def launch_search(want, region, seed, speed=8.0, toward=11):
    """Seeded search around the links `region` for a launch that `want(classification)` accepts with every decision MARGIN away from
    flipping; the ball flies at `speed` towards the origin of link `toward`."""
    def make(ctx):
        rb, model, geom = ctx["rb"], ctx["model"], ctx["geom"]
        rng = np.random.default_rng(seed)
        for _ in range(4000):
            b = int(rng.choice(region))
            p = rb[b, 0:3] + rng.uniform(-0.22, 0.22, 3)
            d = rb[toward, 0:3] - p
            ball = _ball(p, rb[toward, 7:10] + speed * d / max(np.linalg.norm(d), 1e-9))
            cl = classify(rb, model, geom, ball)
            if want(cl) and decisive_margin(cl) >= 2 * MARGIN and not any(c["row"] for c in cl["cyl"]):
                return ball
        raise AssertionError("no launch found")
    return make


def _count_is(k):
    return lambda cl: (len(cl["cand"]) == k if k < 4 else len(cl["cand"]) >= 4) and not any(hr["inside"] for hr in cl["hulls"].values())


def _three_loaded(cl):  # exactly three candidates, all within the contact offset and closing: the third one carries load at once
    hs = [cl["hulls"][b] for b in cl["cand"]]
    return _count_is(3)(cl) and all(h["gap"] < COFF - MARGIN and h["vrel"] < -1.0 for h in hs)


def _near_miss(cl):  # inside a box's reach, yet no hull within the activation threshold
    return len(cl["cand"]) == 0 and len(cl["boxes"]) >= 1


# name -> (launch, expectation).  Expectation keys: cyl = {j: region} rows expected of the cylinders (every other one: no row);
# hull = (link, feature) the designed feature; count = hull candidates (">=4": at least four); inside = link whose hull holds the centre;
# free = no row at all; boxes = at least one / no bounding box in reach; in racket hull = the hull of the racket's link holds the centre;
# hand only = the hand (the racket link's child) is the one hull candidate
CASES = {
    "head face+": (launch_cyl("face+"), {"cyl": {1: "face+"}, "count": 0}),
    "head face-": (launch_cyl("face-"), {"cyl": {1: "face-"}, "count": 0}),
    "head side": (launch_cyl("side"), {"cyl": {1: "side"}, "count": 0}),
    "head rim": (launch_cyl("rim"), {"cyl": {1: "rim+"}, "count": 0}),
    "head inside+": (launch_cyl("inside+"), {"cyl": {1: "inside+"}, "count": 0}),
    "head inside-": (launch_cyl("inside-"), {"cyl": {1: "inside-"}, "count": 0}),
    "handle side": (launch_cyl("handle side"), {"cyl": {0: "side"}}),
    "handle cap": (launch_cyl("handle cap"), {"cyl": {0: "face-"}}),
    "throat": (launch_cyl("throat"), {"cyl": {0: "side", 1: "rim+"}}),
    "racket link": (launch_cyl("racket link"), {"cyl": {0: "side"}, "in racket hull": True, "hand only": True}),
    "racket spec closing": (launch_cyl("spec closing"), {"cyl": {1: "face+"}, "count": 0, "speculative": True}),
    "racket spec receding": (launch_cyl("spec receding"), {"cyl": {}, "count": 0, "free": True}),
    "toe vertex below": (launch_hull(4, 1, [0.3, 0, -1]), {"cyl": {}, "hull": (4, 1)}),
    "toe edge above": (launch_hull(4, 2, [0.5, 0, 1]), {"cyl": {}, "hull": (4, 2)}),
    "toe face front": (launch_hull(4, 3, [1, 0.3, 0.2]), {"cyl": {}, "hull": (4, 3)}),
    "chest vertex": (launch_hull(11, 1, [1, 0.2, 0]), {"cyl": {}, "hull": (11, 1)}),
    "chest edge back": (launch_hull(11, 2, [-1, 0, 0]), {"cyl": {}, "hull": (11, 2)}),
    "chest face": (launch_hull(11, 3, [1, 0, 0]), {"cyl": {}, "hull": (11, 3)}),
    "head vertex above": (launch_hull(13, 1, [0, 0, 1]), {"cyl": {}, "hull": (13, 1)}),
    "head edge": (launch_hull(13, 2, [1, 0, 0.3]), {"cyl": {}, "hull": (13, 2)}),
    "head face back": (launch_hull(13, 3, [-1, 0, 0.2]), {"cyl": {}, "hull": (13, 3)}),
    "shin face front": (launch_hull(2, 3, [1, 0, 0]), {"cyl": {}, "hull": (2, 3)}),
    "inside shin": (launch_inside(2, "centroid"), {"cyl": {}, "inside": 2}),
    "box centre": (launch_inside(6, "box"), {"cyl": {}, "inside": 6, "at centre": True}),
    "near miss": (launch_search(_near_miss, [1, 5, 2, 6, 16, 21], 1), {"cyl": {}, "count": 0, "free": True, "boxes": True}),
    "far": (launch_far, {"cyl": {}, "count": 0, "free": True, "boxes": False}),
    "count 1": (launch_search(_count_is(1), [2, 6, 1, 5], 2, toward=2), {"cyl": {}, "count": 1}),
    "count 2": (launch_search(_count_is(2), [2, 6, 12, 15], 3, toward=12), {"cyl": {}, "count": 2}),
    "count 3": (launch_search(_three_loaded, [11, 12, 14, 19, 13, 10], 4), {"cyl": {}, "count": 3}),
    "count 4": (launch_search(_count_is(4), [11, 12, 14, 15], 5), {"cyl": {}, "count": ">=4"}),
    "hull spec closing": (launch_hull(11, 3, [1, 0, 0], gap=0.06, speed=10.0), {"cyl": {}, "hull": (11, 3), "speculative": True}),
    "hull spec receding": (launch_hull(11, 3, [1, 0, 0], gap=0.06, speed=-10.0), {"cyl": {}, "count": 0, "free": True}),
}

# envs 2w and 2w + 1 share wave w (pairing by load off).  Env 0: a hull case - next to "far" (no ball contact at all) in the batch of 3,
# next to "count 3" in the batch of 34.  Waves with hull candidates in both envs (chest vertex | count 3, count 1 | count 2 ...), in one
# env only (far | toe vertex, near miss | inside shin: lower and upper half), a cylinder case next to a hull case (head rim | chest face).
BATCH_3 = ["chest vertex", "far", "count 4"]
BATCH_34 = ["chest vertex", "count 3", "head face+", "head face-", "far", "toe vertex below", "head rim", "chest face", "count 1", "count 2",
            "head side", "head inside+", "inside shin", "near miss", "head inside-", "handle side", "count 4", "racket spec receding",
            "handle cap", "throat", "racket link", "toe edge above", "racket spec closing", "hull spec closing", "hull spec receding", "toe face front",
            "chest edge back", "head vertex above", "head edge", "head face back", "box centre", "shin face front", "far", "count 4"]
BATCH_CYL = ["head face+", "head face-", "head side", "head rim", "head inside+", "head inside-", "handle side", "handle cap", "throat", "racket link",
             "racket spec closing", "racket spec receding"]  # the cylinder group, for the left-handed player
BATCHES = {3: BATCH_3, 34: BATCH_34, 12: BATCH_CYL}


@functools.lru_cache(maxsize=None)
def env_of(case, player):
    """Everything about one env that does not depend on the solver: state, launch, classification."""
    model, geom = models(player)
    launch, expect = CASES[case]
    state = state_of(case)
    o = oracle_for(player, "pgs", state)
    rb = o.get_state()[3]
    ball = launch({"rb": rb, "model": model, "geom": geom, "player": player})
    cl = classify(rb, model, geom, ball, want_feature=(expect["hull"][0],) if "hull" in expect else ())
    return {"case": case, "player": player, "state": state, "rb": rb, "ball": ball, "cl": cl, "expect": expect}
