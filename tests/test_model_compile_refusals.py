"""The host-side compiler of a body model (csrc/model_compile.hip) refuses through v2p_model_create before any device call (no GPU):
each refusal with today's message and code."""
import ctypes

import numpy as np

from vid2player3d_amd import _lib
from vid2player3d_amd.model import load_baked_model

INVALID, UNSUPPORTED = -1, -2


def _create(**changed):
    L, m = _lib.load(), load_baked_model()
    f = dict(parents=m.parents, local_pos=m.local_pos, mass=m.mass, com=m.com, inertia=m.inertia, kp=m.kp, kd=m.kd, armature=m.armature,
             hull_offsets=m.hull_offsets, hull_verts=m.hull_verts, limit_lower=m.limit_lower, limit_upper=m.limit_upper)
    f.update(changed)
    keep = {k: np.ascontiguousarray(v, dtype=np.int32 if k in ("parents", "hull_offsets") else np.float32) for k, v in f.items()}
    d = _lib.ModelDesc(num_bodies=m.num_bodies, **{k: a.ctypes.data_as(_lib.c_i32 if a.dtype == np.int32 else _lib.c_f) for k, a in keep.items()})
    h = ctypes.c_void_p()
    rc = L.v2p_model_create(ctypes.byref(d), 0, ctypes.byref(h))
    assert rc != 0 and not h.value, "the model was not refused"
    return rc, L.v2p_last_error().decode()


def test_an_unordered_parent_is_refused():
    m = load_baked_model()
    parents = np.array(m.parents, dtype=np.int32)
    parents[3] = 5
    assert _create(parents=parents) == (INVALID, "v2p_model_create: parents must be topologically ordered with a single root (body 3 has parent 5)")


def test_per_axis_gains_are_refused():
    m = load_baked_model()
    kp = np.array(m.kp, dtype=np.float32).reshape(-1, 3).copy()
    kp[4, 1] += 1.0  # joint of body 5
    assert _create(kp=kp) == (UNSUPPORTED, "v2p_model_create: joint of body 5 has per-axis gains; only isotropic spherical-joint gains are built")


def test_an_empty_joint_range_is_refused():
    m = load_baked_model()
    lo = np.array(m.limit_lower, dtype=np.float32).reshape(-1, 3).copy()
    hi = np.array(m.limit_upper, dtype=np.float32).reshape(-1, 3)
    lo[6, 2] = hi[6, 2] + 0.5  # joint of body 7
    assert _create(limit_lower=lo) == (INVALID, "v2p_model_create: body 7: joint range is empty")


def test_more_than_64_hull_vertices_on_a_body_are_refused():
    m = load_baked_model()
    offs = np.array(m.hull_offsets, dtype=np.int32)
    verts = np.array(m.hull_verts, dtype=np.float32).reshape(-1, 3)
    extra = 65 - (offs[1] - offs[0])
    verts = np.concatenate([verts[:offs[1]], np.repeat(verts[offs[1] - 1:offs[1]], extra, axis=0), verts[offs[1]:]])
    offs[1:] += extra
    assert _create(hull_offsets=offs, hull_verts=verts) == (UNSUPPORTED, "v2p_model_create: body 0 has 65 hull vertices (1..64 supported)")
