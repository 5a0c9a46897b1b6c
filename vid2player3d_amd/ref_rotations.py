"""The rotation conversions of the reference (utils/konia_transform.py, utils/torch_transform.py) on numpy arrays: the one statement
the checkers of the motion generator (`mvae`) and of the imitation target (`mvae_target`) are built from, as csrc/ref_rotations.hpp is
for the kernels.  dt = numpy.float64 evaluates the same statement in double precision.  The product never calls them.

probes (a dict, or None) receives the floats that pick a branch, raw and full length: every call appends one raveled array per name,
    rot6d_norm                       rot6d_to_rotmat: the two norms compared with 1e-8 (two arrays per call)
    trace, diag01, diag02, diag12    rotmat_to_quat: m00 + m11 + m22 and m00 - m11, m00 - m22, m11 - m22, all compared with 0
    branch                           rotmat_to_quat: the branch taken, 0 .. 3
    quat_w, sin2                     quat_to_angle_axis: w and x^2 + y^2 + z^2, compared with 0
    theta2                           angle_axis_to_rotmat: compared with 1e-6
Which of them decide where (a difference of the diagonal only where the trace does not) is the business of whoever asserts on them."""
import numpy as np


def _record(probes, **values):
    if probes is not None:
        for k, v in values.items():
            probes.setdefault(k, []).append(np.ravel(v))


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def szd(num, den, dt):
    """safe_zero_division (utils/konia_transform.py:336-344)"""
    den = np.where(np.abs(den) < dt(1e-6), den + dt(1e-6), den)
    return num / den


def rot6d_to_rotmat_reference(r6, dt=np.float32, probes=None):
    """rot6d_to_rotmat (utils/torch_transform.py:221-235): [..., 6] -> [..., 3, 3], columns b1 b2 b3."""
    r6 = np.asarray(r6, dtype=dt)
    a1, a2 = r6[..., :3].copy(), r6[..., 3:].copy()
    small = _norm(a1) < dt(1e-8)
    _record(probes, rot6d_norm=_norm(a1))
    a1[small] = np.array([1, 0, 0], dt)
    b1 = a1 / np.maximum(_norm(a1), dt(1e-9))[..., None]
    u = a2 - (b1 * a2).sum(-1)[..., None] * b1
    b2 = u / np.maximum(_norm(u), dt(1e-9))[..., None]
    small = _norm(b2) < dt(1e-8)
    _record(probes, rot6d_norm=_norm(u))
    b2[small] = np.array([0, 1, 0], dt)
    return np.stack([b1, b2, np.cross(b1, b2)], -1)


def rotmat_to_quat_reference(m, dt=np.float32, probes=None):
    """rotation_matrix_to_quaternion (utils/konia_transform.py:347-438): [..., 3, 3] -> [..., 4] (w, x, y, z)."""
    m = np.asarray(m, dtype=dt)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., i, j] for i in range(3) for j in range(3)]
    one, two, eps = dt(1), dt(2), dt(1e-6)
    trace = m00 + m11 + m22
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(np.maximum(trace + one, eps)) * two
        c0 = np.stack([dt(0.25) * sq, szd(m21 - m12, sq, dt), szd(m02 - m20, sq, dt), szd(m10 - m01, sq, dt)], -1)
        sq = np.sqrt(np.maximum(one + m00 - m11 - m22, eps)) * two
        c1 = np.stack([szd(m21 - m12, sq, dt), dt(0.25) * sq, szd(m01 + m10, sq, dt), szd(m02 + m20, sq, dt)], -1)
        sq = np.sqrt(np.maximum(one + m11 - m00 - m22, eps)) * two
        c2 = np.stack([szd(m02 - m20, sq, dt), szd(m01 + m10, sq, dt), dt(0.25) * sq, szd(m12 + m21, sq, dt)], -1)
        sq = np.sqrt(np.maximum(one + m22 - m00 - m11, eps)) * two
        c3 = np.stack([szd(m10 - m01, sq, dt), szd(m02 + m20, sq, dt), szd(m12 + m21, sq, dt), dt(0.25) * sq], -1)
        b1, b2 = (m00 > m11) & (m00 > m22), m11 > m22
        q = np.where((trace > 0)[..., None], c0, np.where(b1[..., None], c1, np.where(b2[..., None], c2, c3)))
        _record(probes, trace=trace, diag01=m00 - m11, diag02=m00 - m22, diag12=m11 - m22, branch=np.where(trace > 0, 0, np.where(b1, 1, np.where(b2, 2, 3))))
    return q.astype(dt)


def quat_to_angle_axis_reference(q, dt=np.float32, probes=None, wide_atan2=False):
    """quaternion_to_angle_axis (utils/konia_transform.py:557-628) of (w, x, y, z).  wide_atan2: the one arctangent is evaluated in float64
    and rounded once to dt - the correctly rounded value for all but one argument in some 2^29, which no float32 library promises and
    which a kernel that does the same reproduces bit for bit (csrc/tennis_eval.hip)."""
    q = np.asarray(q, dtype=dt)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two, eps = dt(2), dt(1e-6)
    with np.errstate(invalid="ignore", divide="ignore"):
        s2 = x * x + y * y + z * z
        s = np.sqrt(np.maximum(s2, eps))
        at = (lambda y, x: np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(dt)) if wide_atan2 else np.arctan2
        two_theta = two * np.where(w < 0, at(-s, -w), at(s, w))  # (s >= 1e-3: torch_safe_atan2 never shifts)
        k = np.where(s2 > 0, szd(two_theta, s, dt), two)
    _record(probes, quat_w=w, sin2=s2)
    return (q[..., 1:] * k[..., None]).astype(dt)


def rotmat_to_angle_axis_reference(m, dt=np.float32, probes=None, wide_atan2=False):
    """rotation_matrix_to_angle_axis (utils/konia_transform.py:631-655, through the wxyz quaternion): [..., 3, 3] -> [..., 3].
    wide_atan2: as quat_to_angle_axis_reference's."""
    return quat_to_angle_axis_reference(rotmat_to_quat_reference(m, dt, probes), dt, probes, wide_atan2)


def angle_axis_to_rotmat_reference(aa, dt=np.float32, probes=None, wide_trig=False):
    """angle_axis_to_rotation_matrix (utils/konia_transform.py:282-333): [..., 3] -> [..., 3, 3].  wide_trig: sine and cosine are
    evaluated in float64 and rounded once to dt, as wide_atan2 does for the arctangent - what a kernel that does the same reproduces bit
    for bit (csrc/two_hand_fix.hip)."""
    aa = np.asarray(aa, dtype=dt)
    rx, ry, rz = aa[..., 0], aa[..., 1], aa[..., 2]
    theta2 = rx * rx + ry * ry + rz * rz
    eps, one = dt(1e-6), dt(1)
    theta = np.sqrt(np.maximum(theta2, eps))
    wx, wy, wz = rx / (theta + eps), ry / (theta + eps), rz / (theta + eps)
    if wide_trig:
        c, s = np.cos(theta.astype(np.float64)).astype(dt), np.sin(theta.astype(np.float64)).astype(dt)
    else:
        c, s = np.cos(theta), np.sin(theta)
    t = one - c
    normal = np.stack([c + wx * wx * t, wx * wy * t - wz * s, wy * s + wx * wz * t, wz * s + wx * wy * t, c + wy * wy * t, -wx * s + wy * wz * t,
                       -wy * s + wx * wz * t, wx * s + wy * wz * t, c + wz * wz * t], -1)
    o = np.ones_like(rx)
    taylor = np.stack([o, -rz, ry, rz, o, -rx, -ry, rx, o], -1)
    _record(probes, theta2=theta2)
    return np.where((theta2 > eps)[..., None], normal, taylor).reshape(aa.shape[:-1] + (3, 3)).astype(dt)
