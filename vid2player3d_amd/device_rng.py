"""The numpy statement of csrc/philox.hpp: Philox4x32-10 and the laws that turn its words into values.

The controller's kernels draw their random numbers themselves, from a counter: key = (seed_lo, seed_hi), counter = (env, block |
stream << 28, call_lo, call_hi).  A draw depends on (seed, call, env, block) alone - not on which other envs draw in the same launch -
so a launch needs no host read and no compaction.  `philox_words` gives the words a kernel sees; the laws below are the header's, on
arrays.  The product never calls this module on its hot path: it is the checker of the tests and the tools.

    uniform in [0, 1)     u = (w >> 8) * 2^-24
    integer in [lo, hi)   lo + ((uint64)w * (hi - lo) >> 32)
    normal pair           u1 = ((w0 >> 8) + 1) * 2^-24, u2 = (w1 >> 8) * 2^-24, r = sqrt(-2 ln u1): (r cos 2 pi u2, r sin 2 pi u2)
"""
import math

import numpy as np

STREAM_WALK, STREAM_RESET, STREAM_ROOT, STREAM_SERVE = 0, 1, 2, 3
ROOT_XY_SCALE, ROOT_XY_OFFSET = (2.0, 1.5), (0.0, -13.0)  # `draw_root_xy` (mvae_player.py:230-236): the start of a reset player near the baseline's centre
SERVE_VEL_SCALE, SERVE_VEL_OFFSET = (4.0, 4.0, 3.0), (-2.0, 28.0, 5.0)  # `_reset_balls` (humanoid_smpl_im_mvae_dual.py:61-63): the velocity of a serve
WHOLE_CALL = 0xFFFFFFFF
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
LARGEST_NORMAL = math.sqrt(48.0 * math.log(2.0))  # u1 = 2^-24: 5.768
_u32, _u64 = np.uint32, np.uint64
_MASK = _u64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """Philox4x32 of counters [..., 4] under keys [..., 2] (uint32, broadcast against each other): words [..., 4] uint32."""
    c = np.asarray(counter, dtype=_u64)
    k = np.asarray(key, dtype=_u64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0, p1 = _u64(M0) * c0, _u64(M1) * c2  # (both factors below 2^32: the product fits 64 bits)
        c0, c1, c2, c3 = (p1 >> _u64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> _u64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _u64(W0)) & _MASK, (k1 + _u64(W1)) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(_u32)


def philox_words(seed, call, stream, n, blocks, envs=None):
    """The words of envs 0 .. n-1 (or of `envs`, e.g. [WHOLE_CALL]) in call `call` of `stream` under `seed`: [n, 4 * blocks] uint32, word
    4b + j = word j of block b."""
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    env = np.arange(n, dtype=_u64) if envs is None else np.asarray(envs, dtype=_u64)
    if not 0 <= int(stream) < 16 or not 0 <= int(blocks) <= 2 ** 28:
        raise ValueError("philox_words: stream %r outside 0..15 or blocks %r outside 0..2^28" % (stream, blocks))
    counter = np.zeros((len(env), int(blocks), 4), dtype=_u64)
    counter[..., 0] = env[:, None]
    counter[..., 1] = np.arange(int(blocks), dtype=_u64)[None] | _u64(int(stream) << 28)
    counter[..., 2], counter[..., 3] = call & 0xFFFFFFFF, call >> 32
    return philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=_u64)).reshape(len(env), 4 * int(blocks))


def uniform(words, dt=np.float32):
    return (np.asarray(words, dtype=_u32) >> _u32(8)).astype(dt) * dt(2.0 ** -24)


def integer(words, lo, hi):
    """lo + ((uint64)w * (hi - lo) >> 32), int64"""
    if not 0 < int(hi) - int(lo) <= 2 ** 32:
        raise ValueError("integer: [%r, %r) is empty or wider than 2^32" % (lo, hi))
    return np.int64(lo) + ((np.asarray(words, dtype=_u64) * _u64(int(hi) - int(lo))) >> _u64(32)).astype(np.int64)


def normals(words, dt=np.float32):
    """Box-Muller on consecutive word pairs of the last axis (even length): element 2p is r cos, 2p+1 is r sin of words 2p, 2p+1.  With
    dt float32 every operation is float32, the header's order; float64 is the same law in double."""
    w = np.asarray(words, dtype=_u32)
    if w.shape[-1] % 2:
        raise ValueError("normals: an odd number of words")
    u1 = ((w[..., 0::2] >> _u32(8)) + _u32(1)).astype(dt) * dt(2.0 ** -24)
    u2 = (w[..., 1::2] >> _u32(8)).astype(dt) * dt(2.0 ** -24)
    r = np.sqrt(dt(-2.0) * np.log(u1))
    angle = dt(6.283185307179586) * u2
    out = np.empty(w.shape, dtype=dt)
    out[..., 0::2], out[..., 1::2] = r * np.cos(angle), r * np.sin(angle)
    return out


def clamped_normals(words, bound, dt=np.float32):
    """torch.clamp(normals, -bound, bound)"""
    return np.clip(normals(words, dt), dt(-bound), dt(bound))


def root_xy_reference(seed, call, n, envs=None):
    """The start [n,2] float32 that `v2p_mvae_reset_flagged` draws for envs 0 .. n-1 (or `envs`) in call `call` under `seed`:
    x = (u0 - 0.5) * 2 + 0, y = (u1 - 0.5) * 1.5 + (-13) in float32, every operation rounded on its own, u0 and u1 the uniforms of words 0
    and 1 of block 0 of STREAM_ROOT.  A draw depends on (seed, call, env) alone."""
    f = np.float32
    u = uniform(philox_words(seed, call, STREAM_ROOT, n, 1, envs)[:, :2])
    return ((u - f(0.5)) * np.array(ROOT_XY_SCALE, f) + np.array(ROOT_XY_OFFSET, f)).astype(f)


def serve_vel_reference(seed, call, n, envs=None):
    """The serve velocity [n,3] float32 that `v2p_tennis_dual_serve_flagged` draws for the balls of envs 0 .. n-1 (or `envs`: the servers'
    env ids) in call `call` under `seed`: u * (4, 4, 3) + (-2, 28, 5) in float32, the product and the sum each rounded on its own, u the
    uniforms of words 0..2 of block 0 of STREAM_SERVE.  A draw depends on (seed, call, the server's env id) alone."""
    f = np.float32
    u = uniform(philox_words(seed, call, STREAM_SERVE, n, 1, envs)[:, :3])
    return (u * np.array(SERVE_VEL_SCALE, f) + np.array(SERVE_VEL_OFFSET, f)).astype(f)
