// The counter-based random generator of the controller's kernels: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers:
// as easy as 1, 2, 3", SC 2011; the Random123 known answers are in tests/test_device_rng.py) and the laws that turn its 32-bit words into
// values.  Stated once here and once in numpy (vid2player3d_amd/device_rng.py); callable from device and host code, so a plain C++
// program can print what a kernel draws.
//
// A draw depends on (seed, call, env, block) alone, not on which other envs draw in the same launch:
//     key     = (seed_lo, seed_hi)
//     counter = (env, block | stream << 28, call_lo, call_hi)
// `stream` keeps the uses apart (the random walk of pre_physics_step, the task reset, the start of a reset player, the serve of a reset pair), `call` is the host's count of launches of that use
// and `block` numbers the four-word outputs of one env in one call (below 2^28).  env = PHILOX_WHOLE_CALL is the one draw that all envs
// of a call share.
//
// The laws (w, w0, w1: words):
//     uniform in [0, 1)      u = (w >> 8) * 2^-24                                  (exact in float32)
//     integer in [lo, hi)    lo + ((uint64)w * (hi - lo) >> 32)                    (w = 0 -> lo, w = 2^32 - 1 -> hi - 1)
//     normal pair            u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (w1 >> 8) * 2^-24,  r = sqrt(-2 ln u1),
//                            (r cos 2 pi u2, r sin 2 pi u2)                        (Box-Muller; |z| <= sqrt(48 ln 2) = 5.77)
// with precise logf, sqrtf, sincosf.  A unit that includes this file is built without FMA contraction and without fast-math, as
// tennis_task.hip is: the products and the sum-free chain above then round the same way wherever they are compiled.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PHILOX_HD __host__ __device__ inline
#else
#define PHILOX_HD inline
#endif

namespace v2p {

constexpr uint32_t PHILOX_STREAM_WALK = 0, PHILOX_STREAM_RESET = 1, PHILOX_STREAM_ROOT = 2, PHILOX_STREAM_SERVE = 3;
constexpr uint32_t PHILOX_WHOLE_CALL = 0xffffffffu;
constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10 of counter c[4] under key k[2] into out[4]
PHILOX_HD void philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of (seed, call, stream, env, block)
PHILOX_HD void philox_block(uint64_t seed, uint64_t call, uint32_t stream, uint32_t env, uint32_t block, uint32_t out[4]) {
    const uint32_t c[4] = {env, block | (stream << 28), (uint32_t)call, (uint32_t)(call >> 32)};
    const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    philox4x32_10(c, k, out);
}

PHILOX_HD float philox_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }

PHILOX_HD int64_t philox_integer(uint32_t w, int64_t lo, int64_t hi) { return lo + (int64_t)(((uint64_t)w * (uint64_t)(hi - lo)) >> 32); }

PHILOX_HD void philox_normal_pair(uint32_t w0, uint32_t w1, float* z0, float* z1) {
    const float u1 = (float)((w0 >> 8) + 1u) * 5.9604644775390625e-8f, u2 = (float)(w1 >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    *z0 = r * c;
    *z1 = r * s;
}

// torch.clamp(z, -bound, bound)
PHILOX_HD float philox_clamp(float z, float bound) { return z < -bound ? -bound : (z > bound ? bound : z); }

}  // namespace v2p
