// The two-player controller's reset of finished pairs, driven by flags (`PhysicsMVAEControllerDual._reset_envs`,
// physics_mvae_controller_dual.py:22-66, with `HumanoidSMPLIMMVAEDual._reset_balls`, humanoid_smpl_im_mvae_dual.py:52-63, for the pairs
// whose `reset_buf` is up): every launch runs over envs 0 .. n-1 and a pair neither of whose flags is up keeps every bit.  No id list is
// read, so the host needs no `nonzero()` of a device result to queue them.  The whole reset:
//
//   v2p_ctl_pair_reset_begin         the mask made whole, `_reset_env_tensors`, `_num_reset += 1`, the pair's reaction / recovery flags
//   v2p_mvae_dual_reset_flagged      the generator's ready / serve frames (mvae_player_dual_flagged.hip; `dual_mode: True`:
//                                    v2p_mvae_reset_flagged on the per-env table)
//   v2p_mvae_target_reset_flagged    `_reset_actors` + `_set_env_state` (flag_reset.hip)
//   v2p_env_push_state_flagged       the exposed state goes into the engine (flag_reset.hip)
//   v2p_tennis_dual_serve_flagged    `_reset_balls`: the ball at the server's racket head, with the serve's spin and velocity
//   v2p_tennis_dual_handover         the serve becomes the receiver's incoming ball (tennis_task.hip, by the two flags begin wrote)
//   v2p_ctl_pair_reset_end           the mask
//
// Envs 2k and 2k+1 are a pair; one thread owns both of a pair's words wherever a pair's flag is written, so nothing races.  The
// receiver of a pair is its even env with serve_from near (V2P_SERVE_FROM_NEAR) and its odd env with far; the server is the other.
//
// The serve velocity restates torch's `u * (4, 4, 3) + (-2, 28, 5)` in float32, the product and the sum each rounded on its own (the
// unit is built without FMA contraction): u = row (server >> 1) of the caller's table, or philox_uniform of words 0..2 of block 0 of
// stream PHILOX_STREAM_SERVE under (seed, call, the server's env id) - device_rng.serve_vel_reference is the numpy statement.
#include "pair_reset.hpp"
#include "philox.hpp"

namespace v2p {

namespace {

constexpr int PR_BLOCK = 256;

// one thread per pair
__global__ __launch_bounds__(PR_BLOCK) void ctl_pair_reset_begin_kernel(int64_t pairs, int64_t* __restrict__ flags, const v2p_ctl_reset_buffers b, int receiver_side) {
    const int64_t p = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
    if (p >= pairs) return;
    const int64_t f0 = flags[2 * p], f1 = flags[2 * p + 1];
    if (f0 == 0 && f1 == 0) return;
    // a half-flagged pair is made whole: the per-env launches that follow read a whole mask
    if (f0 == 0) flags[2 * p] = 1;
    if (f1 == 0) flags[2 * p + 1] = 1;
    for (int k = 0; k < 2; ++k) {
        const int64_t e = 2 * p + k;
        const bool receiver = k == receiver_side;
        b.progress[e] = 0;
        b.terminate[e] = 0;
        b.num_reset_reaction[e] = 0;
        b.distance[e] = 0.f;
        b.num_reset[e] = b.num_reset[e] + 1;
        b.reset_reaction[e] = receiver ? 1 : 0;
        b.reset_recovery[e] = receiver ? 0 : 1;
    }
}

// one thread per pair: the ball of the pair's server
__global__ __launch_bounds__(PR_BLOCK) void tennis_dual_serve_flagged_kernel(int64_t pairs, const int64_t* __restrict__ flags, int receiver_side,
                                                                             const float* __restrict__ racket_pos, float* __restrict__ ball_state,
                                                                             const float* __restrict__ draws, const v2p_serve_rule rule) {
    const int64_t p = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
    if (p >= pairs) return;
    if (flags[2 * p] == 0 && flags[2 * p + 1] == 0) return;
    const int64_t s = 2 * p + (1 - receiver_side);
    float u[3];
    if (draws) {
        for (int k = 0; k < 3; ++k) u[k] = draws[p * 3 + k];
    } else {
        uint32_t words[4];
        philox_block(rule.seed, rule.call, PHILOX_STREAM_SERVE, (uint32_t)s, 0, words);
        for (int k = 0; k < 3; ++k) u[k] = philox_uniform(words[k]);
    }
    float* ball = ball_state + s * 13;
    for (int k = 0; k < 3; ++k) ball[k] = racket_pos[s * 3 + k];
    ball[7] = u[0] * 4.0f + (-2.0f);
    ball[8] = u[1] * 4.0f + 28.0f;
    ball[9] = u[2] * 3.0f + 5.0f;
    ball[10] = -40.0f;
    ball[11] = 0.0f;
    ball[12] = 0.0f;
}

// one thread per env: the mask and nothing else (the reaction and recovery flags stay up, as after the id-list reset)
__global__ __launch_bounds__(PR_BLOCK) void ctl_pair_reset_end_kernel(int64_t n, int64_t* __restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
    if (e >= n) return;
    if (flags[e] == 0) return;
    flags[e] = 0;
}

unsigned blocks_of(int64_t count) { return (unsigned)((count + PR_BLOCK - 1) / PR_BLOCK); }

}  // namespace

int launch_ctl_pair_reset_begin(int64_t n, int64_t* flags, const v2p_ctl_reset_buffers& b, int serve_from, hipStream_t s) {
    const int receiver_side = serve_from == V2P_SERVE_FROM_NEAR ? 0 : 1;
    hipLaunchKernelGGL(ctl_pair_reset_begin_kernel, dim3(blocks_of(n / 2)), dim3(PR_BLOCK), 0, s, n / 2, flags, b, receiver_side);
    return check_hip(hipGetLastError(), "ctl_pair_reset_begin_kernel");
}

int launch_tennis_dual_serve_flagged(int64_t n, const int64_t* flags, int serve_from, const float* racket_pos, float* ball_state, const float* draws,
                                     const v2p_serve_rule& rule, hipStream_t s) {
    const int receiver_side = serve_from == V2P_SERVE_FROM_NEAR ? 0 : 1;
    hipLaunchKernelGGL(tennis_dual_serve_flagged_kernel, dim3(blocks_of(n / 2)), dim3(PR_BLOCK), 0, s, n / 2, flags, receiver_side, racket_pos, ball_state, draws, rule);
    return check_hip(hipGetLastError(), "tennis_dual_serve_flagged_kernel");
}

int launch_ctl_pair_reset_end(int64_t n, int64_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(ctl_pair_reset_end_kernel, dim3(blocks_of(n)), dim3(PR_BLOCK), 0, s, n, flags);
    return check_hip(hipGetLastError(), "ctl_pair_reset_end_kernel");
}

}  // namespace v2p
