// The flag-driven half of the single-player controller's `_reset_envs` (vid2player/env/tasks/physics_mvae_controller.py:167-242) in one
// launch over all envs: the ball draw of `_reset_balls` (humanoid_smpl_im_mvae.py:503-524) from the offline pool
// (TennisBallGeneratorOffline.generate, utils/tennis_ball.py:422-456), `_reset_recovery_tasks`, `_reset_reaction_tasks` and the
// observation of the flagged envs.  rl_games calls env.reset(done_ids) after every step, so this runs every control step; as torch code
// it is three nonzero() host reads and some 35 indexed launches.
//
// One wave64 per env, four envs per workgroup, as the task step: the per-env scalar work is uniform over the wave and stored by lane 0,
// the lanes stride the trajectory row, the history fill and the observation's columns.  A wave whose env has neither flag returns at
// once.  The random numbers are csrc/philox.hpp's: a draw depends on (seed, call, env) alone, so nothing has to be counted or compacted.
//
// A translation unit of its own: tennis_task.hip's kernels stay the machine code they were (tools/kernel_identity.py).  The observation
// row is the TEXT of tennis_row.inc, included as the step kernel includes it; what that text leans on of tennis_task.hip's anonymous
// namespace (the row's width, tt_rot6d, the three constants) is said again below, to the letter.
//
// Built without FMA contraction like tennis_task.hip: the arithmetic restates torch elementwise float32 code.
#include "philox.hpp"
#include "ref_rotations.hpp"
#include "tennis_reset.hpp"

namespace v2p {

namespace {

constexpr int TT_WAVE = 64;
constexpr int TT_WPB = 4;  // waves (envs) per workgroup
constexpr int TT_ACTOR = V2P_TENNIS_ACTOR_OBS;
constexpr int TT_FRAMES = V2P_TENNIS_TRAJ_FRAMES;
constexpr int TR_ROW_ITERS = (TT_FRAMES * 3 + TT_WAVE - 1) / TT_WAVE;  // passes of a wave over a ball_traj row

struct TennisResetArgs {
    v2p_tennis_cfg c;
    v2p_tennis_buffers b;
    v2p_tennis_reset_cfg rc;
    v2p_tennis_reset_buffers r;
    int64_t n;
    int width;  // floats of an observation row
};

// tennis_task.hip's tt_rot6d: column k of quat_to_rot6d on the (x, y, z, w) numbers read as (w, x, y, z)
__device__ inline float tt_rot6d(const float* q4, int k) {
    const float n = ref_clamp_min(sqrtf(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]), 1e-12f);
    const float w = q4[0] / n, x = q4[1] / n, y = q4[2] / n, z = q4[3] / n;
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
    switch (k) {
        case 0: return 1.f - (ty * y + tz * z);
        case 1: return ty * x + tz * w;
        case 2: return tz * x - ty * w;
        case 3: return ty * x - tz * w;
        case 4: return 1.f - (tx * x + tz * z);
        default: return tz * y + tx * w;
    }
}

__global__ __launch_bounds__(TT_WAVE* TT_WPB) void tennis_reset_kernel(const TennisResetArgs a) {
    const int lane = threadIdx.x & (TT_WAVE - 1);
    const int64_t e = (int64_t)blockIdx.x * TT_WPB + (threadIdx.x >> 6);
    if (e >= a.n) return;  // (the whole wave)
    const v2p_tennis_cfg& c = a.c;
    const v2p_tennis_buffers& b = a.b;
    const v2p_tennis_reset_cfg& rc = a.rc;
    const v2p_tennis_reset_buffers& r = a.r;
    const bool react = b.reset_reaction[e] != 0, recover = b.reset_recovery[e] != 0;
    if (!react && !recover) return;  // (the whole wave)
    const int L = c.obs_ball_traj_length;

    float bpos[3] = {r.ball_state[e * 13], r.ball_state[e * 13 + 1], r.ball_state[e * 13 + 2]};
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (react) {
        if (r.words) {
            for (int i = 0; i < 8; ++i) w[i] = r.words[e * 8 + i];
        } else {
            philox_block(rc.seed, rc.call, PHILOX_STREAM_RESET, (uint32_t)e, 0, w);
            if (rc.target_mode == V2P_TENNIS_TARGET_CONTINUOUS) philox_block(rc.seed, rc.call, PHILOX_STREAM_RESET, PHILOX_WHOLE_CALL, 0, w + 4);
        }
        // ---- the pool row (TennisBallGeneratorOffline.indices)
        int64_t idx;
        if (rc.pool_rule == V2P_TENNIS_POOL_ROUND_ROBIN) {
            idx = r.sample_idx[e];
            idx = idx < 0 ? 0 : (idx > rc.pool_rows - 1 ? rc.pool_rows - 1 : idx);  // (a stale counter must not index outside the pool)
        } else {
            idx = philox_integer(w[0], 0, rc.pool_rows);
            if (bpos[1] > 0.f) {
                // long((x + 4) / 8 * rows), float32; a value no int64 holds (NaN, inf) counts as far below: row 0 after the clamp
                const float nf = (bpos[0] + 4.f) / 8.f * (float)rc.pool_rows;
                const int64_t base = (nf >= -1e15f && nf <= 1e15f) ? (int64_t)nf : (int64_t)-1000000000000000ll;
                const int64_t near = base + philox_integer(w[1], -1000, 1000);
                idx = near < 0 ? 0 : (near > rc.pool_rows - 1 ? rc.pool_rows - 1 : near);
            }
        }
        const float* row = r.pool + idx * rc.pool_stride;
        // ---- the new trajectory row, read whole before it is written; zeros past the pool's frames
        float v[TR_ROW_ITERS];
#pragma unroll
        for (int k = 0; k < TR_ROW_ITERS; ++k) {
            const int i = k * TT_WAVE + lane;
            v[k] = (i < rc.pool_frames * 3) ? row[7 + i] : 0.f;
        }
        float* traj = r.ball_traj + e * (TT_FRAMES * 3);
#pragma unroll
        for (int k = 0; k < TR_ROW_ITERS; ++k) {
            const int i = k * TT_WAVE + lane;
            if (i < TT_FRAMES * 3) traj[i] = v[k];
        }
        // ---- reset_balls: the launch state; spin = vspin 2 pi normalize(vel x (0, 0, -1)) as torch evaluates it (:508-509)
        const float vel[3] = {row[3], row[4], row[5]}, vspin = row[6];
        const float c0 = vel[1] * -1.f - vel[2] * 0.f, c1 = vel[2] * 0.f - vel[0] * -1.f, c2 = vel[0] * 0.f - vel[1] * 0.f;
        const float nrm = ref_clamp_min(sqrtf(c0 * c0 + c1 * c1 + c2 * c2), 1e-12f);
        const float mag = vspin * 3.14159265358979323846f * 2.f;
        for (int i = 0; i < 3; ++i) bpos[i] = row[i];
        if (lane == 0) {
            if (rc.pool_rule == V2P_TENNIS_POOL_ROUND_ROBIN) r.sample_idx[e] = (idx + 1) % rc.pool_rows;
            float* s = r.ball_state + e * 13;
            for (int i = 0; i < 3; ++i) s[i] = row[i];
            s[3] = 0.f; s[4] = 0.f; s[5] = 0.f; s[6] = 1.f;
            for (int i = 0; i < 3; ++i) s[7 + i] = vel[i];
            s[10] = mag * (c0 / nrm);
            s[11] = mag * (c1 / nrm);
            s[12] = mag * (c2 / nrm);
            r.has_bounce[e] = 0;
            for (int i = 0; i < 3; ++i) r.bounce_pos[e * 3 + i] = 0.f;
            r.has_racket_contact[e] = 0;
            b.traj_cursor[e] = 0;
            b.prev_ball_vy[e] = vel[1];
        }
    }
    // ---- _reset_recovery_tasks (:242-245)
    if (recover && lane == 0) {
        r.tar_action[e] = 0;
        r.has_bounce[e] = 0;
        for (int i = 0; i < 3; ++i) r.bounce_pos[e * 3 + i] = 0.f;
    }
    // ---- _reset_reaction_tasks (:207-240); an env with both flags ends with tar_action = 1
    if (react) {
        if (c.use_history_ball_obs)
            for (int i = lane; i < 3 * L; i += TT_WAVE) b.ball_obs[e * (int64_t)(L * 3) + i] = bpos[i % 3];
        if (lane == 0) {
            b.tar_time[e] = 0;
            r.tar_action[e] = 1;
            r.num_reset_reaction[e] = r.num_reset_reaction[e] + 1;
            b.bounce_in[e] = 0;
            for (int i = 0; i < 3; ++i) b.est_bounce_pos[e * 3 + i] = 0.f;
            b.est_bounce_time[e] = 0.f;
            b.est_bounce_in[e] = 0;
            b.est_max_height[e] = 0.f;
            r.swing_type_cycle[e] = -1;
            r.tar_time_total[e] = rc.reset_reaction_nframes + philox_integer(w[2], -5, 5);
            if (rc.target_mode == V2P_TENNIS_TARGET_CONTINUOUS) {
                for (int i = 0; i < 3; ++i) r.target_bounce_pos[e * 3 + i] = philox_uniform(w[4 + i]) * (rc.target_max[i] - rc.target_min[i]) + rc.target_min[i];
            } else if (rc.target_mode == V2P_TENNIS_TARGET_DISCRETE) {
                const float u = philox_uniform(w[3]);
                r.target_bounce_pos[e * 3] = u < 0.33f ? -3.f : (u > 0.67f ? 3.f : 0.f);
                r.target_bounce_pos[e * 3 + 1] = 10.f;
                r.target_bounce_pos[e * 3 + 2] = 0.f;
            }
        }
    }
    // ---- _compute_observations(flagged envs): the row reads what other lanes of this wave have just written (window, cursor, history,
    // target), hence the fence
    __threadfence_block();
    const float* rb = b.rb_state + e * (V2P_NUM_BODIES * 13);
    const float* rk = b.racket_state + e * 13;
    const float root[3] = {rb[0], rb[1], rb[2]};
    const float rvel[3] = {b.root_states[e * 13 + 7], b.root_states[e * 13 + 8], b.root_states[e * 13 + 9]};
    const float rpos[3] = {rk[0], rk[1], rk[2]};
#define TT_ROW_RACKET_NORMAL
#define TT_ROW_GRIP(i) c.grip_normal[i]
#include "tennis_row.inc"
#undef TT_ROW_GRIP
#undef TT_ROW_RACKET_NORMAL
#define TT_ROW_OBSERVATION
#define TT_ROW_LANES TT_WAVE
#include "tennis_row.inc"
#undef TT_ROW_LANES
#undef TT_ROW_OBSERVATION
    (void)nan_seen;
    (void)cursor;
}

}  // namespace

int launch_tennis_task_reset(const v2p_tennis_cfg& c, const v2p_tennis_reset_cfg& rc, int64_t n, const v2p_tennis_buffers& b, const v2p_tennis_reset_buffers& r,
                             hipStream_t s) {
    TennisResetArgs a;
    a.c = c;
    a.b = b;
    a.rc = rc;
    a.r = r;
    a.n = n;
    a.width = TT_ACTOR + 3 * c.obs_ball_traj_length + (c.use_random_ball_target ? 2 : 0);
    const dim3 grid((unsigned)((n + TT_WPB - 1) / TT_WPB)), block(TT_WAVE * TT_WPB);
    hipLaunchKernelGGL(tennis_reset_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "tennis_reset_kernel");
}

}  // namespace v2p
