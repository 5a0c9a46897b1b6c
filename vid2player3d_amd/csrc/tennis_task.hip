// The tennis controller's task step (vid2player/env/tasks/physics_mvae_controller.py, PhysicsMVAEController) in one launch:
// v2p_tennis_task_step = post_physics_step (:441-452) + the window roll of physics_step (:365-366), v2p_tennis_task_obs =
// _compute_observations(env_ids) at reset time (:198-199).
//
// One wave64 per env.  An observation row is 257 .. 527 floats: the lanes stride its columns, so the row's stores are coalesced and the
// NaN test of _compute_reset (:412) is one wave-wide vote.  The per-env scalar work (racket hit, bounce bookkeeping, estimator lookup,
// reward, flags; some 60 loads) is computed by every lane on the same addresses - uniform, the loads broadcast - and stored by lane 0.
// The estimator's two dependent gathers run only in the step an env's racket hits the ball.
//
// The arithmetic restates torch elementwise float32 code (built without FMA contraction like task_ops.hip): the same operations in the
// same order, scalars of the reference's Python code rounded to float32 where torch rounds them.
#include "tennis_task.hpp"

namespace v2p {

namespace {

constexpr int TT_WAVE = 64;
constexpr int TT_WPB = 4;  // waves (envs) per workgroup
constexpr int TT_ACTOR = V2P_TENNIS_ACTOR_OBS;
constexpr int TT_FRAMES = V2P_TENNIS_TRAJ_FRAMES;
constexpr float TT_NET_HEIGHT = 1.07f;  // utils/tennis_ball.py:20
// the court of the bounce tests (physics_mvae_controller.py:285-286)
constexpr float TT_COURT_X0 = -4.11f, TT_COURT_X1 = 4.11f, TT_COURT_Y0 = 0.f, TT_COURT_Y1 = 11.89f;

struct TennisArgs {
    v2p_tennis_cfg c;
    v2p_tennis_buffers b;
    const int64_t* env_ids;  // obs only
    int64_t rows, num_envs;
    int width;               // floats of an observation row
    // the grids as torch sees them: (lo, hi - step, step) of every range in float32, and the two strides of the table index
    float g_lo[5], g_top[5], g_step[5], vx_hi, vy_hi, ty_hi, dim1, dim2;
};

// x.clamp_min(lo) / torch.clamp as torch evaluates them: a NaN stays a NaN (fmaxf / fminf would drop it)
__device__ inline float tt_clamp_min(float x, float lo) { return x < lo ? lo : x; }
__device__ inline float tt_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// round((clamp(v, lo, hi - step) - lo) / step), float32, halves to even (torch.round)
__device__ inline float tt_index(const TennisArgs& a, int g, float v) {
    const float cl = tt_clamp(v, a.g_lo[g], a.g_top[g]);
    return rintf((cl - a.g_lo[g]) / a.g_step[g]);
}

__device__ inline bool tt_in_court(float x, float y) { return (x > TT_COURT_X0) && (x < TT_COURT_X1) && (y > TT_COURT_Y0) && (y < TT_COURT_Y1); }

// column c (0..143) of quat_to_rot6d(rigid_body_rot[:, :24]): the reference hands Isaac Gym's (x, y, z, w) numbers to
// quaternion_to_rotation_matrix with its default order WXYZ (utils/torch_transform.py:249-250, konia_transform.py:474-549), so the four
// numbers are unpacked as w, x, y, z = q[0], q[1], q[2], q[3]; rot6d = columns 0 and 1 of that matrix
__device__ inline float tt_rot6d(const float* q4, int k) {
    const float n = tt_clamp_min(sqrtf(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]), 1e-12f);
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

template <bool STEP>
__global__ __launch_bounds__(TT_WAVE* TT_WPB) void tennis_task_kernel(const TennisArgs a) {
    const int lane = threadIdx.x & (TT_WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * TT_WPB + (threadIdx.x >> 6);
    if (row >= a.rows) return;  // (the whole wave)
    const int64_t e = STEP ? row : a.env_ids[row];
    if (e < 0 || e >= a.num_envs) return;
    const v2p_tennis_cfg& c = a.c;
    const v2p_tennis_buffers& b = a.b;
    const int L = c.obs_ball_traj_length;

    const float* rb = b.rb_state + e * (V2P_NUM_BODIES * 13);
    const float* rk = b.racket_state + e * 13;
    const float* ball = b.ball_state + e * 13;
    const float root[3] = {rb[0], rb[1], rb[2]};
    const float rvel[3] = {b.root_states[e * 13 + 7], b.root_states[e * 13 + 8], b.root_states[e * 13 + 9]};
    const float rpos[3] = {rk[0], rk[1], rk[2]};
    const float bpos[3] = {ball[0], ball[1], ball[2]};
    // racket normal: rotation of the wrist link (a proper xyzw -> wxyz conversion here, humanoid_smpl_im_mvae.py:831-845) x grip normal
    float rnorm[3];
    {
        int64_t wl = b.wrist_link[e];
        wl = wl < 0 ? 0 : (wl > V2P_NUM_BODIES - 1 ? V2P_NUM_BODIES - 1 : wl);
        const float* q = rb + wl * 13 + 3;
        const float n = tt_clamp_min(sqrtf(q[3] * q[3] + q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), 1e-12f);
        const float w = q[3] / n, x = q[0] / n, y = q[1] / n, z = q[2] / n;
        const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
        const float m[9] = {1.f - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w, ty * x + tz * w, 1.f - (tx * x + tz * z),
                            tz * y - tx * w,         tz * x - ty * w, tz * y + tx * w, 1.f - (tx * x + ty * y)};
        for (int i = 0; i < 3; ++i) rnorm[i] = m[3 * i] * c.grip_normal[0] + m[3 * i + 1] * c.grip_normal[1] + m[3 * i + 2] * c.grip_normal[2];
    }

    // ---- the step's scalar part before the observation: counters, racket hit, _update_state, reward
    int64_t tar_time = 0, progress = 0, tar_action = 0;
    bool hit = false, hit_est_out = false;  // (hit_est_out: return_w_estimate's `has_contact & ~est_bounce_in`, :431)
    if (STEP) {
        tar_time = b.tar_time[e] + 1;
        progress = b.progress[e] + 1;
        tar_action = b.tar_action[e];
        hit = b.has_racket_contact[e] != 0;
        bool hit_now = b.has_racket_contact_now[e] != 0;
        const float vy = ball[8];
        if (c.contact_by_velocity) {
            hit_now = !hit && (vy > 0.f) && ((vy - b.prev_ball_vy[e]) > 10.f);
            hit = hit || hit_now;
        }
        bool bounce_in = b.bounce_in[e] != 0;
        if (tar_action == 0 && b.has_bounce_now[e]) bounce_in = tt_in_court(b.bounce_pos[e * 3], b.bounce_pos[e * 3 + 1]);
        float est[3] = {b.est_bounce_pos[e * 3], b.est_bounce_pos[e * 3 + 1], b.est_bounce_pos[e * 3 + 2]};
        float est_time = b.est_bounce_time[e], est_peak = b.est_max_height[e];
        bool est_in = b.est_bounce_in[e] != 0;
        bool overflow = false;
        if (hit_now) {
            // TennisBallOutEstimator.estimate (tennis_ball_out_estimator.py:164-205) of this one ball
            const float s0 = ball[0], s1 = ball[1], s2 = ball[2], s7 = ball[7], s8 = ball[8], s9 = ball[9];
            bool valid = (s8 > a.g_lo[0]) && (s9 > a.g_lo[1]) && (s9 < a.vy_hi) && (s2 < a.ty_hi);
            const float x_net = s0 + s7 * fabsf(s1 / s8);
            valid = valid && (x_net > -4.f) && (x_net < 4.f);
            if (valid) {
                const float vel_x = sqrtf(s7 * s7 + s8 * s8);
                overflow = vel_x >= a.vx_hi;
                const float vspin = sqrtf(ball[10] * ball[10] + ball[11] * ball[11] + ball[12] * ball[12]) / 6.283185307179586f;
                const float fidx = tt_index(a, 0, vel_x) * a.dim1 * a.dim2 + tt_index(a, 1, s9) * a.dim2 + tt_index(a, 2, vspin);
                int64_t ti = (int64_t)fidx;
                ti = ti < 0 ? 0 : (ti > c.table_rows - 1 ? c.table_rows - 1 : ti);
                int hi = (int)tt_index(a, 4, s2);
                hi = hi < 0 ? 0 : (hi > c.table_ny - 1 ? c.table_ny - 1 : hi);
                const float* ty = b.traj_out_y + (ti * c.table_ny + hi) * 2;
                const float* tx = b.traj_out_x + ti * c.table_nx;
                float bx = s0 + ty[0] * s7 / vel_x, by = s1 + ty[0] * s8 / vel_x, bt = ty[1];
                int ni = (int)tt_index(a, 3, -s1 / s8 * vel_x);
                ni = ni < 0 ? 0 : (ni > c.table_nx - 1 ? c.table_nx - 1 : ni);
                if (tx[ni] + s2 < TT_NET_HEIGHT) bx = by = bt = 0.f;  // into the net
                float top = -INFINITY;
                for (int k = lane; k < c.table_nx; k += TT_WAVE) top = fmaxf(top, tx[k]);
                for (int m = TT_WAVE / 2; m > 0; m >>= 1) top = fmaxf(top, __shfl_xor(top, m, TT_WAVE));
                est[0] = bx; est[1] = by; est_time = bt; est_peak = s2 + top;
                est_in = tt_in_court(bx, by);
            }
        }
        // the reward (compute_reward_reach / _return / _return_w_estimate, :492-602)
        const float phase = b.phase_pred[e];
        const int64_t swing = c.reward_type == V2P_TENNIS_REWARD_RETURN_W_ESTIMATE ? b.swing_type_cycle[e] : b.swing_type[e];
        const float d0 = bpos[0] - rpos[0], d1 = bpos[1] - rpos[1], d2 = bpos[2] - rpos[2];
        const float pos_err = d0 * d0 + d1 * d1 + d2 * d2;
        const bool early = c.reward_type == V2P_TENNIS_REWARD_REACH ? swing == -1 : swing >= 2;
        const float pd = phase - (early ? 3.f : 3.14159265358979323846f);
        const float near = expf(-c.scale_pos * pos_err) * expf(-c.scale_phase * (pd * pd));
        const float* tg = b.target_bounce_pos + e * 3;
        float rew, sub0, sub1 = 0.f;
        if (c.reward_type == V2P_TENNIS_REWARD_REACH) {
            sub0 = (tar_action == 1 ? 1.f : 0.f) * near;
            rew = sub0 * c.weight_pos;
        } else {
            sub0 = (hit ? 0.f : 1.f) * near + (hit ? 1.f : 0.f);
            if (c.reward_type == V2P_TENNIS_REWARD_RETURN) {
                const float* p = b.has_bounce[e] ? b.bounce_pos + e * 3 : bpos;
                const float u0 = p[0] - tg[0], u1 = p[1] - tg[1], u2 = p[2] - tg[2];
                sub1 = (hit ? 1.f : 0.f) * tt_clamp((400.f - (u0 * u0 + u1 * u1 + u2 * u2)) / 400.f, 0.f, 1.f);
            } else {
                const float u0 = est[0] - tg[0], u1 = est[1] - tg[1], u2 = est[2] - tg[2];
                sub1 = (est_in ? 1.f : 0.f) * expf(-c.scale_bounce_pos * (u0 * u0 + u1 * u1 + u2 * u2)) * expf(-c.scale_bounce_time * est_time);
            }
            rew = c.weight_pos * sub0 + c.weight_ball_pos * sub1;
        }
        if (lane == 0) {
            b.tar_time[e] = tar_time;
            b.progress[e] = progress;
            if (c.contact_by_velocity) {
                b.has_racket_contact[e] = hit ? 1 : 0;
                b.has_racket_contact_now[e] = hit_now ? 1 : 0;
            }
            b.prev_ball_vy[e] = vy;
            b.bounce_in[e] = bounce_in ? 1 : 0;
            b.est_bounce_pos[e * 3] = est[0];
            b.est_bounce_pos[e * 3 + 1] = est[1];
            b.est_bounce_time[e] = est_time;
            b.est_max_height[e] = est_peak;
            b.est_bounce_in[e] = est_in ? 1 : 0;
            if (overflow) atomicAdd((unsigned long long*)b.vel_x_overflow, 1ull);
            b.rew[e] = rew;
            if (c.reward_type == V2P_TENNIS_REWARD_REACH) b.sub_rewards[e] = sub0;
            else { b.sub_rewards[e * 2] = sub0; b.sub_rewards[e * 2 + 1] = sub1; }
        }
        hit_est_out = hit && !est_in;
    }

    // ---- the observation row (_compute_actor_obs :333-342, _compute_task_obs :344-360)
    float* obs = b.obs + e * a.width;
    bool nan_seen = false;
    for (int col = lane; col < TT_ACTOR; col += TT_WAVE) {
        float v;
        if (col < 3) v = root[col];
        else if (col < 6) v = rvel[col - 3];
        else if (col < 78) {
            const int k = col - 6, body = 1 + k / 3, ax = k % 3;
            v = (body < V2P_NUM_BODIES ? rb[body * 13 + ax] : rk[ax]) - root[ax];
        } else if (col < 222) {
            const int k = col - 78;
            v = tt_rot6d(rb + (k / 6) * 13 + 3, k % 6);
        } else v = rnorm[col - 222];
        obs[col] = v;
        nan_seen = nan_seen || (v != v);
    }
    const int cursor = (!c.use_history_ball_obs) ? min(max(b.traj_cursor[e], 0), TT_FRAMES) : 0;
    float* hist = b.ball_obs ? b.ball_obs + e * (int64_t)(L * 3) : nullptr;
    for (int i = lane; i < 3 * L; i += TT_WAVE) {
        float v = 0.f;
        if (hist) {
            // roll(-1) in place: slots [64 k, 64 k + 63] are written after the wave has read [64 k + 3, 64 k + 66], and no later
            // iteration reads below 64 (k + 1) + 3
            v = i < 3 * (L - 1) ? hist[i + 3] : bpos[i - 3 * (L - 1)];
            hist[i] = v;
        }
        if (!c.use_history_ball_obs) {
            const int f = cursor + i / 3;
            v = f < TT_FRAMES ? b.ball_traj[e * (TT_FRAMES * 3) + f * 3 + i % 3] : 0.f;
        }
        v = v - rpos[i % 3];
        obs[TT_ACTOR + i] = v;
        nan_seen = nan_seen || (v != v);
    }
    if (c.use_random_ball_target && lane < 2) {
        const float v = b.target_bounce_pos[e * 3 + lane] - root[lane];
        obs[TT_ACTOR + 3 * L + lane] = v;
        nan_seen = nan_seen || (v != v);
    }
    if (lane < 3) {
        b.racket_pos[e * 3 + lane] = rpos[lane];
        b.racket_normal[e * 3 + lane] = rnorm[lane];
    }
    if (!STEP) return;

    // ---- _compute_reset (:408-436) and the window's advance
    const bool has_nan = __any(nan_seen ? 1 : 0) != 0;
    if (lane != 0) return;
    bool terminated = (root[0] < c.court_min[0]) || (root[1] < c.court_min[1]) || (root[0] > c.court_max[0]) || (root[1] > c.court_max[1]);
    terminated = terminated || has_nan;
    bool reset = (progress >= c.max_episode_length - 1) ? true : terminated;
    bool reaction = tar_time == b.tar_time_total[e];
    const bool behind = bpos[1] < root[1] - 1.f;
    bool recovery = (tar_action == 1) && (hit || behind);
    b.distance[e] = b.distance[e] + sqrtf(rvel[0] * rvel[0] + rvel[1] * rvel[1]);
    bool terminate = terminated;
    if (c.enable_early_termination) {
        terminate = terminate || ((recovery && !hit) || behind);
        if (c.reward_type == V2P_TENNIS_REWARD_RETURN_W_ESTIMATE) terminate = terminate || hit_est_out;
    }
    if (terminate) { terminated = true; reset = true; recovery = false; }
    reaction = reaction || reset;
    b.terminate[e] = terminated ? 1 : 0;
    b.reset[e] = reset ? 1 : 0;
    b.reset_reaction[e] = reaction ? 1 : 0;
    b.reset_recovery[e] = recovery ? 1 : 0;
    if (!c.use_history_ball_obs) b.traj_cursor[e] = min(cursor + 1, TT_FRAMES);
}

int fill_args(TennisArgs& a, const v2p_tennis_cfg& c, const v2p_tennis_buffers& b) {
    a.c = c;
    a.b = b;
    a.width = TT_ACTOR + 3 * c.obs_ball_traj_length + (c.use_random_ball_target ? 2 : 0);
    for (int g = 0; g < 5; ++g) {
        a.g_lo[g] = (float)c.grid[g][0];
        a.g_top[g] = (float)(c.grid[g][1] - c.grid[g][2]);
        a.g_step[g] = (float)c.grid[g][2];
    }
    a.vx_hi = (float)c.grid[0][1];
    a.vy_hi = (float)c.grid[1][1];
    a.ty_hi = (float)c.grid[4][1];
    a.dim1 = (float)((c.grid[1][1] - c.grid[1][0]) / c.grid[1][2]);
    a.dim2 = (float)((c.grid[2][1] - c.grid[2][0]) / c.grid[2][2]);
    return V2P_OK;
}

}  // namespace

int launch_tennis_task_step(const v2p_tennis_cfg& c, int64_t n, const v2p_tennis_buffers& b, hipStream_t s) {
    TennisArgs a;
    fill_args(a, c, b);
    a.env_ids = nullptr;
    a.rows = a.num_envs = n;
    const dim3 grid((unsigned)((n + TT_WPB - 1) / TT_WPB)), block(TT_WAVE * TT_WPB);
    hipLaunchKernelGGL(tennis_task_kernel<true>, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "tennis_task_kernel");
}

int launch_tennis_task_obs(const v2p_tennis_cfg& c, int64_t num_envs, const v2p_tennis_buffers& b, const int64_t* env_ids, int64_t n_ids, hipStream_t s) {
    TennisArgs a;
    fill_args(a, c, b);
    a.env_ids = env_ids;
    a.rows = n_ids;
    a.num_envs = num_envs;
    const dim3 grid((unsigned)((n_ids + TT_WPB - 1) / TT_WPB)), block(TT_WAVE * TT_WPB);
    hipLaunchKernelGGL(tennis_task_kernel<false>, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "tennis_task_obs_kernel");
}

}  // namespace v2p
