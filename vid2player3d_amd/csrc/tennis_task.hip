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
//
// The two-player batch (physics_mvae_controller_dual.py, PhysicsMVAEControllerDual; envs 2k and 2k+1 are opponents) adds two launches.
// v2p_tennis_dual_step is a third instantiation of the step kernel, with the dual reset law: the rows of a pair lie in one workgroup and
// exchange their flags through LDS with one barrier.  v2p_tennis_dual_handover is the flag-driven half of the dual `_reset_envs`, one
// wavefront per pair: lanes 0..31 on the even env, 32..63 on the odd one, so that what an env takes from its opponent (the
// in-estimator's state, table row and direction) crosses the halves lane to lane.
#include <type_traits>

#include "ref_rotations.hpp"
#include "tennis_task.hpp"
#include "tennis_task_dev.hpp"

namespace v2p {

namespace {

// the two-player step's arguments: the racket normal in the wrist frame by the env's parity (the reference's `grip` list,
// humanoid_smpl_im_mvae.py:839-842)
struct TennisDualArgs : TennisArgs {
    float grip[2][3];
};

// One wave per row.  STEP: the whole task step of env `row`, else the observation of env env_ids[row].  DUAL (with STEP): the step of a
// two-player batch (PhysicsMVAEControllerDual) - no out-estimator, the grip of the env's parity and the dual reset law, whose flags
// cross the pair: rows is even and TT_WPB is, so env e and its opponent e ^ 1 are waves w and w ^ 1 of one workgroup.  Each leaves its
// own flags in LDS, and after the one barrier lane 0 closes the law with the opponent's (:108-121).  Every wave of the workgroup reaches
// that barrier: in this form nothing returns before it, and a wave without a row skips the work.  Nothing of the opponent is recomputed
// from global memory - its wave rewrites has_racket_contact, prev_ball_vy and bounce_in in this launch.
static_assert(TT_WPB % 2 == 0, "a pair must share a workgroup");
template <bool STEP, bool DUAL = false>
__global__ __launch_bounds__(TT_WAVE* TT_WPB) void tennis_task_kernel(const std::conditional_t<DUAL, TennisDualArgs, TennisArgs> a) {
    static_assert(STEP || !DUAL, "the dual form is a step");
    const int lane = threadIdx.x & (TT_WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * TT_WPB + (threadIdx.x >> 6);
    if (!DUAL && row >= a.rows) return;  // (the whole wave)
    // DUAL: the env's own half of the law, recovery | terminate << 1
    [[maybe_unused]] int own_flags = 0;
    if (!DUAL || row < a.rows) {
    const int64_t e = STEP ? row : a.env_ids[row];
    if (!DUAL && (e < 0 || e >= a.num_envs)) return;
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
    [[maybe_unused]] const float* grip = nullptr;
    if constexpr (DUAL) grip = a.grip[e & 1];
#define TT_ROW_RACKET_NORMAL
#define TT_ROW_GRIP(i) (DUAL ? grip[i] : c.grip_normal[i])
#include "tennis_row.inc"
#undef TT_ROW_GRIP
#undef TT_ROW_RACKET_NORMAL

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
        if constexpr (DUAL) {
            // the env's own half of PhysicsMVAEControllerDual._compute_reset (:96-114)
            const bool has_bounce = b.has_bounce[e] != 0;
            const bool recovery = (tar_action == 1) && (hit || (bpos[1] < root[1] - 1.f) || (has_bounce && bpos[2] < 0.05f));
            const bool terminate = (recovery && !hit) || (tar_action == 0 && has_bounce && !bounce_in);
            own_flags = (recovery ? 1 : 0) | (terminate ? 2 : 0);
        }
        float est[3] = {b.est_bounce_pos[e * 3], b.est_bounce_pos[e * 3 + 1], b.est_bounce_pos[e * 3 + 2]};
        float est_time = b.est_bounce_time[e], est_peak = b.est_max_height[e];
        bool est_in = b.est_bounce_in[e] != 0;
        bool overflow = false;
        if (!DUAL && hit_now) {  // (the dual controller has no out-estimator, :73, 299: est_* keep what they hold)
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
            if (!DUAL) {
                b.est_bounce_pos[e * 3] = est[0];
                b.est_bounce_pos[e * 3 + 1] = est[1];
                b.est_bounce_time[e] = est_time;
                b.est_max_height[e] = est_peak;
                b.est_bounce_in[e] = est_in ? 1 : 0;
                if (overflow) atomicAdd((unsigned long long*)b.vel_x_overflow, 1ull);
            }
            b.rew[e] = rew;
            if (c.reward_type == V2P_TENNIS_REWARD_REACH) b.sub_rewards[e] = sub0;
            else { b.sub_rewards[e * 2] = sub0; b.sub_rewards[e * 2 + 1] = sub1; }
        }
        hit_est_out = hit && !est_in;
    }

    // ---- the observation row
#define TT_ROW_OBSERVATION
#define TT_ROW_LANES TT_WAVE
#include "tennis_row.inc"
#undef TT_ROW_LANES
#undef TT_ROW_OBSERVATION
    if (!STEP) return;

    if constexpr (DUAL) {
        // ---- _compute_stats and the window's advance; the reset law closes after the barrier
        if (lane == 0) {
            b.distance[e] = b.distance[e] + sqrtf(rvel[0] * rvel[0] + rvel[1] * rvel[1]);
            if (!c.use_history_ball_obs) b.traj_cursor[e] = min(cursor + 1, TT_FRAMES);
        }
    } else {
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
    }
    if constexpr (DUAL) {
        // ---- the pair's exchange and the rest of PhysicsMVAEControllerDual._compute_reset (:108-121)
        __shared__ int pair_flags[TT_WPB];
        const int w = threadIdx.x >> 6;
        if (lane == 0) pair_flags[w] = own_flags;
        __syncthreads();
        if (row >= a.rows || lane != 0) return;
        const int opponent = pair_flags[w ^ 1];
        bool recovery = (own_flags & 1) != 0, reaction = (opponent & 1) != 0;  // recovery also marks the reaction of the opponent
        if ((own_flags | opponent) & 2) {
            a.b.reset[row] = 1;  // (left alone otherwise, as in the reference; the `terminate` buffer is not written)
            recovery = reaction = false;
        }
        a.b.reset_reaction[row] = reaction ? 1 : 0;
        a.b.reset_recovery[row] = recovery ? 1 : 0;
    }
}

// ---- the hand-over: the flag-driven half of PhysicsMVAEControllerDual._reset_envs (:42-64) with HumanoidSMPLIMMVAEDual._reset_balls
// (humanoid_smpl_im_mvae_dual.py:65-79) and TennisBallInEstimator.estimate (utils/tennis_ball_in_estimator.py:22-79)
constexpr int TH_HALF = TT_WAVE / 2;                                   // lanes of an env
constexpr int TH_ROW_ITERS = (TT_FRAMES * 3 + TH_HALF - 1) / TH_HALF;  // passes of a half wave over a ball_traj row

struct TennisHandArgs {
    TennisArgs a;
    v2p_tennis_dual_buffers d;
    float grip[2][3];
    // the in-estimator's grids HEIGHT, VEL_X, VEL_Y, VSPIN as torch sees them: (lo, hi - step, step) in float32 and the cells of each
    // range, (hi - lo) / step, as the float32 factor of the row index
    float i_lo[4], i_top[4], i_step[4], i_dim[4];
    int64_t in_rows, pairs;
    int in_frames;
};

__device__ inline float th_cell(const TennisHandArgs& h, int g, float v) {
    const float cl = tt_clamp(v, h.i_lo[g], h.i_top[g]);
    return rintf((cl - h.i_lo[g]) / h.i_step[g]);
}

// spin * 2 pi * normalize(cross(vel, (0, 0, -1))) as torch evaluates it (:70-71, 76-77)
__device__ inline void th_ang_vel(const float* v, float spin, float* out) {
    const float c0 = v[1] * -1.f - v[2] * 0.f, c1 = v[2] * 0.f - v[0] * -1.f, c2 = v[0] * 0.f - v[1] * 0.f;
    const float n = ref_clamp_min(sqrtf(c0 * c0 + c1 * c1 + c2 * c2), 1e-12f);
    const float mag = spin * 3.14159265358979323846f * 2.f;
    out[0] = mag * (c0 / n);
    out[1] = mag * (c1 / n);
    out[2] = mag * (c2 / n);
}

// `_compute_observations` of one env by LANES lanes: the text of the step kernel's row
template <int LANES>
__device__ void th_observation(const TennisArgs& a, const float* grip, int64_t e, int lane, const float (&bpos)[3]) {
    const v2p_tennis_cfg& c = a.c;
    const v2p_tennis_buffers& b = a.b;
    const int L = c.obs_ball_traj_length;
    const float* rb = b.rb_state + e * (V2P_NUM_BODIES * 13);
    const float* rk = b.racket_state + e * 13;
    const float root[3] = {rb[0], rb[1], rb[2]};
    const float rvel[3] = {b.root_states[e * 13 + 7], b.root_states[e * 13 + 8], b.root_states[e * 13 + 9]};
    const float rpos[3] = {rk[0], rk[1], rk[2]};
#define TT_ROW_RACKET_NORMAL
#define TT_ROW_GRIP(i) grip[i]
#include "tennis_row.inc"
#undef TT_ROW_GRIP
#undef TT_ROW_RACKET_NORMAL
#define TT_ROW_OBSERVATION
#define TT_ROW_LANES LANES
#include "tennis_row.inc"
#undef TT_ROW_LANES
#undef TT_ROW_OBSERVATION
    (void)nan_seen;
    (void)cursor;
}

// One wavefront per pair: lanes 0..31 work on env 2p, lanes 32..63 on env 2p+1, each half uniformly on its env's scalars.  An env
// writes only its own rows, and what it needs of its opponent reaches it through __shfl_xor(., 32) before either half has written
// anything, so the two halves cannot race.  Every cross-lane operation stands before the first divergent branch.
__global__ __launch_bounds__(TT_WAVE* TT_WPB) void tennis_handover_kernel(const TennisHandArgs h) {
    const int lane = threadIdx.x & (TT_WAVE - 1), hl = lane & (TH_HALF - 1);
    const int64_t pair = (int64_t)blockIdx.x * TT_WPB + (threadIdx.x >> 6);
    if (pair >= h.pairs) return;  // (the whole wave)
    const int64_t e = 2 * pair + (lane >> 5);
    const v2p_tennis_cfg& c = h.a.c;
    const v2p_tennis_buffers& b = h.a.b;
    const v2p_tennis_dual_buffers& d = h.d;

    // ---- a. both ball states: the env's own row; the opponent's comes through the lanes below
    float own[13];
    for (int i = 0; i < 13; ++i) own[i] = d.ball_state[e * 13 + i];
    const bool react = b.reset_reaction[e] != 0, recover = b.reset_recovery[e] != 0;
    const bool opp_react = __shfl_xor(react ? 1 : 0, TH_HALF, TT_WAVE) != 0;

    // ---- b. the in-estimator on this env's state, where the opponent reacts to it: the state that comes in on the other side (s_in),
    // the one that leaves here (s_out), the table row and the direction
    float s_in[13], s_out[13], dir[2] = {0.f, 0.f};
    int64_t trow = 0;
    for (int i = 0; i < 13; ++i) s_in[i] = s_out[i] = own[i];
    if (opp_react) {
        const float vel_x = sqrtf(own[7] * own[7] + own[8] * own[8]);
        dir[0] = own[7] / vel_x;
        dir[1] = own[8] / vel_x;
        const float vspin = sqrtf(own[10] * own[10] + own[11] * own[11] + own[12] * own[12]) / 6.283185307179586f;
        const float ih = th_cell(h, 0, own[2]), ix = th_cell(h, 1, vel_x), iy = th_cell(h, 2, own[9]), iv = th_cell(h, 3, vspin);
        const float fidx = ih * h.i_dim[1] * h.i_dim[2] * h.i_dim[3] + ix * h.i_dim[2] * h.i_dim[3] + iy * h.i_dim[3] + iv;
        trow = (int64_t)fidx;
        trow = trow < 0 ? 0 : (trow > h.in_rows - 1 ? h.in_rows - 1 : trow);  // (a NaN state must not index outside the table)
        const float height_q = ih * h.i_step[0] + h.i_lo[0], vel_x_q = ix * h.i_step[1] + h.i_lo[1];
        const float vel_y_q = iy * h.i_step[2] + h.i_lo[2], vspin_q = iv * h.i_step[3] + h.i_lo[3];
        s_in[0] = own[0] * -1.f;
        s_in[1] = own[1] * -1.f;
        s_in[2] = height_q;
        s_in[7] = -vel_x_q * dir[0];
        s_in[8] = -vel_x_q * dir[1];
        s_in[9] = vel_y_q;
        th_ang_vel(s_in + 7, vspin_q, s_in + 10);
        for (int i = 0; i < 13; ++i) s_out[i] = s_in[i];
        s_out[0] = s_in[0] * -1.f;
        s_out[1] = s_in[1] * -1.f;
        s_out[7] = s_in[7] * -1.f;
        s_out[8] = s_in[8] * -1.f;
        th_ang_vel(s_out + 7, vspin_q, s_out + 10);
    }
    // what the opponent made of ITS state for this env: in-state, table row, direction, launch point
    float got[13];
    for (int i = 0; i < 13; ++i) got[i] = __shfl_xor(s_in[i], TH_HALF, TT_WAVE);
    const int64_t got_row = (int64_t)__shfl_xor((int)trow, TH_HALF, TT_WAVE);
    const float got_dir[2] = {__shfl_xor(dir[0], TH_HALF, TT_WAVE), __shfl_xor(dir[1], TH_HALF, TT_WAVE)};
    const float got_xy[2] = {__shfl_xor(own[0], TH_HALF, TT_WAVE), __shfl_xor(own[1], TH_HALF, TT_WAVE)};
    // (no cross-lane operation below this line)
    // Where both envs of a pair react, the reference's sorted opponent list (utils/common.py:111-115) pairs each with ITSELF: its flight
    // is the table row of its own state, not of its opponent's
    const bool self = react && opp_react;
    const int64_t src_row = self ? trow : got_row;
    const float src_dir[2] = {self ? dir[0] : got_dir[0], self ? dir[1] : got_dir[1]};
    const float src_xy[2] = {self ? own[0] : got_xy[0], self ? own[1] : got_xy[1]};

    // ---- c. the table row's F frames, transformed and mirrored (:61-62), in front of frames F..99 of the env's window: the
    // reference's `_ball_traj[ids, :F] = new_traj` on its rolled tensor.  The old row is read whole before it is written.
    // (With use_history_ball_obs nobody reads the window, and its cursor stands still: it is not kept.)
    if (react && !c.use_history_ball_obs) {
        float* row = d.ball_traj + e * (TT_FRAMES * 3);
        const int F = h.in_frames;
        const int cursor = min(max(b.traj_cursor[e], 0), TT_FRAMES);
        const float* table = d.traj_in + src_row * (int64_t)(F * 2);
        float v[TH_ROW_ITERS];
#pragma unroll
        for (int k = 0; k < TH_ROW_ITERS; ++k) {
            const int i = k * TH_HALF + hl, f = i / 3, ax = i % 3;
            v[k] = 0.f;
            if (i < TT_FRAMES * 3) {
                if (f < F) {
                    const float dist = table[f * 2], height = table[f * 2 + 1];
                    v[k] = ax == 2 ? height : (dist * src_dir[ax & 1] + src_xy[ax & 1]) * -1.f;
                } else if (cursor + f < TT_FRAMES) v[k] = row[(cursor + f) * 3 + ax];
            }
        }
#pragma unroll
        for (int k = 0; k < TH_ROW_ITERS; ++k) {
            const int i = k * TH_HALF + hl;
            if (i < TT_FRAMES * 3) row[i] = v[k];
        }
        if (hl == 0) b.traj_cursor[e] = 0;
    }

    // ---- d. the ball states: ball_states_in to the reacting env, then ball_states_out to its opponent - where both react, out wins
    float fin[13];
    for (int i = 0; i < 13; ++i) fin[i] = opp_react ? s_out[i] : (react ? got[i] : own[i]);
    if (hl == 0) {
        if (react || opp_react)
            for (int i = 0; i < 13; ++i) d.ball_state[e * 13 + i] = fin[i];
        // ---- e. _reset_balls :75-79 (the opponent's prev_ball_vy stays)
        if (react) {
            d.has_bounce[e] = 0;
            for (int i = 0; i < 3; ++i) d.bounce_pos[e * 3 + i] = 0.f;
            b.has_racket_contact[e] = 0;
            b.prev_ball_vy[e] = fin[8];
        }
        // ---- f. _reset_recovery_tasks (:91-94)
        if (recover) {
            d.tar_action[e] = 0;
            d.has_bounce[e] = 0;
            for (int i = 0; i < 3; ++i) d.bounce_pos[e * 3 + i] = 0.f;
        }
    }
    if (!react) return;
    // ---- g. the dual _reset_reaction_tasks (:68-89); an env in both lists ends with tar_action = 1
    const int L = c.obs_ball_traj_length;
    if (c.use_history_ball_obs)
        for (int i = hl; i < 3 * L; i += TH_HALF) b.ball_obs[e * (int64_t)(L * 3) + i] = fin[i % 3];
    if (hl == 0) {
        b.tar_time[e] = 0;
        d.tar_action[e] = 1;
        d.num_reset_reaction[e] = d.num_reset_reaction[e] + 1;
        b.bounce_in[e] = 0;
        if (c.use_random_ball_target) {
            const float u = d.target_draw[e];
            d.target_bounce_pos[e * 3] = u < 0.33f ? -3.f : (u > 0.67f ? 3.f : 0.f);
            d.target_bounce_pos[e * 3 + 1] = 10.f;
            d.target_bounce_pos[e * 3 + 2] = 0.f;
        }
        if (c.reward_type == V2P_TENNIS_REWARD_RETURN_W_ESTIMATE) {
            for (int i = 0; i < 3; ++i) b.est_bounce_pos[e * 3 + i] = 0.f;
            b.est_bounce_time[e] = 0.f;
            b.est_bounce_in[e] = 0;
            b.est_max_height[e] = 0.f;
        }
    }
    // ---- h. _compute_observations(reset_reaction_env_ids) (:64): the row reads what other lanes of this half have just written
    // (window, cursor, history, target), hence the fence
    __threadfence_block();
    const float bpos[3] = {fin[0], fin[1], fin[2]};
    th_observation<TH_HALF>(h.a, h.grip[e & 1], e, hl, bpos);
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

int launch_tennis_dual_step(const v2p_tennis_cfg& c, const v2p_tennis_dual_cfg& dc, int64_t n, const v2p_tennis_buffers& b, hipStream_t s) {
    TennisDualArgs a;
    // (the out-estimator's grids in c are not validated for the two dual calls and may be zero: fill_args then forms inf / NaN on the host
    // in double, and neither kernel reads g_*, vx_hi .. dim2)
    fill_args(a, c, b);
    a.env_ids = nullptr;
    a.rows = a.num_envs = n;
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 3; ++i) a.grip[p][i] = dc.grip_normal[p][i];
    const dim3 grid((unsigned)((n + TT_WPB - 1) / TT_WPB)), block(TT_WAVE * TT_WPB);
    hipLaunchKernelGGL((tennis_task_kernel<true, true>), grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "tennis_task_kernel<STEP, DUAL>");
}

int launch_tennis_dual_handover(const v2p_tennis_cfg& c, const v2p_tennis_dual_cfg& dc, int64_t n, const v2p_tennis_buffers& b,
                                const v2p_tennis_dual_buffers& db, hipStream_t s) {
    TennisHandArgs h;
    fill_args(h.a, c, b);
    h.a.env_ids = nullptr;
    h.a.rows = h.a.num_envs = n;
    h.d = db;
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 3; ++i) h.grip[p][i] = dc.grip_normal[p][i];
    for (int g = 0; g < 4; ++g) {
        h.i_lo[g] = (float)dc.in_grid[g][0];
        h.i_top[g] = (float)(dc.in_grid[g][1] - dc.in_grid[g][2]);
        h.i_step[g] = (float)dc.in_grid[g][2];
        h.i_dim[g] = (float)((dc.in_grid[g][1] - dc.in_grid[g][0]) / dc.in_grid[g][2]);
    }
    h.in_rows = dc.in_rows;
    h.in_frames = dc.in_frames;
    h.pairs = n / 2;
    const dim3 grid((unsigned)((h.pairs + TT_WPB - 1) / TT_WPB)), block(TT_WAVE * TT_WPB);
    hipLaunchKernelGGL(tennis_handover_kernel, grid, block, 0, s, h);
    return check_hip(hipGetLastError(), "tennis_handover_kernel");
}

}  // namespace v2p
