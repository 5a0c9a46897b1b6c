// The tennis controller's evaluation step (vid2player/env/tasks/mvae_controller_vis.py, MVAEControllerVis - what `run.py --test` runs
// in place of PhysicsMVAEController) in one launch: v2p_tennis_eval_step = the task step of tennis_task.hip with the test-mode episode
// law (`_compute_reset`, :64-79), the four per-env meters of `_compute_stats` (:81-95) and one frame of the record (:140-146).
//
// The step's layout: one wave64 per env, TT_WPB envs per workgroup.  Counters, the velocity rule of the racket hit, `_update_state`,
// the out-estimator, the reward and the window's advance are the step kernel's lines (tennis_task.hip, STEP && !DUAL), the observation
// row is tennis_row.inc's text; the arithmetic is built like that file's, without FMA contraction.  What differs stands at the end:
// lane 0 closes the law and updates the env's meters - an env owns its sixteen meter words, so there is no atomic and one order of
// adds - and the lanes write the 72 floats of the env's `_joint_rot` (humanoid_smpl_im_mvae.py:813-820) and the rest of the frame.
// `distance` is not touched (`_compute_stats` replaces the training task's), a NaN in the row and a root outside the court end nothing.
#include "ref_rotations.hpp"
#include "tennis_eval.hpp"
#include "tennis_pose_dev.hpp"
#include "tennis_task_dev.hpp"

namespace v2p {

namespace {

struct TennisEvalArgs {
    TennisArgs a;
    v2p_tennis_eval_buffers x;
    int64_t episode_length, frame;
    // body_of_smpl, 5 bits per joint: a table in the kernel arguments indexed by the lane would be copied to scratch
    uint64_t body_of_smpl[TE_JOINTS / TE_PACK];
};

// AverageMeterUnSync.update (utils/common.py:52-63) of one env: sum += val, count += 1, avg = sum / count (float32 / int64 is a
// float32 division in torch), max = where(val > max, val, max)
__device__ inline void te_meter(const v2p_tennis_eval_buffers& x, int m, int64_t e, float val) {
    const float sum = x.meter_sum[m][e] + val;
    const int64_t count = x.meter_count[m][e] + 1;
    const float top = x.meter_max[m][e];
    x.meter_sum[m][e] = sum;
    x.meter_count[m][e] = count;
    x.meter_avg[m][e] = sum / (float)count;
    x.meter_max[m][e] = val > top ? val : top;
}

__global__ __launch_bounds__(TT_WAVE* TT_WPB) void tennis_eval_kernel(const TennisEvalArgs h) {
    const TennisArgs& a = h.a;
    const int lane = threadIdx.x & (TT_WAVE - 1);
    const int64_t e = (int64_t)blockIdx.x * TT_WPB + (threadIdx.x >> 6);
    if (e >= a.rows) return;  // (the whole wave)
    const v2p_tennis_cfg& c = a.c;
    const v2p_tennis_buffers& b = a.b;
    const v2p_tennis_eval_buffers& x = h.x;
    const int L = c.obs_ball_traj_length;

    const float* rb = b.rb_state + e * (V2P_NUM_BODIES * 13);
    const float* rk = b.racket_state + e * 13;
    const float* ball = b.ball_state + e * 13;
    const float root[3] = {rb[0], rb[1], rb[2]};
    const float rvel[3] = {b.root_states[e * 13 + 7], b.root_states[e * 13 + 8], b.root_states[e * 13 + 9]};
    const float rpos[3] = {rk[0], rk[1], rk[2]};
    const float bpos[3] = {ball[0], ball[1], ball[2]};
#define TT_ROW_RACKET_NORMAL
#define TT_ROW_GRIP(i) c.grip_normal[i]
#include "tennis_row.inc"
#undef TT_ROW_GRIP
#undef TT_ROW_RACKET_NORMAL

    // ---- the step's scalar part before the observation, as in tennis_task_kernel<true>: counters, racket hit, _update_state, reward
    const int64_t tar_time = b.tar_time[e] + 1, progress = b.progress[e] + 1, tar_action = b.tar_action[e];
    bool hit = b.has_racket_contact[e] != 0;
    bool hit_now = b.has_racket_contact_now[e] != 0;
    const float vy = ball[8];
    if (c.contact_by_velocity) {
        hit_now = !hit && (vy > 0.f) && ((vy - b.prev_ball_vy[e]) > 10.f);
        hit = hit || hit_now;
    }
    const bool has_bounce = b.has_bounce[e] != 0;
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
    const int64_t cycle = b.swing_type_cycle[e];
    const int64_t swing = c.reward_type == V2P_TENNIS_REWARD_RETURN_W_ESTIMATE ? cycle : b.swing_type[e];
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
            const float* p = has_bounce ? b.bounce_pos + e * 3 : bpos;
            const float u0 = p[0] - tg[0], u1 = p[1] - tg[1], u2 = p[2] - tg[2];
            sub1 = (hit ? 1.f : 0.f) * tt_clamp((400.f - (u0 * u0 + u1 * u1 + u2 * u2)) / 400.f, 0.f, 1.f);
        } else {
            const float u0 = est[0] - tg[0], u1 = est[1] - tg[1], u2 = est[2] - tg[2];
            sub1 = (est_in ? 1.f : 0.f) * expf(-c.scale_bounce_pos * (u0 * u0 + u1 * u1 + u2 * u2)) * expf(-c.scale_bounce_time * est_time);
        }
        rew = c.weight_pos * sub0 + c.weight_ball_pos * sub1;
    }
    // `_compute_stats`' bounce error, on the target the observation is about to read (nothing below writes it)
    const float g0 = est[0] - tg[0], g1 = est[1] - tg[1], g2 = est[2] - tg[2];
    const float bounce_err = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
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

    // ---- the observation row
#define TT_ROW_OBSERVATION
#define TT_ROW_LANES TT_WAVE
#include "tennis_row.inc"
#undef TT_ROW_LANES
#undef TT_ROW_OBSERVATION
    (void)nan_seen;  // (a NaN in the row ends nothing here)

    // ---- the record's frame (:140-146): the lanes write the env's 72 floats of `_joint_rot`, lanes 0..2 the three positions
    if (x.joint_rot) {
        const int64_t at = h.frame * a.rows + e;
        te_pose_row(rb, x.dof_state, e, h.body_of_smpl, lane, TT_WAVE, x.joint_rot, at);  // (tennis_pose_dev.hpp)
        if (lane < 3) {
            x.root_pos[at * 3 + lane] = rb[lane];
            x.ball_pos[at * 3 + lane] = ball[lane];
            x.target_pos[at * 3 + lane] = tg[lane];
        }
        if (lane == 0) {
            x.phase[at] = phase;
            x.swing_type_cycle[at] = cycle;
        }
    }
    if (lane != 0) return;

    // ---- MVAEControllerVis._compute_reset (:64-79), `_compute_stats` (:81-95) and the window's advance
    const bool terminate = progress > h.episode_length;
    const bool in_time = tar_time >= b.tar_time_total[e];
    bool reaction = (hit && tar_action == 0 && has_bounce && in_time) || (!hit && in_time);
    bool recovery = (tar_action == 1) && (hit || (bpos[1] < root[1] - 1.f) || (fabsf(vy) < 2.f));
    if (terminate) { reaction = true; recovery = false; }
    b.terminate[e] = terminate ? 1 : 0;
    b.reset[e] = terminate ? 1 : 0;
    b.reset_reaction[e] = reaction ? 1 : 0;
    b.reset_recovery[e] = recovery ? 1 : 0;
    if (recovery) {
        te_meter(x, V2P_TENNIS_METER_HIT_RATE, e, hit ? 1.f : 0.f);
        te_meter(x, V2P_TENNIS_METER_FH_RATIO, e, cycle == 1 ? 1.f : 0.f);
        te_meter(x, V2P_TENNIS_METER_BOUNCE_IN_RATE, e, est_in ? 1.f : 0.f);
        if (est_in) te_meter(x, V2P_TENNIS_METER_BOUNCE_IN_POS_ERROR, e, bounce_err);
    }
    if (!c.use_history_ball_obs) b.traj_cursor[e] = min(cursor + 1, TT_FRAMES);
}

}  // namespace

int launch_tennis_eval_step(const v2p_tennis_cfg& c, const v2p_tennis_eval_cfg& ec, int64_t n, const v2p_tennis_buffers& b, const v2p_tennis_eval_buffers& x,
                            int64_t frame, hipStream_t s) {
    TennisEvalArgs h;
    fill_args(h.a, c, b);
    h.a.env_ids = nullptr;
    h.a.rows = h.a.num_envs = n;
    h.x = x;
    h.episode_length = ec.episode_length;
    h.frame = frame;
    te_pack_body_of_smpl(ec.body_of_smpl, h.body_of_smpl);
    const dim3 grid((unsigned)((n + TT_WPB - 1) / TT_WPB)), block(TT_WAVE * TT_WPB);
    hipLaunchKernelGGL(tennis_eval_kernel, grid, block, 0, s, h);
    return check_hip(hipGetLastError(), "tennis_eval_kernel");
}

}  // namespace v2p
