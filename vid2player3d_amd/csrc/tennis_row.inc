// Two pieces of an env's row that the task-step kernel and the hand-over kernel of tennis_task.hip both need, as TEXT: the step kernel
// includes them into its body, the hand-over through two device functions; the evaluation step (tennis_eval.hip) includes them like the
// step kernel.  They are text and not functions of the step kernel because
// the existing instantiations of tennis_task_kernel must stay the machine code they were (tools/kernel_identity.py), and moving
// either piece into a function call - inlined or not - moves their instruction streams.  A change that is allowed to move the old
// kernels' code should turn both pieces into __device__ functions: as text they lean on a dozen names of the including scope.
//
// TT_ROW_RACKET_NORMAL: `float rnorm[3]`, the racket normal - rotation of the wrist link (a proper xyzw -> wxyz conversion here,
// humanoid_smpl_im_mvae.py:831-845) x grip normal.  Reads rb, b, e and TT_ROW_GRIP(i), component i of the env's grip normal.
//
// TT_ROW_OBSERVATION: the observation row (_compute_actor_obs :333-342, _compute_task_obs :344-360) with the history roll, racket_pos
// and racket_normal.  TT_ROW_LANES lanes (`lane` 0 .. TT_ROW_LANES-1, in lockstep) stride the columns.  Reads a, b, c, e, lane, L, rb,
// rk, root, rvel, rpos, bpos, rnorm; leaves `nan_seen` (this lane saw a NaN) and `cursor` (the first frame of the env's window).
#if defined(TT_ROW_RACKET_NORMAL)
    float rnorm[3];
    {
        int64_t wl = b.wrist_link[e];
        wl = wl < 0 ? 0 : (wl > V2P_NUM_BODIES - 1 ? V2P_NUM_BODIES - 1 : wl);
        const float* q = rb + wl * 13 + 3;
        const float n = ref_clamp_min(sqrtf(q[3] * q[3] + q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), 1e-12f);
        const float w = q[3] / n, x = q[0] / n, y = q[1] / n, z = q[2] / n;
        const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
        const float m[9] = {1.f - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w, ty * x + tz * w, 1.f - (tx * x + tz * z),
                            tz * y - tx * w,         tz * x - ty * w, tz * y + tx * w, 1.f - (tx * x + ty * y)};
        for (int i = 0; i < 3; ++i) rnorm[i] = m[3 * i] * TT_ROW_GRIP(0) + m[3 * i + 1] * TT_ROW_GRIP(1) + m[3 * i + 2] * TT_ROW_GRIP(2);
    }
#elif defined(TT_ROW_OBSERVATION)
    float* obs = b.obs + e * a.width;
    bool nan_seen = false;
    for (int col = lane; col < TT_ACTOR; col += TT_ROW_LANES) {
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
    for (int i = lane; i < 3 * L; i += TT_ROW_LANES) {
        float v = 0.f;
        if (hist) {
            // roll(-1) in place, W = TT_ROW_LANES: slots [W k, W k + W - 1] are written after the lanes have read [W k + 3, W k + W + 2],
            // and no later iteration reads below W (k + 1) + 3
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
#else
#error "tennis_row.inc: define TT_ROW_RACKET_NORMAL or TT_ROW_OBSERVATION"
#endif
