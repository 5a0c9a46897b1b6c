// What the kernels of the tennis controller's task step (tennis_task.hip) and of its test-mode step (tennis_eval.hip) share: the launch
// shape, the kernel arguments with the out-estimator's grids as torch sees them, and the small pieces of torch arithmetic of a row.
// Moved here from tennis_task.hip as they stood - the text of both files' kernels is the same as before (tools/kernel_identity.py).
#pragma once
#include "ref_rotations.hpp"
#include "v2p_internal.hpp"

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

// torch.clamp as torch evaluates it: a NaN stays a NaN (fminf / fmaxf would drop it); clamp_min is ref_rotations.hpp's
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

// (host) the kernel arguments of a cfg and its buffers; env_ids, rows and num_envs are the launcher's
inline int fill_args(TennisArgs& a, const v2p_tennis_cfg& c, const v2p_tennis_buffers& b) {
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

}  // namespace v2p
