// What stands around the policy networks' dense layers in a control step of the tennis controller (vid2player/players/im_player.py:187-199,
// players/v2p_player.py:113-131): v2p_policy_input is clamp(obs, +-clip_obs) -> the network's input normaliser (models/running_norm.py:31-42
// in eval mode, or rl_games' RunningMeanStd in eval mode), v2p_ll_policy_input the same behind the low-level policy's 734-d observation
// computed in place from the engine's state, v2p_ll_policy_actions clamp(mu, +-clip_actions) -> `_action_to_pd_targets`.  The dense
// layers between them stay with hipBLASLt: an 8192 x 1024 x 1024 fp32 layer runs near the fp32 MFMA peak there, and a row tile of a
// fused kernel would re-read all weights per workgroup.
//
// A two-player batch (models/im_network_builder_dual.py:37-45: rows 0::2 through network1, rows 1::2 through network2, outputs
// interleaved) is written in side-major order - env i is row (i & 1) * (n / 2) + (i >> 1) - so that each network's operand is one
// contiguous block: the gathers and the interleaving cat of the reference are index arithmetic of these kernels.
//
// All three are bound by their launch and by HBM: 8192 x 734 floats are 24 MB in and out.  The elementwise kernels take one thread per
// element (adjacent lanes, adjacent columns); the low-level one shares obs_imitation_kernel's mapping and device code (eight envs of 24
// body lanes per workgroup), stages the eight rows in LDS (23 KB) and lets the whole workgroup stride them for the clamp, the
// normaliser and both stores - the raw rows of a workgroup are one contiguous piece of the output.
//
// Built without FMA contraction like tennis_task.hip; the division and the square root are the correctly rounded ones (no fast-math
// flag in this object): the results are torch's float32 elementwise results bit for bit.
#include <math.h>

#include "policy_io.hpp"
#include "mvae_target.hpp"
#include "v2p_dev.hpp"
#include "phys_common.hpp"

namespace v2p {

namespace {

#include "post_ops.inc"
#include "obs_imitation_row.inc"

constexpr int PI_BLOCK = 256;
constexpr int LL_BLOCK = 192;              // 8 envs x 24 bodies = 3 wave64, as obs_imitation_kernel
constexpr int LL_ENVS = LL_BLOCK / NB;
constexpr int LL_OBS = POLICY_LL_OBS;

// torch.clamp(v, -c, c): compare-and-select, so that a NaN stays a NaN (fminf / fmaxf would return the bound)
__device__ __forceinline__ float clamp_torch(float v, float c) {
    v = v < -c ? -c : v;
    return v > c ? c : v;
}

__device__ __forceinline__ float policy_norm(const v2p_policy_norm& nm, int64_t k, float v) {
    if (nm.kind == V2P_NORM_RUNNING) return clamp_torch((v - nm.mean[k]) / (nm.spread[k] + 1e-8f), nm.clip);
    if (nm.kind == V2P_NORM_MEAN_VAR) return clamp_torch((v - nm.mean[k]) / sqrtf(nm.spread[k] + nm.eps), nm.clip);
    return v;
}

// the network's row of env e
__device__ __forceinline__ int64_t side_major_row(int sides, int64_t n, int64_t e) { return sides == 2 ? (e & 1) * (n >> 1) + (e >> 1) : e; }

// one thread per element
__global__ __launch_bounds__(PI_BLOCK) void policy_input_kernel(const v2p_policy_input_cfg c, int64_t n, int64_t dim, const float* obs, float* x) {
    const int64_t tid = (int64_t)blockIdx.x * PI_BLOCK + threadIdx.x;
    if (tid >= n * dim) return;
    const int64_t e = tid / dim, k = tid - e * dim;
    const float v = clamp_torch(obs[tid], c.clip_obs);
    x[side_major_row(c.sides, n, e) * dim + k] = policy_norm(c.norm[c.sides == 2 ? (int)(e & 1) : 0], k, v);
}

__global__ __launch_bounds__(LL_BLOCK) void ll_policy_input_kernel(const v2p_policy_input_cfg c, int64_t n, const ObsImSrc in, float* raw, float* x) {
    __shared__ float rows[LL_ENVS * LL_OBS];
    const int le = threadIdx.x / NB, j = threadIdx.x % NB;
    const int64_t e0 = (int64_t)blockIdx.x * LL_ENVS;
    if (e0 + le < n) obs_imitation_row<ObsImEngine>(in, e0 + le, j, rows + le * LL_OBS);
    __syncthreads();
    const int64_t left = n - e0;
    const int count = (int)(left < LL_ENVS ? left : LL_ENVS) * LL_OBS;
    for (int idx = threadIdx.x; idx < count; idx += LL_BLOCK) {
        const int r = idx / LL_OBS, k = idx - r * LL_OBS;
        const int64_t e = e0 + r;
        const float v = rows[idx];
        if (raw) raw[e0 * LL_OBS + idx] = v;
        x[side_major_row(c.sides, n, e) * LL_OBS + k] = policy_norm(c.norm[c.sides == 2 ? (int)(e & 1) : 0], k, clamp_torch(v, c.clip_obs));
    }
}

// one thread per action component of the output (env order)
__global__ __launch_bounds__(PI_BLOCK) void ll_policy_actions_kernel(const v2p_mvae_target_cfg c, const v2p_mvae_target_buffers b, int64_t n, int sides,
                                                                     float clip_actions, const float* mu, float* out) {
    const int64_t tid = (int64_t)blockIdx.x * PI_BLOCK + threadIdx.x;
    if (tid >= n * NACT) return;
    const int64_t e = tid / NACT;
    const int col = (int)(tid - e * NACT);
    out[tid] = mvae_pd_target(c, b, e, col, clamp_torch(mu[side_major_row(sides, n, e) * NACT + col], clip_actions));
}

}  // namespace

int launch_policy_input(const v2p_policy_input_cfg& c, int64_t n, int64_t dim, const float* obs, float* x, hipStream_t s) {
    if (n <= 0) return V2P_OK;
    hipLaunchKernelGGL(policy_input_kernel, dim3((unsigned)((n * dim + PI_BLOCK - 1) / PI_BLOCK)), dim3(PI_BLOCK), 0, s, c, n, dim, obs, x);
    return check_hip(hipGetLastError(), "policy_input_kernel");
}

int launch_ll_policy_input(const v2p_policy_input_cfg& c, int64_t n, const v2p_ll_policy_src& src, float* raw_obs, float* x, hipStream_t s) {
    if (n <= 0) return V2P_OK;
    const float *rb = src.rb_state, *ds = src.dof_state, *tg = src.target;
    const ObsImSrc in = {rb, rb + 3, ds, ds + 1, rb + 7, rb + 10, src.motion_bodies, NB * 13, NB * 13, NDOF * 2, NDOF * 2, NB * 13, NB * 13, 11,
                         tg + MS_RB_POS, tg + MS_RB_ROT, tg + MS_DOF_POS, src.target_stride, src.target_stride, src.target_stride, 1, 1, 0};
    hipLaunchKernelGGL(ll_policy_input_kernel, dim3((unsigned)((n + LL_ENVS - 1) / LL_ENVS)), dim3(LL_BLOCK), 0, s, c, n, in, raw_obs, x);
    return check_hip(hipGetLastError(), "ll_policy_input_kernel");
}

int launch_ll_policy_actions(const v2p_mvae_target_cfg& c, int64_t n, int32_t sides, float clip_actions, const float* mu, const v2p_mvae_target_buffers& b,
                             float* actions_out, hipStream_t s) {
    if (n <= 0) return V2P_OK;
    hipLaunchKernelGGL(ll_policy_actions_kernel, dim3((unsigned)((n * NACT + PI_BLOCK - 1) / PI_BLOCK)), dim3(PI_BLOCK), 0, s, c, b, n, (int)sides, clip_actions, mu,
                       actions_out);
    return check_hip(hipGetLastError(), "ll_policy_actions_kernel");
}

}  // namespace v2p
