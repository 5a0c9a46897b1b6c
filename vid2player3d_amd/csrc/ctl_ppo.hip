// The three row kernels of the tennis controller's PPO agent (V2PAgent, vid2player/agents/v2p_agent.py, over PhysicsMVAEController):
//   ctl_policy_head_kernel     what V2PModel.Network.forward(is_train = False) and the env wrapper do behind the `mu` layer
//                              (models/v2p_models.py:41-52, env/tasks/vec_task.py:103): sample, neglogp, the clamp the task steps on
//   ctl_rollout_record_kernel  the bookkeeping of play_steps behind env_step (v2p_agent.py:245-276)
//   ppo_loss_kernel (+ _reduce) the loss head of calc_gradients (v2p_agent.py:329-362, 395-397), forward and backward
// The dense layers between them stay with hipBLASLt (see policy_io.hip).  All three are bound by their launch and by HBM.
//
// Mapping.  The head and the loss take ONE WAVE PER ROW: an action row has at most 128 columns, lane k holds columns k and k + 64, the
// row sums (neglogp, KL, bound loss, dof_res) are butterflies over the wave - no LDS, no scratch; four rows per 256-thread workgroup.
// The record gives workgroup 0 the per-env scalars and every sum (thread t: envs t, t + 256, ... in rising order, float64) and lets the
// other workgroups stream the observation rows, 16 bytes per lane where the pointers allow it: its sums need no atomic and no word
// handed from one workgroup to another inside the launch, so they are the same bits on every run.  The loss reduces its statistics
// in two launches for the same reason (per-workgroup partials in float64, then one workgroup adds them in workgroup order): the eight
// XCDs of the chip have private L2s, and a partial handed over inside a launch would need an agent-scope release / acquire per workgroup.
//
// Built without FMA contraction like policy_io.hip; the division is the correctly rounded one (no fast-math flag in this object): the
// elementwise results are torch's float32 results bit for bit.
#include <math.h>

#include "ctl_ppo.hpp"
#include "v2p_dev.hpp"

namespace v2p {

namespace {

constexpr int BLOCK = 256;
constexpr int ROWS_PER_BLOCK = BLOCK / 64;
constexpr int NSTAT = 6;  // partial sums of the loss: actor, critic, bound, dof_res, clipped, KL
constexpr double HALF_LOG_2PI = 0.91893853320467274178;

// torch.clamp(v, lo, hi): compare-and-select, so that a NaN stays a NaN (fminf / fmaxf would return the bound)
__device__ __forceinline__ float clamp_torch(float v, float lo, float hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one wave per row
__global__ __launch_bounds__(BLOCK) void ctl_policy_head_kernel(int64_t n, int A, const float* __restrict__ mu, const float* __restrict__ logstd,
                                                                const float* __restrict__ sigma, const float* __restrict__ noise, float clip,
                                                                float* __restrict__ actions_row, float* __restrict__ mus_row, float* __restrict__ sigmas_row,
                                                                float* __restrict__ neglogp_row, float* __restrict__ actions_clamped) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n) return;  // (uniform over the wave)
    float q = 0.f, ls = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < A) {
            const int64_t i = r * A + k;
            const float m = mu[i], s = sigma[k];
            const float a = m + s * noise[i];
            const float t = (a - m) / s;
            q += t * t;
            ls += logstd[k];
            if (actions_row) actions_row[i] = a;
            if (mus_row) mus_row[i] = m;
            if (sigmas_row) sigmas_row[i] = s;
            actions_clamped[i] = clamp_torch(a, -clip, clip);
        }
    }
    q = wave_sum(q);
    ls = wave_sum(ls);
    if (lane == 0) neglogp_row[r] = 0.5f * q + (float)(HALF_LOG_2PI * A) + ls;
}

// workgroup 0: the per-env scalars and the sums; workgroups 1 ..: the observation rows
__global__ __launch_bounds__(BLOCK) void ctl_rollout_record_kernel(int64_t n, int64_t obs_dim, int S, float clip_obs, const float* __restrict__ obs,
                                                                   const float* __restrict__ rew, const int64_t* __restrict__ reset,
                                                                   const int64_t* __restrict__ terminate, const float* __restrict__ sub_rewards,
                                                                   float* __restrict__ next_obs_row, float* __restrict__ rewards_row, float* __restrict__ dones_row,
                                                                   float* __restrict__ terminated, float* __restrict__ cur_rewards, float* __restrict__ cur_lengths,
                                                                   double* __restrict__ acc, double* __restrict__ sub_acc) {
    if (blockIdx.x > 0) {
        const int64_t total = n * obs_dim, nb = gridDim.x - 1, bi = blockIdx.x - 1;
        if ((((uintptr_t)obs | (uintptr_t)next_obs_row) & 15) == 0 && (total & 3) == 0) {
            const float4* s4 = (const float4*)obs;
            float4* d4 = (float4*)next_obs_row;
            for (int64_t i = bi * BLOCK + threadIdx.x; i < total / 4; i += nb * BLOCK) {
                float4 v = s4[i];
                v.x = clamp_torch(v.x, -clip_obs, clip_obs);
                v.y = clamp_torch(v.y, -clip_obs, clip_obs);
                v.z = clamp_torch(v.z, -clip_obs, clip_obs);
                v.w = clamp_torch(v.w, -clip_obs, clip_obs);
                d4[i] = v;
            }
        } else {
            for (int64_t i = bi * BLOCK + threadIdx.x; i < total; i += nb * BLOCK) next_obs_row[i] = clamp_torch(obs[i], -clip_obs, clip_obs);
        }
        return;
    }
    constexpr int NV = 4 + CTL_PPO_MAX_SUB_REWARDS;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += BLOCK) {
        const float r = rew[e], d = (float)reset[e];
        const bool done = reset[e] != 0;
        const float cr = cur_rewards[e] + r, cl = cur_lengths[e] + 1.f;
        rewards_row[e] = r;
        dones_row[e] = d;
        terminated[e] = (float)terminate[e];
        v[0] += done ? 1.0 : 0.0;
        v[1] += done ? (double)cr : 0.0;
        v[2] += done ? (double)cl : 0.0;
        v[3] += (double)r;
#pragma unroll
        for (int k = 0; k < CTL_PPO_MAX_SUB_REWARDS; ++k)
            if (k < S) v[4 + k] += (double)sub_rewards[e * S + k];
        const float not_done = 1.f - d;
        cur_rewards[e] = cr * not_done;
        cur_lengths[e] = cl * not_done;
    }
    __shared__ double red[ROWS_PER_BLOCK][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < 4 + S) {
        const int k = threadIdx.x;
        const double s = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        if (k < 4) acc[k] += s;
        else sub_acc[k - 4] += s;
    }
}

// one wave per row, grid-stride over groups of four rows; partials[block * NSTAT + k]
__global__ __launch_bounds__(BLOCK) void ppo_loss_kernel(const v2p_ppo_loss_cfg c, int64_t B, const v2p_ppo_loss_buffers b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int A = c.num_actions;
    const float lo = (float)(1.0 - c.e_clip), hi = (float)(1.0 + c.e_clip), ec = (float)c.e_clip;
    const float inv_b = 1.f / (float)B;
    float sg[2] = {1.f, 1.f}, os[2] = {1.f, 1.f}, ls = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < A) {
            sg[h] = b.sigma[k];
            os[h] = b.old_sigma[k];
            ls += b.logstd[k];
        }
    }
    ls = wave_sum(ls);
    const float nlp_const = (float)(HALF_LOG_2PI * A);
    double part[NSTAT];
#pragma unroll
    for (int k = 0; k < NSTAT; ++k) part[k] = 0.0;
    const float nanv = __builtin_nanf("");
    for (int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + wave; r < B; r += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        const int64_t j = b.idx ? b.idx[r] : r;
        if (j < 0 || j >= c.dataset_rows) {  // (uniform over the wave)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (lane + 64 * h < A) b.grad_mu[r * A + lane + 64 * h] = nanv;
            if (lane == 0) b.grad_value[r] = nanv;
#pragma unroll
            for (int k = 0; k < NSTAT; ++k) part[k] += (double)nanv;
            continue;
        }
        float m[2], t[2], gb[2];
        float q = 0.f, kl = 0.f, bl = 0.f, dr = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = lane + 64 * h;
            m[h] = t[h] = gb[h] = 0.f;
            if (k < A) {
                const float mk = b.mu[r * A + k], s = sg[h], o = os[h];
                const float tk = (b.actions[j * A + k] - mk) / s;
                q += tk * tk;
                const float dm = b.old_mu[j * A + k] - mk;
                const float c1 = logf(o / s + 1e-5f);
                const float c2 = (s * s + dm * dm) / (2.f * (o * o + 1e-5f));
                kl += c1 + c2 - 0.5f;
                float g = 0.f;
                if (c.has_bounds_loss) {
                    float up = mk - 1.f, dn = mk + 1.f;
                    up = up < 0.f ? 0.f : up;  // clamp_min(mu - 1, 0)
                    dn = dn > 0.f ? 0.f : dn;  // clamp_max(mu + 1, 0)
                    bl += dn * dn + up * up;
                    g = c.bounds_loss_coef * (2.f * (up + dn));
                }
                if (k >= c.c0 && k < c.c1) {
                    dr += mk * mk;
                    g += c.dof_res_weight * (2.f * mk);
                }
                m[h] = mk;
                t[h] = tk;
                gb[h] = g;
            }
        }
        q = wave_sum(q);
        kl = wave_sum(kl);
        bl = wave_sum(bl);
        dr = wave_sum(dr);
        const float nlp = 0.5f * q + nlp_const + ls;
        const float ratio = expf(b.old_neglogp[j] - nlp);
        const float adv = b.advantages[j];
        const float x = -(adv * ratio), y = -(adv * clamp_torch(ratio, lo, hi));
        const float al = x > y ? x : y;
        // autograd: the max hands its gradient to the larger side and splits it on a tie; the clamp passes it inside its inclusive bounds
        const float gx = x > y ? 1.f : (x == y ? 0.5f : 0.f), gy = 1.f - gx;
        const bool inside = ratio >= lo && ratio <= hi;
        const float d_ratio = gx * -adv + (inside ? gy * -adv : 0.f);
        const float d_nlp = d_ratio * -ratio;  // ratio = exp(old - neglogp)
        const float v = b.value[r], ret = b.returns[j];
        const float dv = ret - v;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = lane + 64 * h;
            if (k < A) b.grad_mu[r * A + k] = inv_b * (d_nlp * -(t[h] / sg[h]) + gb[h]);  // d neglogp / d mu = -(a - mu) / sigma^2
        }
        if (lane == 0) b.grad_value[r] = inv_b * (c.critic_coef * (2.f * (v - ret)));
        part[0] += (double)al;
        part[1] += (double)(dv * dv);
        part[2] += (double)bl;
        part[3] += (double)dr;
        part[4] += fabsf(ratio - 1.f) > ec ? 1.0 : 0.0;
        part[5] += (double)kl;
    }
    __shared__ double red[ROWS_PER_BLOCK][NSTAT];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NSTAT; ++k) red[wave][k] = part[k];
    }
    __syncthreads();
    if (threadIdx.x < NSTAT) {
        const int k = threadIdx.x;
        b.partials[(int64_t)blockIdx.x * NSTAT + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// one workgroup of 64: thread k < NSTAT adds the partials of statistic k in workgroup order; thread NSTAT takes the entropy
__global__ __launch_bounds__(64) void ppo_loss_reduce_kernel(const v2p_ppo_loss_cfg c, int64_t B, int blocks, const v2p_ppo_loss_buffers b) {
    __shared__ double mean[NSTAT + 1];
    const int k = threadIdx.x;
    if (k < NSTAT) {
        double s = 0.0;
        for (int i = 0; i < blocks; ++i) s += b.partials[(int64_t)i * NSTAT + k];
        mean[k] = s / (double)B;
    } else if (k == NSTAT) {
        // Normal(mu, sigma).entropy().sum(-1): the same for every row under a fixed sigma.  One thread, once per launch: taken in float64
        // (0.5 + 0.5 log(2 pi) and log(sigma) nearly cancel where sigma is near 0.24; a float32 log would leave its last bit in the sum)
        double ent = 0.0;
        for (int i = 0; i < c.num_actions; ++i) ent += (0.5 + HALF_LOG_2PI) + log((double)b.sigma[i]);
        mean[NSTAT] = ent;
    }
    __syncthreads();
    if (k < NSTAT) b.stats[k] = mean[k];
    if (k == NSTAT) {
        b.stats[6] = mean[NSTAT];
        b.stats[7] = mean[0] + (double)c.critic_coef * mean[1] - (double)c.entropy_coef * mean[NSTAT] + (c.has_bounds_loss ? (double)c.bounds_loss_coef * mean[2] : 0.0) +
                     (double)c.dof_res_weight * mean[3];
    }
}

}  // namespace

int launch_ctl_policy_head(int64_t n, int32_t num_actions, const float* mu, const float* logstd, const float* sigma, const float* noise, float clip_actions,
                           float* actions_row, float* mus_row, float* sigmas_row, float* neglogp_row, float* actions_clamped, hipStream_t s) {
    if (n <= 0) return V2P_OK;
    hipLaunchKernelGGL(ctl_policy_head_kernel, dim3((unsigned)((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(BLOCK), 0, s, n, (int)num_actions, mu, logstd, sigma,
                       noise, clip_actions, actions_row, mus_row, sigmas_row, neglogp_row, actions_clamped);
    return check_hip(hipGetLastError(), "ctl_policy_head_kernel");
}

int launch_ctl_rollout_record(int64_t n, int64_t obs_dim, int32_t num_sub, float clip_obs, const float* obs, const float* rew, const int64_t* reset,
                              const int64_t* terminate, const float* sub_rewards, float* next_obs_row, float* rewards_row, float* dones_row, float* terminated,
                              float* cur_rewards, float* cur_lengths, double* acc, double* sub_acc, hipStream_t s) {
    if (n <= 0) return V2P_OK;
    const int64_t total = n * obs_dim;
    int64_t copy_blocks = (total / 4 + 1023) / 1024;  // ~4 float4 per thread
    copy_blocks = copy_blocks < 1 ? 1 : (copy_blocks > 4096 ? 4096 : copy_blocks);
    hipLaunchKernelGGL(ctl_rollout_record_kernel, dim3((unsigned)(1 + copy_blocks)), dim3(BLOCK), 0, s, n, obs_dim, (int)num_sub, clip_obs, obs, rew, reset, terminate,
                       sub_rewards, next_obs_row, rewards_row, dones_row, terminated, cur_rewards, cur_lengths, acc, sub_acc);
    return check_hip(hipGetLastError(), "ctl_rollout_record_kernel");
}

int launch_ppo_loss(const v2p_ppo_loss_cfg& c, int64_t B, const v2p_ppo_loss_buffers& b, hipStream_t s) {
    if (B <= 0) return V2P_OK;
    int64_t blocks = (B + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    if (blocks > V2P_PPO_LOSS_MAX_BLOCKS) blocks = V2P_PPO_LOSS_MAX_BLOCKS;
    hipLaunchKernelGGL(ppo_loss_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, c, B, b);
    int rc = check_hip(hipGetLastError(), "ppo_loss_kernel");
    if (rc != V2P_OK) return rc;
    hipLaunchKernelGGL(ppo_loss_reduce_kernel, dim3(1), dim3(64), 0, s, c, B, (int)blocks, b);
    return check_hip(hipGetLastError(), "ppo_loss_reduce_kernel");
}

}  // namespace v2p
