// The action part of the tennis controller's pre_physics_step (vid2player/env/tasks/physics_mvae_controller.py:247-266) in one launch:
// the copy of the policy's actions, the scaled latent, the scaled residual-DoF and residual-root columns, and - the reason this is a
// kernel - `random_walk_in_recovery` (:252-257): the latent of an env in recovery (tar_action == 0) is replaced by clamp(N(0,1), -5, 5),
// after vae_action_scale has been applied, so the scale does not reach the drawn values.
//
// The reference sizes a slice by a host read (in_recovery.sum()) and deals draw k to the k-th recovery env.  Here env i owns its draws:
// the counter-based generator of philox.hpp makes them from (seed, call, env, block), whatever the other envs do.  Both are iid draws.
//
// Eight lanes per env, 32 envs per workgroup of 256.  Lane g of an env holds latent columns 4g .. 4g+3: one generator block, two
// Box-Muller pairs.  It also carries the columns behind the latent (at most a handful) g, g + 8, ...  The launch is bound by its own
// latency: 8192 envs are 1 MB in and 2 MB out.  `words` [N,32], when given, stands in for the generator's output and nothing else
// changes: one code path follows the word fetch (the tests and the numpy statement meet there).
//
// Built without FMA contraction like tennis_task.hip: the products are torch's `actions[:, a:b] * scale` on float32, bit for bit.
#include "controller_actions.hpp"
#include "philox.hpp"

namespace v2p {

namespace {

constexpr int CA_LANES = 8;   // lanes of an env
constexpr int CA_BLOCK = 256;
constexpr int CA_LATENT = V2P_MVAE_LATENT;
static_assert(CA_LANES * 4 == CA_LATENT, "a lane holds one four-word block of the latent");

struct ControllerActionsArgs {
    v2p_controller_actions_cfg c;
    v2p_controller_actions_buffers b;
    int64_t n;
};

__global__ __launch_bounds__(CA_BLOCK) void controller_actions_kernel(const ControllerActionsArgs a) {
    const int64_t t = (int64_t)blockIdx.x * CA_BLOCK + threadIdx.x;
    const int64_t e = t / CA_LANES;
    const int g = (int)(t % CA_LANES);
    if (e >= a.n) return;
    const v2p_controller_actions_cfg& c = a.c;
    const v2p_controller_actions_buffers& b = a.b;
    const int nr = c.num_res_dof, nroot = c.num_res_root, width = CA_LATENT + nr + nroot;
    const float* in = b.actions + e * b.actions_stride;
    float* copy = b.actions_out + e * (int64_t)width;

    float x[4], z[4];
    for (int i = 0; i < 4; ++i) x[i] = in[4 * g + i];
    for (int i = 0; i < 4; ++i) copy[4 * g + i] = x[i];
    for (int i = 0; i < 4; ++i) z[i] = x[i] * c.vae_action_scale;
    if (c.random_walk && b.tar_action[e] == 0) {
        uint32_t w[4];
        if (b.words) {
            for (int i = 0; i < 4; ++i) w[i] = b.words[e * CA_LATENT + 4 * g + i];
        } else {
            philox_block(c.seed, c.call, PHILOX_STREAM_WALK, (uint32_t)e, (uint32_t)g, w);
        }
        philox_normal_pair(w[0], w[1], &z[0], &z[1]);
        philox_normal_pair(w[2], w[3], &z[2], &z[3]);
        for (int i = 0; i < 4; ++i) z[i] = philox_clamp(z[i], c.clamp);
    }
    for (int i = 0; i < 4; ++i) b.mvae_actions[e * CA_LATENT + 4 * g + i] = z[i];

    for (int k = g; k < nr + nroot; k += CA_LANES) {
        const float v = in[CA_LATENT + k];
        copy[CA_LATENT + k] = v;
        if (k < nr) b.res_dof_actions[e * (int64_t)nr + k] = v * c.residual_dof_scale;
        else b.res_root_actions[e * (int64_t)nroot + (k - nr)] = v * c.residual_root_scale;
    }
}

}  // namespace

int launch_controller_actions(const v2p_controller_actions_cfg& c, int64_t n, const v2p_controller_actions_buffers& b, hipStream_t s) {
    ControllerActionsArgs a;
    a.c = c;
    a.b = b;
    a.n = n;
    const int64_t threads = n * CA_LANES;
    const dim3 grid((unsigned)((threads + CA_BLOCK - 1) / CA_BLOCK)), block(CA_BLOCK);
    hipLaunchKernelGGL(controller_actions_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "controller_actions_kernel");
}

}  // namespace v2p
