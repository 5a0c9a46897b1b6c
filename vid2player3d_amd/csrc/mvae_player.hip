// The MotionVAE motion generator of a control step (vid2player/players/mvae_player.py `MVAEPlayer.step` / `reset`, around
// motion_vae/model.py:186-252 `MixedDecoder.forward`): v2p_mvae_step is the gate, the three expert-blended layers and
// `_update_mvae_state(init=False)` in one launch; v2p_mvae_reset is `_update_mvae_state(init=True)` for a list of env ids.
//
// The decoder.  The reference blends the six experts' weights per env and multiplies with one matrix per env (239,168 blended weights
// per env, written and read back).  Here every expert is computed and the RESULTS are blended, out = sum_e c_e (x W_e + b_e): the same
// function, a GEMM with shared weights and the blend in its epilogue.  A workgroup of four waves owns MV_TILE = 32 envs.  Its
// activations stay in LDS: two [32][324] buffers hold cat(z, previous) of the layer being read and of the layer being written, and the
// gate has two small ones.  The product runs on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: a k-ordered fmaf chain per output): a
// wave takes a tile of 32 output columns, keeps SIX accumulators - one per expert, 96 registers - and walks K once; lane l feeds
// A[env l&31][k = 2s + (l>>5)] from LDS and B[k][column l&31] from the packed weights.  Both operands are laid out so that four
// consecutive k-steps of a lane are 16 contiguous bytes: the weights are repacked on the host (v2p_rollout.h, v2p_mvae_weights), and the
// LDS buffers store column k of a row at mv_perm(k).  The weights (5.7 MB) are read by every workgroup and stay in L2 / Infinity Cache.
//
// The state update restates torch elementwise float32 code (built without FMA contraction like tennis_task.hip): the same operations in
// the same order.  Eight threads share an env: columns are stored coalesced over the tile, joints are dealt three to a thread.
//
// Where the text is.  The layers, conversions and tables: mvae_player_dev.hpp.  The bodies of the two kernels: mvae_rows.inc, as text,
// shared with the two-player kernels of mvae_player_dual.hip (v2p_mvae_dual_step / _reset) - see there why text and why two units.
#include "mvae_player_dev.hpp"

namespace v2p {

namespace {

// ---------------------------------------------------------------------------------------------------------------- the step
__global__ __launch_bounds__(MV_THREADS) void mvae_step_kernel(const MvArgs a) {
    __shared__ __attribute__((aligned(16))) float bufA[MV_TILE * MV_XS];
    __shared__ __attribute__((aligned(16))) float bufB[MV_TILE * MV_XS];
    __shared__ __attribute__((aligned(16))) float g1[MV_TILE * MV_GS];
    __shared__ __attribute__((aligned(16))) float g2[MV_TILE * MV_GS];
    __shared__ float coef[MV_TILE * 8];
    __shared__ float s_phase[MV_TILE];
    __shared__ int s_swing[MV_TILE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t env0 = (int64_t)blockIdx.x * MV_TILE;
    const int rows = (int)((a.n - env0) < MV_TILE ? (a.n - env0) : MV_TILE);

#define MV_TEXT_STEP
#define MV_ENV(row) (env0 + row)
#define MV_SIDE_W a.w
#define MV_SIDE_C a.c
#define MV_ROOT_AVG avg
#define MV_ROOT_STD sd
#include "mvae_rows.inc"
#undef MV_ROOT_STD
#undef MV_ROOT_AVG
#undef MV_SIDE_C
#undef MV_SIDE_W
#undef MV_ENV
#undef MV_TEXT_STEP
}

// ---------------------------------------------------------------------------------------------------------------- the reset
// one wave per id: lanes stride the columns, lanes 0..23 take a joint each, lane 0 walks the racket's chain
__global__ __launch_bounds__(256) void mvae_reset_kernel(const MvArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;  // (the whole wave)
#define MV_TEXT_RESET
#define MV_SIDE_W a.w
#define MV_SIDE_C a.c
#define MV_RACKET_RIGHTHAND a.c.righthand
#define MV_RACKET_DIR(k) MV_EASTERN_DIR_##k
#define MV_RACKET_NORMAL(k) MV_EASTERN_NORMAL_##k
#define MV_BIND a.bind
#include "mvae_rows.inc"
#undef MV_BIND
#undef MV_RACKET_NORMAL
#undef MV_RACKET_DIR
#undef MV_RACKET_RIGHTHAND
#undef MV_SIDE_C
#undef MV_SIDE_W
#undef MV_TEXT_RESET
}

}  // namespace

int launch_mvae_step(const v2p_mvae_cfg& c, int64_t n, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const float* latents, const float* residual,
                     hipStream_t s) {
    MvArgs a = {};
    a.c = c; a.w = w; a.b = b;
    a.latents = latents; a.residual = residual;
    a.n = a.num_envs = n;
    const dim3 grid((unsigned)((n + MV_TILE - 1) / MV_TILE)), block(MV_THREADS);
    hipLaunchKernelGGL(mvae_step_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "mvae_step_kernel");
}

int launch_mvae_reset(const v2p_mvae_cfg& c, int64_t num_envs, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const int64_t* env_ids, int64_t n_ids,
                      const float* init_feature, const float* root_xy, const float* joint_pos_bind_rel, hipStream_t s) {
    MvArgs a = {};
    a.c = c; a.w = w; a.b = b;
    a.env_ids = env_ids; a.init_feature = init_feature; a.root_xy = root_xy; a.bind = joint_pos_bind_rel;
    a.n = n_ids; a.num_envs = num_envs;
    const dim3 grid((unsigned)((n_ids + 3) / 4)), block(256);
    hipLaunchKernelGGL(mvae_reset_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "mvae_reset_kernel");
}

}  // namespace v2p
