// The MotionVAE motion generator of a two-player batch (vid2player/players/mvae_player.py `MVAEPlayer` with `dual_mode: different`):
// v2p_mvae_dual_step and v2p_mvae_dual_reset.  The kernels' bodies are the single player's (mvae_rows.inc), the layers mvae_player_dev.hpp's.
#include "mvae_player_dev.hpp"

namespace v2p {

namespace {

// the two-player kernels': a cfg and a weight set per side (env 2k: side 0, env 2k+1: side 1), one state
struct MvDualArgs {
    v2p_mvae_cfg c0, c1;
    v2p_mvae_weights ws0, ws1;
    v2p_mvae_buffers b;
    const float *latents, *residual;
    const int64_t* env_ids;                        // reset only
    const float *init_feature, *root_xy, *bind;    // reset only
    v2p_mvae_racket racket;                        // reset only
    int64_t n, num_envs, bind_rows;
    int mapping;                                   // step only: V2P_MVAE_DUAL_MAP_*
};

// ---------------------------------------------------------------------------------------------------------------- two players
// `MVAEPlayer.step` under `_is_dual` (mvae_player.py:184-199): env 2k is side 0, env 2k+1 side 1, each side with its own weights,
// statistics, hand and player rule.  A workgroup keeps the single kernel's form and serves 32 envs of ONE side - a tile that mixed the
// sides would load both weight sets and run every MFMA with half its rows dead.  Two mappings of workgroups to sides are
// built: under V2P_MVAE_DUAL_MAP_PARITY workgroup b takes side b & 1 and, of that side's n / 2 envs, rows 32 (b >> 1) .., envs
// 2 (32 (b >> 1) + r) + side; under V2P_MVAE_DUAL_MAP_HALVES the grid's first half takes side 0 and its second half side 1.  The numbers
// are the same bit for bit; which is faster is a measurement (HALVES at 8192 envs, by 3.0 %).  One quirk of the reference is reproduced: its non-init branch writes the root
// columns of EVERY env's condition (:254-262), side 1's call runs last, so those three columns are normalised with side 1's avg and
// std in the even envs too.
__global__ __launch_bounds__(MV_THREADS) void mvae_dual_step_kernel(const MvDualArgs a) {
    __shared__ __attribute__((aligned(16))) float bufA[MV_TILE * MV_XS];
    __shared__ __attribute__((aligned(16))) float bufB[MV_TILE * MV_XS];
    __shared__ __attribute__((aligned(16))) float g1[MV_TILE * MV_GS];
    __shared__ __attribute__((aligned(16))) float g2[MV_TILE * MV_GS];
    __shared__ float coef[MV_TILE * 8];
    __shared__ float s_phase[MV_TILE];
    __shared__ int s_swing[MV_TILE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int half = (int)(gridDim.x >> 1), blk = (int)blockIdx.x;
    const int side = a.mapping == V2P_MVAE_DUAL_MAP_HALVES ? (blk >= half ? 1 : 0) : (blk & 1);
    const int64_t row0 = (int64_t)(a.mapping == V2P_MVAE_DUAL_MAP_HALVES ? (blk >= half ? blk - half : blk) : (blk >> 1)) * MV_TILE;
    const int64_t side_n = a.n >> 1;  // (n is even)
    const int rows = (int)((side_n - row0) < MV_TILE ? (side_n - row0) : MV_TILE);
    const v2p_mvae_weights sw = side ? a.ws1 : a.ws0;
    const v2p_mvae_cfg sc = side ? a.c1 : a.c0;

#define MV_TEXT_STEP
#define MV_ENV(row) (2 * (row0 + row) + side)
#define MV_SIDE_W sw
#define MV_SIDE_C sc
#define MV_ROOT_AVG a.ws1.avg
#define MV_ROOT_STD a.ws1.std
#include "mvae_rows.inc"
#undef MV_ROOT_STD
#undef MV_ROOT_AVG
#undef MV_SIDE_C
#undef MV_SIDE_W
#undef MV_ENV
#undef MV_TEXT_STEP
}

// `reset_dual` under `_is_dual` (:167-180) for a list of whole pairs, ascending: a row is normalised with its own side's statistics; the
// racket is ONE object for both sides (:56-57: the server's hand and grip), and `infer_with_fk` reads joint_pos_bind_rel[:batch] by the
// position in a side's sub-list - the pair at list positions 2i, 2i + 1 reads row i
__global__ __launch_bounds__(256) void mvae_dual_reset_kernel(const MvDualArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;  // (the whole wave)
    const float* bind = a.bind + (a.bind_rows > 1 ? (i >> 1) * (MV_JOINTS * 3) : 0);
#define MV_TEXT_RESET
#define MV_SIDE_W (e & 1 ? a.ws1 : a.ws0)
#define MV_SIDE_C a.c0
#define MV_RACKET_RIGHTHAND a.racket.righthand
#define MV_RACKET_DIR(k) a.racket.dir[k]
#define MV_RACKET_NORMAL(k) a.racket.normal[k]
#define MV_BIND bind
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

int launch_mvae_dual_step(const v2p_mvae_cfg (&c)[2], int64_t n, const v2p_mvae_weights (&w)[2], const v2p_mvae_buffers& b, const float* latents, const float* residual,
                          int mapping, hipStream_t s) {
    MvDualArgs a = {};
    a.c0 = c[0]; a.c1 = c[1]; a.ws0 = w[0]; a.ws1 = w[1]; a.b = b;
    a.latents = latents; a.residual = residual;
    a.n = a.num_envs = n;
    a.mapping = mapping;
    const dim3 grid((unsigned)(2 * ((n / 2 + MV_TILE - 1) / MV_TILE))), block(MV_THREADS);
    hipLaunchKernelGGL(mvae_dual_step_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "mvae_dual_step_kernel");
}

int launch_mvae_dual_reset(const v2p_mvae_cfg (&c)[2], int64_t num_envs, const v2p_mvae_weights (&w)[2], const v2p_mvae_buffers& b, const v2p_mvae_racket& racket,
                           const int64_t* env_ids, int64_t n_ids, const float* init_feature, const float* root_xy, const float* joint_pos_bind_rel, int64_t bind_rows,
                           hipStream_t s) {
    MvDualArgs a = {};
    a.c0 = c[0]; a.c1 = c[1]; a.ws0 = w[0]; a.ws1 = w[1]; a.b = b; a.racket = racket;
    a.env_ids = env_ids; a.init_feature = init_feature; a.root_xy = root_xy; a.bind = joint_pos_bind_rel; a.bind_rows = bind_rows;
    a.n = n_ids; a.num_envs = num_envs;
    const dim3 grid((unsigned)((n_ids + 3) / 4)), block(256);
    hipLaunchKernelGGL(mvae_dual_reset_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "mvae_dual_reset_kernel");
}

}  // namespace v2p
