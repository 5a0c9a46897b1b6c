// The two-player motion generator's reset by flags: v2p_mvae_dual_reset_flagged is `reset_dual` under `_is_dual` (v2p_mvae_dual_reset,
// mvae_player_dual.hip) for every env whose flag is up, in one launch over all envs - no id list, no gather of the ready and serve
// frames, no draw made by the host.  The caller raises both flags of a finished pair (v2p_ctl_pair_reset_begin makes a mask whole).
//
// The law is the reset text of mvae_rows.inc (MV_TEXT_RESET), included once more, with the side macros of mvae_dual_reset_kernel - a
// row is normalised with the statistics of its own side (env & 1), every reset env walks the batch's ONE racket object - and the
// register-resident view of mvae_player_flagged.hip: entry e is env e, and the start is held in two registers (the row of the caller's
// table, or the kernel's own draw, or the centre).  The side's avg and std are both read and then one is chosen - a choice between the
// two weight structs themselves is a choice of address (DESIGN.md item 15 records what that form cost in LDS and scratch).
//
// init_feature is [num_envs,288] by ENV: the caller interleaves the serve and ready frames by parity and serve_from once.
// joint_pos_bind_rel is ONE [24,3] row: the id-list form reads the row of a pair's POSITION in the list, which without a list would be a
// prefix count of the flagged pairs - the C ABI refuses bind_rows > 1.
//
// A unit of its own: every kernel of mvae_player_dual.hip and mvae_player_flagged.hip must stay the machine code it was.
#include "mvae_player_dev.hpp"
#include "pair_reset.hpp"
#include "philox.hpp"

namespace v2p {

namespace {

struct MvDualFlagArgs {
    v2p_mvae_cfg c;                                // side 0's: the text reads is_train, on which the sides agree
    const float *avg0, *std0, *avg1, *std1;        // [288] each: the statistics of side 0 and of side 1
    v2p_mvae_buffers b;
    v2p_mvae_racket racket;
    const int64_t* flags;                          // [num_envs]
    const float *init_feature, *root_xy, *bind;    // [num_envs,288], [num_envs,2] or null, [24,3]
    v2p_mvae_root_rule rule;                       // read where root_xy is null
    int64_t num_envs;
};

// what the reset text indexes as lists, for a launch in which entry e is env e (as in mvae_player_flagged.hip)
struct MvOwnRow {
    __device__ int64_t operator[](int64_t i) const { return i; }
};
struct MvStart {  // element 2 i + k of the wave's env: component k (both read, then one chosen)
    float x, y;
    __device__ float operator[](int64_t k) const {
        const float vx = x, vy = y;
        return (k & 1) ? vy : vx;
    }
};
struct MvFlagView {  // (values only: the view lives in registers)
    MvOwnRow env_ids;
    const float* init_feature;
    MvStart root_xy;
    int64_t num_envs;
    v2p_mvae_buffers b;
};
struct MvSideStats {  // what the text reads of MV_SIDE_W
    const float *avg, *std;
};

// one wave per env: lanes stride the columns, lanes 0..23 take a joint each, lane 0 walks the racket's chain
__global__ __launch_bounds__(256) void mvae_dual_reset_flagged_kernel(const MvDualFlagArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= g.num_envs) return;  // (the whole wave)
    if (g.flags[i] == 0) return;  // (the whole wave)
    MvStart start = {0.f, -13.f};  // the centre of the baseline
    if (g.root_xy) {
        start.x = g.root_xy[i * 2];
        start.y = g.root_xy[i * 2 + 1];
    } else if (g.rule.rule == V2P_MVAE_ROOT_DRAW) {
        uint32_t words[4];
        philox_block(g.rule.seed, g.rule.call, PHILOX_STREAM_ROOT, (uint32_t)i, 0, words);
        start.x = (philox_uniform(words[0]) - 0.5f) * 2.0f + 0.0f;
        start.y = (philox_uniform(words[1]) - 0.5f) * 1.5f + (-13.0f);
    }
    const float *avg0 = g.avg0, *avg1 = g.avg1, *std0 = g.std0, *std1 = g.std1;
    const bool odd = (i & 1) != 0;
    const MvSideStats side = {odd ? avg1 : avg0, odd ? std1 : std0};
    const MvFlagView a = {MvOwnRow(), g.init_feature, start, g.num_envs, g.b};
#define MV_TEXT_RESET
#define MV_SIDE_W side
#define MV_SIDE_C g.c
#define MV_RACKET_RIGHTHAND g.racket.righthand
#define MV_RACKET_DIR(k) g.racket.dir[k]
#define MV_RACKET_NORMAL(k) g.racket.normal[k]
#define MV_BIND g.bind
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

int launch_mvae_dual_reset_flagged(const v2p_mvae_cfg (&c)[2], int64_t num_envs, const v2p_mvae_weights (&w)[2], const v2p_mvae_buffers& b, const v2p_mvae_racket& racket,
                                   const int64_t* flags, const float* init_feature, const float* root_xy, const v2p_mvae_root_rule& rule, const float* joint_pos_bind_rel,
                                   hipStream_t s) {
    MvDualFlagArgs g = {};
    g.c = c[0]; g.b = b; g.racket = racket;
    g.avg0 = w[0].avg; g.std0 = w[0].std; g.avg1 = w[1].avg; g.std1 = w[1].std;
    g.flags = flags; g.init_feature = init_feature; g.root_xy = root_xy; g.bind = joint_pos_bind_rel;
    g.rule = rule;
    g.num_envs = num_envs;
    const dim3 grid((unsigned)((num_envs + 3) / 4)), block(256);
    hipLaunchKernelGGL(mvae_dual_reset_flagged_kernel, grid, block, 0, s, g);
    return check_hip(hipGetLastError(), "mvae_dual_reset_flagged_kernel");
}

}  // namespace v2p
