// The motion generator's reset by flags: v2p_mvae_reset_flagged is `MVAEPlayer.reset(env_ids)` (v2p_mvae_reset, mvae_player.hip) for
// every env whose flag is up, in one launch over all envs - no id list, no gather of the initial frames, no draw made by the host.
//
// The law is the single player's reset text (mvae_rows.inc, MV_TEXT_RESET), included a third time.  The text reads a list: entry i is
// env a.env_ids[i], with row i of init_feature and of root_xy.  Here the list is the batch itself - entry e is env e - so the text is
// given a view `a` whose env_ids[i] is i and whose root_xy[2 i + k] is component k of the env's start, already in registers: the row
// of the caller's table, or the kernel's own draw, or the centre.  One wave per env as in mvae_reset_kernel; the flag is wave-uniform,
// so an env that is not flagged costs its wave one load and leaves (nothing in the text synchronises across waves).
//
// The draw restates `MotionVAEPlayer.draw_root_xy` (mvae_player.py:230-236) in float32, each operation rounded on its own (the unit is
// built without FMA contraction): x = (u0 - 0.5) * 2 + 0, y = (u1 - 0.5) * 1.5 + (-13), u0 and u1 = philox_uniform of words 0 and 1 of
// block 0 of stream PHILOX_STREAM_ROOT under (seed, call, env): it depends on those three alone, never on which other envs are flagged
// (device_rng.root_xy_reference is the numpy statement).
//
// A unit of its own: mvae_step_kernel and mvae_reset_kernel must stay the machine code they were (see mvae_player_dev.hpp).
#include "flag_reset.hpp"
#include "mvae_player_dev.hpp"
#include "philox.hpp"

namespace v2p {

namespace {

struct MvFlagArgs {
    v2p_mvae_cfg c;
    v2p_mvae_weights w;
    v2p_mvae_buffers b;
    const int64_t* flags;                          // [num_envs]
    const float *init_feature, *root_xy, *bind;    // [num_envs,288], [num_envs,2] or null, [24,3]
    v2p_mvae_root_rule rule;                       // read where root_xy is null
    int64_t num_envs;
};

// what the reset text indexes as lists, for a launch in which entry e is env e
struct MvOwnRow {
    __device__ int64_t operator[](int64_t i) const { return i; }
};
struct MvStart {  // element 2 i + k of the wave's env: component k (selects, so that the pair stays in registers)
    float x, y;
    __device__ float operator[](int64_t k) const {
        const float vx = x, vy = y;  // (both read, then one chosen: a choice between the two members themselves is a choice of address)
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

// one wave per env: lanes stride the columns, lanes 0..23 take a joint each, lane 0 walks the racket's chain
__global__ __launch_bounds__(256) void mvae_reset_flagged_kernel(const MvFlagArgs g) {
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
    const MvFlagView a = {MvOwnRow(), g.init_feature, start, g.num_envs, g.b};
#define MV_TEXT_RESET
#define MV_SIDE_W g.w
#define MV_SIDE_C g.c
#define MV_RACKET_RIGHTHAND g.c.righthand
#define MV_RACKET_DIR(k) MV_EASTERN_DIR_##k
#define MV_RACKET_NORMAL(k) MV_EASTERN_NORMAL_##k
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

int launch_mvae_reset_flagged(const v2p_mvae_cfg& c, int64_t num_envs, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const int64_t* flags,
                              const float* init_feature, const float* root_xy, const v2p_mvae_root_rule& rule, const float* joint_pos_bind_rel, hipStream_t s) {
    MvFlagArgs g = {};
    g.c = c; g.w = w; g.b = b;
    g.flags = flags; g.init_feature = init_feature; g.root_xy = root_xy; g.bind = joint_pos_bind_rel;
    g.rule = rule;
    g.num_envs = num_envs;
    const dim3 grid((unsigned)((num_envs + 3) / 4)), block(256);
    hipLaunchKernelGGL(mvae_reset_flagged_kernel, grid, block, 0, s, g);
    return check_hip(hipGetLastError(), "mvae_reset_flagged_kernel");
}

}  // namespace v2p
