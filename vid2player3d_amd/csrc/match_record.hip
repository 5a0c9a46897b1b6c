// The record of a match run (vid2player/env/tasks/mvae_controller_vis_dual.py:156-195, MVAEControllerVisDual.render_vis with
// cfg env.record): every control step each env's frame goes to slot `progress_buf` of its own L slots, and when pairs finish the
// rallies with the largest summed `_distance` are kept - here without the reference's six .cpu() copies, its nonzero() and its host
// lists.  Three kernels, two entries:
//
//   v2p_match_record_frame   match_record_frame_kernel: one wave64 per env, TT_WPB envs per workgroup, shaped like tennis_eval_kernel.
//                            The pose row is tennis_pose_dev.hpp's (the evaluation step's lines); the arithmetic is built like that
//                            unit's, without FMA contraction.  An env whose progress is outside [0, L) stores nothing and raises its
//                            word of `overflow`.
//   v2p_match_record_select  match_record_select_kernel: ONE workgroup scans the n/2 pairs for the finished pair with the largest
//                            float32 sum of the two `_distance` words (lowest index among equals), thread 0 then runs the reference's
//                            insertion on the best tables and writes the decision {pair or -1, storage slot, nframes};
//                            match_record_copy_kernel: one wave per frame of the 2 x L the pair may hold, returns at once on -1, else
//                            copies slots [0, nframes) of both envs into the storage slot.  Ranks move through best_slot, frames never.
//
// Plain vector stores, no atomics: an env's slots, the tables (thread 0 of the one workgroup) and a storage slot's frames each have one
// writer per launch, so two runs give the same bits.
#include <limits.h>

#include "match_record.hpp"
#include "tennis_pose_dev.hpp"
#include "tennis_task_dev.hpp"

namespace v2p {

namespace {

constexpr int MR_SELECT_THREADS = 1024;  // the one workgroup of the selection: 16 waves
constexpr int MR_COPY_WPB = 4;           // frames (waves) per workgroup of the copy

struct MatchRecordArgs {
    v2p_match_record_buffers b;
    int64_t n, length;
    int32_t num_best;
    uint64_t body_of_smpl[TE_JOINTS / TE_PACK];
};

__global__ __launch_bounds__(TT_WAVE* TT_WPB) void match_record_frame_kernel(const MatchRecordArgs h) {
    const int lane = threadIdx.x & (TT_WAVE - 1);
    const int64_t e = (int64_t)blockIdx.x * TT_WPB + (threadIdx.x >> 6);
    if (e >= h.n) return;  // (the whole wave)
    const v2p_match_record_buffers& b = h.b;
    const int64_t p = b.progress[e];
    if (p < 0 || p >= h.length) {  // the reference would raise (or, below zero, wrap): nothing outside the env's own L slots is written
        if (lane == 0) b.overflow[e] = 1;
        return;
    }
    const int64_t at = e * h.length + p;
    const float* rb = b.rb_state + e * (V2P_NUM_BODIES * 13);
    const float* ball = b.ball_state + e * 13;
    te_pose_row(rb, b.dof_state, e, h.body_of_smpl, lane, TT_WAVE, b.joint_rot_all, at);
    if (lane < 3) {
        b.root_pos_all[at * 3 + lane] = rb[lane];
        b.ball_pos_all[at * 3 + lane] = ball[lane];
    }
    if (lane == 0) {
        b.phase_all[at] = b.phase_pred[e];
        b.swing_type_all[at] = b.swing_type_cycle[e];
        b.tar_action_all[at] = b.tar_action[e];
    }
}

// the better of two candidates (distance, pair): the larger distance, the lower pair among equals; (-inf, INT_MAX) is "none"
__device__ inline void mr_better(float& d, int& k, float od, int ok) {
    if (od > d || (od == d && ok < k)) { d = od; k = ok; }
}

__global__ __launch_bounds__(MR_SELECT_THREADS) void match_record_select_kernel(const MatchRecordArgs h) {
    __shared__ float wave_d[MR_SELECT_THREADS / TT_WAVE];
    __shared__ int wave_k[MR_SELECT_THREADS / TT_WAVE];
    const v2p_match_record_buffers& b = h.b;
    const int pairs = (int)(h.n / 2);
    float d = -INFINITY;
    int k = INT_MAX;
    for (int i = threadIdx.x; i < pairs; i += MR_SELECT_THREADS) {
        const bool done = (b.reset[2 * (int64_t)i] != 0) || (b.reset[2 * (int64_t)i + 1] != 0);
        const float sum = b.distance[2 * (int64_t)i] + b.distance[2 * (int64_t)i + 1];
        if (done && sum == sum) mr_better(d, k, sum, i);  // (a NaN sum is no candidate)
    }
    for (int m = TT_WAVE / 2; m > 0; m >>= 1) mr_better(d, k, __shfl_xor(d, m, TT_WAVE), __shfl_xor(k, m, TT_WAVE));
    if ((threadIdx.x & (TT_WAVE - 1)) == 0) {
        wave_d[threadIdx.x >> 6] = d;
        wave_k[threadIdx.x >> 6] = k;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < MR_SELECT_THREADS / TT_WAVE; ++w) mr_better(d, k, wave_d[w], wave_k[w]);

    // mvae_controller_vis_dual.py:169-195 on the tables: only this one pair is considered
    int pair = -1, slot = -1, nframes = 0;
    const int K = h.num_best;
    int count = b.best_count[0];
    count = count < 0 ? 0 : (count > K ? K : count);
    if (k != INT_MAX && (count == 0 || d > b.best_distance[count - 1])) {
        int pos = 0;
        while (pos < count && !(d > b.best_distance[pos])) ++pos;  // in front of the first entry it beats: equal entries stay ahead
        const int64_t progress = b.progress[2 * (int64_t)k];
        pair = k;
        nframes = (int)(progress < 0 ? 0 : (progress > h.length ? h.length : progress));
        slot = count < K ? count : b.best_slot[K - 1];  // a free storage slot, or the evicted entry's
        slot = slot < 0 ? 0 : (slot > K - 1 ? K - 1 : slot);
        const int kept = count < K ? count + 1 : K;
        for (int r = kept - 1; r > pos; --r) {
            b.best_distance[r] = b.best_distance[r - 1];
            b.best_pair[r] = b.best_pair[r - 1];
            b.best_nframes[r] = b.best_nframes[r - 1];
            b.best_slot[r] = b.best_slot[r - 1];
        }
        b.best_distance[pos] = d;
        b.best_pair[pos] = pair;
        b.best_nframes[pos] = nframes;
        b.best_slot[pos] = slot;
        b.best_count[0] = kept;
    }
    b.decision[0] = pair;
    b.decision[1] = slot;
    b.decision[2] = nframes;
}

__global__ __launch_bounds__(TT_WAVE* MR_COPY_WPB) void match_record_copy_kernel(const MatchRecordArgs h) {
    const v2p_match_record_buffers& b = h.b;
    const int pair = b.decision[0];
    if (pair < 0) return;
    const int lane = threadIdx.x & (TT_WAVE - 1);
    const int64_t f = (int64_t)blockIdx.x * MR_COPY_WPB + (threadIdx.x >> 6);  // frame f of the 2 x L
    if (f >= 2 * h.length) return;
    const int64_t side = f / h.length, i = f % h.length;
    const int slot = b.decision[1], nframes = b.decision[2];
    if (i >= nframes || (int64_t)pair >= h.n / 2 || slot < 0 || slot >= h.num_best) return;
    const int64_t src = (2 * (int64_t)pair + side) * h.length + i, dst = (2 * (int64_t)slot + side) * h.length + i;
    for (int c = lane; c < TE_JOINTS * 3; c += TT_WAVE) b.best_joint_rot[dst * (TE_JOINTS * 3) + c] = b.joint_rot_all[src * (TE_JOINTS * 3) + c];
    if (lane < 3) {
        b.best_root_pos[dst * 3 + lane] = b.root_pos_all[src * 3 + lane];
        b.best_ball_pos[dst * 3 + lane] = b.ball_pos_all[src * 3 + lane];
    }
    if (lane == 0) {
        b.best_phase[dst] = b.phase_all[src];
        b.best_swing_type[dst] = b.swing_type_all[src];
        b.best_tar_action[dst] = b.tar_action_all[src];
    }
}

MatchRecordArgs fill(const v2p_match_record_cfg& c, int64_t n, const v2p_match_record_buffers& b) {
    MatchRecordArgs h;
    h.b = b;
    h.n = n;
    h.length = c.record_length;
    h.num_best = c.num_best;
    te_pack_body_of_smpl(c.body_of_smpl, h.body_of_smpl);
    return h;
}

}  // namespace

int match_record_body_fault(const v2p_match_record_cfg& c) { return te_body_of_smpl_fault(c.body_of_smpl); }

int launch_match_record_frame(const v2p_match_record_cfg& c, int64_t n, const v2p_match_record_buffers& b, hipStream_t s) {
    const MatchRecordArgs h = fill(c, n, b);
    const dim3 grid((unsigned)((n + TT_WPB - 1) / TT_WPB)), block(TT_WAVE * TT_WPB);
    hipLaunchKernelGGL(match_record_frame_kernel, grid, block, 0, s, h);
    return check_hip(hipGetLastError(), "match_record_frame_kernel");
}

int launch_match_record_select(const v2p_match_record_cfg& c, int64_t n, const v2p_match_record_buffers& b, hipStream_t s) {
    const MatchRecordArgs h = fill(c, n, b);
    hipLaunchKernelGGL(match_record_select_kernel, dim3(1), dim3(MR_SELECT_THREADS), 0, s, h);
    const int rc = check_hip(hipGetLastError(), "match_record_select_kernel");
    if (rc != V2P_OK) return rc;
    const dim3 grid((unsigned)((2 * c.record_length + MR_COPY_WPB - 1) / MR_COPY_WPB)), block(TT_WAVE * MR_COPY_WPB);
    hipLaunchKernelGGL(match_record_copy_kernel, grid, block, 0, s, h);
    return check_hip(hipGetLastError(), "match_record_copy_kernel");
}

}  // namespace v2p
