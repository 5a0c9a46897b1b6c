// The launch policy of the link-per-lane schedule, in one place: the schedule state of a batch (v2p_env::sched) and the decisions as
// pure functions of plain values - no v2p_env, no HIP, no globals: a host-only C++ program can include this header alone
// (tests/test_ll_schedule.py).  What applies them to a batch and to the arguments of a launch is physics_ll_host.hip.
#pragma once
#include <stdint.h>

namespace v2p {

// ---------------------------------------------------------------------------- the engine's schedule defaults
// What the engine takes where v2p_sim_cfg leaves a schedule field to it - the ONE statement of that policy: batch creation, the build
// choice of a launch and ball attachment all ask here.
struct EngineDefaults {
    int pair_mix_permille, job_mono_permille;
    int job_len, job_lead;  // 0 / -1: decided launch by launch (job_plan)
    long job_timeout_spins;
};
inline EngineDefaults engine_defaults(int64_t n, bool joint_limits, bool regs_build, bool ball) {
    EngineDefaults d;
    // (mixing trades total work for a shorter critical path: it pays while the launch is as long as its heaviest pair, i.e. up to
    // ~4 env pairs per wave slot; beyond that the launch is throughput bound and pairs of equals are cheaper)
    // (the kernels with joint-limit rows or a ball run 2 waves per SIMD: there pairs of equals measured best, profiles/r02g_racket_ball_sweep.txt)
    const bool mix = n <= 12288 && !joint_limits && !ball;
    // defaults: measured best.  Round 2 (profiles/r02_job_mono_sweep.txt): 250 / 250; re-swept on the round-4 kernel (profiles/r04_mono_mix_sweep.txt:
    // 5 x 4 grid at 8192 envs, then across TGS / djokovic / per-clip shapes / 4096 and 12288 envs): 60 / 150 is +1 .. 2 % everywhere - with the
    // walk the heaviest chains are shorter, fewer pairs need to keep their substeps in one workgroup
    // (the register build runs where a launch is as long as its heaviest wave: there every heavy env takes a light partner, 500 - +1.3 % at 1024
    // and 4096 envs against 150, profiles/r04e_dual_build.txt)
    d.pair_mix_permille = mix ? (regs_build ? 500 : 150) : 0;
    // (above 12288 envs, with joint limits or with a ball - where the heavy x light mix is off - 250 stays 0.2 .. 1 % better)
    d.job_mono_permille = mix ? 60 : 250;
    d.job_len = 0;
    d.job_lead = -1;
    d.job_timeout_spins = 50000l;  // ~20 ms: far beyond the longest chain of substeps of a launch
    return d;
}

// ---------------------------------------------------------------------------- the job plan of a launch
// the job settings of a batch: v2p_sim_cfg, the engine's defaults where the cfg leaves a field to the engine, the device's CU count
struct JobCfg {
    int on;             // v2p_sim_cfg.substep_jobs: the physics launch is cut into (substep, env pair) jobs
    // 1 = the engine decides launch by launch: cutting pays once the env pairs no longer fit the GPU's wave slots in one round
    // (CUs x 4 SIMDs x 3 waves; measured: at <= 2/3 of the slots whole control steps per workgroup are 0.3 ... 8 % faster); 2 = always
    int min_blocks;     // ... when it has more env pairs than this (CUs x 8; 0: always)
    int len;            // substeps per job; 0 = the engine decides (2 for launches of >= len2_blocks env pairs, else 1)
    // substeps per job: 1 while the launch is short of jobs, 2 once there are plenty (>= CUs x 32 env pairs: measured crossover at
    // 16384 envs - a job's prologue / hand-over is ~8 % of a one-substep job); v2p_sim_cfg.job_len: A/B switch
    int len2_blocks;
    int lead;           // substeps of the FIRST job of a cut pair (0 = like the others, -1 = the engine decides)
    int mono_permille;  // share of the env pairs (the heaviest) whose substeps stay in one workgroup
};
// One launch of `mono` + jobs_per_pair x (blocks - mono) workgroups, substep-major.  Not cut: mono = blocks (every pair keeps whole
// control steps in one workgroup, nothing is handed over), jobs of length 1.
struct JobPlan {
    bool cut;
    int mono, len, lead;
    unsigned jobs_per_pair, grid;
};
// blocks: env pairs (workgroups of an uncut launch); nsub: substeps per control step; progress: the batch has progress words
inline JobPlan job_plan(const JobCfg& j, unsigned blocks, int nsub, bool ball, bool progress) {
    JobPlan p;
    p.cut = j.on && progress && blocks > 1 && (int)blocks > j.min_blocks;
    p.mono = p.cut ? (int)(blocks * (unsigned)j.mono_permille / 1000u) : (int)blocks;
    p.len = !p.cut ? 1 : (j.len >= 1 ? j.len : (((int)blocks >= j.len2_blocks && nsub % 2 == 0) ? 2 : 1));
    // (lead: substeps of the first job of a cut pair; 0 / out of range = len, i.e. jobs of equal length; -1 = the engine's
    // choice: with one-substep jobs the first job takes two substeps - one hand-over less per pair (a third of the hand-over traffic
    // at four substeps) while the jobs that END a launch stay one substep long; measured +0.3 % at 8192 envs, +1.3 % at 12288, three
    // substeps in the first job -4.7 %: profiles/r04_job_lead.txt)
    // (not with a ball: 12.68 vs 12.79 M)
    const int lead_req = j.lead >= 0 ? j.lead : ((p.len == 1 && nsub >= 4 && !ball) ? 2 : 0);
    p.lead = (p.cut && lead_req >= 1 && lead_req < nsub) ? lead_req : p.len;
    p.jobs_per_pair = 1u + (unsigned)((nsub - p.lead + p.len - 1) / p.len);
    p.grid = (unsigned)p.mono + (blocks - (unsigned)p.mono) * p.jobs_per_pair;
    return p;
}

// ---------------------------------------------------------------------------- the schedule state of a batch
// Device pointers borrow from the batch's DeviceOwner (alloc_env).
struct LlSchedule {
    // pairing (physics_ll_host.hip): envs are handed to waves in descending order of their contact load
    int pair_period;           // 0 = pairing off (v2p_sim_cfg.pair_envs_by_load = 0), else on
    int32_t* pair_key;         // [N] load key of each env after the last physics launch (0..255)
    int32_t* pair_pos;         // [N] arrival index inside its load bin
    int32_t* pair_hist;        // [256] + pair_starts [2][256] + pair_done [1] (one allocation)
    int32_t* pair_done;
    int32_t* perm;             // [N] wave slot -> env of the next physics launch, materialised for v2p_env_debug_pairing only
    int32_t* pair_list[2];     // [256][N] envs of each load bin in arrival order: what the NEXT launch looks its envs up in (double
    int32_t* pair_starts[2];   // [256]    first rank of each bin                  buffered: a launch reads one set and fills the other)
    int pair_buf;              // the set the next launch reads
    int pair_have;             // the last physics launch left (key, pos, start) that have not been scattered into perm yet
    int32_t* pair_slot_env;    // [N] env of each wave slot of the running launch: looked up by the job of the first substep, read by the later ones
    int pair_mix_permille;     // share of the envs (the heaviest) that are paired with the lightest ones instead of with each other
    int pair_mix_default;      // pair_mix_permille was left to the engine (-1)
    // substep jobs
    JobCfg job;
    int job_mono_default;      // job.mono_permille was left at its default (v2p_env_attach_ball moves it)
    int job_interleave;
    long job_timeout_spins;    // see PhysArgs
    int32_t* job_progress;     // [waves + 2] progress word per wave slot, then the recovery and skip counters
    float* job_hand;           // [nsub - 1][N][HAND_FLOATS] the state as one substep job hands it to the next (16-byte chunks), a slot per substep
    int job_epoch;
    // which build of the kernel runs (physics_ll_host.hip: choose_build)
    int ll_regs_build;         // 1: this batch runs the register build of the link-per-lane kernel (two waves per SIMD)
    int kernel_build;          // v2p_sim_cfg.kernel_build (0: ll_regs_build follows the envs resident on the device)
    int build_latched;         // kernel_build 0: the choice is taken at the first launch after creation / after a whole-batch reset and holds until the next one
    int counted_resident;      // this batch is in the device's resident-env count
};

}  // namespace v2p
