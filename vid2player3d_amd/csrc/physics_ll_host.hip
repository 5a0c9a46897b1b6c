// The part of the link-per-lane schedule that does not depend on how physics_ll_kernel is built (physics_ll.hip is compiled twice,
// see its head): the launch policy of ll_schedule.hpp applied to a batch (its schedule fields, the choice of kernel build) and to a
// launch (ll_launch_prepare / ll_launch_done, which both launchers of the physics kernel call), the stand-alone pre-physics kernel of
// the staged API and the explicit slot -> env table of the pairing.  Compiled once, with the flags of the default physics_ll.hip
// object (build.py): env_pre_kernel shares namespace strict with the fused prologue of physics_ll_kernel and must round like it.
#include <hip/hip_runtime.h>

#include <atomic>

#include "phys_common.hpp"

namespace v2p {

#include "strict_ops.inc"

// ---- pairing: a wave costs the union of its two envs' contact structure, so envs are handed to waves in descending order of
// their contact load (heavy waves first also keeps the tail of the launch short; the heaviest quarter each next to one of the lightest).
// A counting sort without a sorting kernel: every env draws an arrival index in its load bin at the end of the physics kernel (atomics)
// and appends itself to the bin's arrival list, the workgroup that finishes last scans the 256 bin counts, and the next launch looks
// its envs up (prologue of physics_ll_kernel).  The order inside a bin depends on arrival, which is harmless: an env's arithmetic does
// not depend on the env it shares a wave with (tests: bit-identical results).  The explicit slot -> env table below is built on
// demand only (v2p_env_debug_pairing).
__global__ void pair_scatter_kernel(PairView pv, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) pair_scatter(pv, e);
}

// ---- stand-alone pre-physics (the staged API, v2p_env_pre_physics): one thread per action component
__global__ void env_pre_kernel(PhysArgs a, PairView pv) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = tid / NACT;
    const int c = (int)(tid - e * NACT);
    if (e >= a.n) return;
    if (c == 0 && pv.perm) pair_scatter(pv, e);
    const bool dead = a.reset[e] == 1;
    float act = a.actions[tid];
    if (dead) { act = 0.f; a.actions[tid] = 0.f; }  // in place on the caller's tensor, like the reference
    if (c < NDOF) {
        const float tar = strict::pd_clamp(act, a.x_dof[(e * NDOF + c) * 2], a.p.pd_tar_lim);
        a.pd_target[e * NDOF + c] = tar;
        a.ctrl[CIDX(CT_PD + c)] = tar;
    } else if (c == NDOF || c == NDOF + 3) {
        const float a1 = dead ? 0.f : a.actions[tid + 1], a2 = dead ? 0.f : a.actions[tid + 2];
        const strict::V3 w = strict::residual_wrench(a.x_rb + e * NB * 13 + 3, act, a1, a2, c == NDOF ? a.p.res_force_scale : a.p.res_torque_scale);
        const int base = c == NDOF ? CT_FORCE : CT_TORQUE;
        a.ctrl[CIDX(base + 0)] = w.x; a.ctrl[CIDX(base + 1)] = w.y; a.ctrl[CIDX(base + 2)] = w.z;
    }
}

int launch_env_pre(v2p_env* env, float* actions, hipStream_t s) {
    PhysArgs a = {};
    a.ctrl = env->ctrl;
    a.actions = actions;
    a.reset = env->buf.reset;
    a.pd_target = env->buf.pd_target;
    a.x_dof = env->buf.dof_state;
    a.x_rb = env->buf.rb_state;
    a.n = env->n;
    a.p = env->p;
    PairView pv{nullptr, nullptr, nullptr, nullptr, 0, 0};  // (the physics kernel looks its envs up itself: nothing to scatter here)
    const int64_t threads = env->n * NACT;
    hipLaunchKernelGGL(env_pre_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a, pv);
    return check_hip(hipGetLastError(), "env_pre_kernel");
}

// ---------------------------------------------------------------------------- the schedule of a batch
// The link-per-lane physics kernel is in the library TWICE (physics_ll.hip): the default object (168 VGPRs, three waves per
// SIMD, contact records and phase-dead values parked in LDS) behind launch_env_physics_ll, and the register build (256 VGPRs, two waves
// per SIMD, everything in registers) behind launch_env_physics_ll_regs.  Where a launch is as long as its heaviest env pair - up to
// ~5000 envs on one GPU - the register build is 7 - 12 % faster (no LDS round trips in the heaviest wave's chain; compiled for ILP), where
// the wave slots are full the LDS build is 15 % faster (profiles/r04e_dual_build.txt).

// envs resident per device (live v2p_env batches of this process): what kernel_build = 0 decides by, launch by launch
static std::atomic<int64_t> g_resident_envs[64];
static int64_t resident_envs(int device) { return (device >= 0 && device < 64) ? g_resident_envs[device].load(std::memory_order_relaxed) : 0; }
static constexpr int64_t REGS_BUILD_MAX_ENVS = 5120;  // measured crossover of the two builds (profiles/r04e_dual_build.txt)

void count_resident_envs(v2p_env* e, bool live) {
    if (live == (e->sched.counted_resident != 0) || e->device < 0 || e->device >= 64) return;
    g_resident_envs[e->device] += live ? e->n : -e->n;
    e->sched.counted_resident = live;
}

// the engine's defaults, applied to the fields of a batch that were left to the engine
EngineDefaults apply_engine_defaults(v2p_env* e) {
    const EngineDefaults d = engine_defaults(e->n, e->p.joint_limits != 0, e->sched.ll_regs_build != 0, e->ball != nullptr);
    if (e->sched.pair_mix_default) e->sched.pair_mix_permille = d.pair_mix_permille;
    if (e->sched.job_mono_default) e->sched.job.mono_permille = d.job_mono_permille;
    return d;
}

void fill_env_schedule(v2p_env* e, const v2p_sim_cfg* c) {
    LlSchedule& sc = e->sched;
    e->schedule = e->num_shapes > 1 ? 0 : c->schedule;  // the env-per-lane cross-check kernel is single-shape
    e->substeps_per_sim = c->substeps;
    sc.pair_period = c->pair_envs_by_load ? 1 : 0;
    sc.job.on = c->substep_jobs ? 1 : 0;
    sc.job_interleave = c->job_no_interleave ? 0 : 1;  // (A/B switch)
    // which build of the link-per-lane kernel this batch runs (see above): v2p_sim_cfg.kernel_build, 0 = by the number of
    // envs RESIDENT on the device - the batches of a process that share a GPU (rollout groups) are bound by instruction issue together,
    // whatever the size of each - re-evaluated launch by launch (choose_build); the value here is the one a lone batch would get
    sc.kernel_build = c->kernel_build;
    sc.ll_regs_build = c->kernel_build ? (c->kernel_build == 2) : (resident_envs(e->device) + e->n <= REGS_BUILD_MAX_ENVS);
    sc.pair_mix_default = c->pair_mix_permille < 0 ? 1 : 0;
    sc.pair_mix_permille = c->pair_mix_permille;
    sc.job_mono_default = c->job_mono_permille < 0 ? 1 : 0;
    sc.job.mono_permille = c->job_mono_permille;
    const EngineDefaults d = apply_engine_defaults(e);
    if (sc.job.on) {
        // (job_timeout_spins < 0: tests force the recovery path)
        sc.job_timeout_spins = c->job_timeout_spins == 0 ? d.job_timeout_spins : (c->job_timeout_spins < 0 ? 0l : (long)c->job_timeout_spins);
        sc.job.len = c->job_len > 0 ? c->job_len : d.job_len;
        sc.job.lead = c->job_lead == 0 ? d.job_lead : (c->job_lead < 0 ? 0 : c->job_lead);
    }
    // the two thresholds of job_plan that follow the device (JobCfg)
    hipDeviceProp_t prop;
    const bool have = hipGetDeviceProperties(&prop, e->device) == hipSuccess;
    sc.job.min_blocks = (c->substep_jobs == 1 && have) ? prop.multiProcessorCount * 8 : 0;
    sc.job.len2_blocks = have ? prop.multiProcessorCount * 32 : 8192;
}

// kernel_build = 0: the build follows the envs resident on the device (a second rollout group created after this batch moves both to the
// three-wave build); the heavy x light pairing share follows the build where it was left to the engine.  The choice is LATCHED: taken at
// the first launch after the batch was created or reset as a whole (an epoch boundary: every env restarts from a reference state) and
// kept until the next such reset - the two builds agree to rounding only, so a live batch must not change build in the middle of an
// epoch because an unrelated batch (an eval task next to training) came or went (advisor r5).
static int build_wanted(const v2p_env* e) { return resident_envs(e->device) <= REGS_BUILD_MAX_ENVS ? 1 : 0; }
void choose_build(v2p_env* e) {
    if (e->sched.kernel_build != 0 || e->sched.build_latched) return;
    e->sched.build_latched = 1;
    const int regs = build_wanted(e);
    if (regs == e->sched.ll_regs_build) return;
    e->sched.ll_regs_build = regs;
    apply_engine_defaults(e);
}
int next_kernel_build(const v2p_env* e) {
    if (e->sched.kernel_build == 0 && !e->sched.build_latched) return build_wanted(e) ? 2 : 1;  // (read-only: what choose_build would take now)
    return e->sched.ll_regs_build ? 2 : 1;
}

bool env_pairing_on(const v2p_env* env) { return env->sched.pair_period > 0 && env->schedule == 0 && env->p.enable_contact && env->n > 2; }

PairView env_pair_view(const v2p_env* env) {
    const LlSchedule& sc = env->sched;
    int mix = (int)(env->n * (int64_t)sc.pair_mix_permille / 1000);
    if (2 * mix > env->n) mix = (int)(env->n / 2);
    return PairView{sc.pair_key, sc.pair_pos, sc.pair_starts[sc.pair_buf], sc.perm, (int32_t)env->n, mix};
}

int launch_env_pairing(v2p_env* env, hipStream_t s) {
    // (v2p_env_debug_pairing only: the wave order the next launch will look up, as an explicit slot -> env table)
    hipLaunchKernelGGL(pair_scatter_kernel, dim3((unsigned)((env->n + 255) / 256)), dim3(256), 0, s, env_pair_view(env), env->n);
    return check_hip(hipGetLastError(), "pair_scatter_kernel");
}

// ---------------------------------------------------------------------------- a launch of physics_ll_kernel, either build
int ll_launch_prepare(v2p_env* env, hipStream_t s, float* actions, int* fused_post, unsigned blocks, bool diag, LlLaunch& L) {
    if (fused_post) *fused_post = 0;
    if (env->p.joint_limits && !env->p.enable_contact) {
        set_error("physics: joint limits run with contacts on");
        return V2P_ERR_UNSUPPORTED;
    }
    if (env->ball && !env->p.enable_contact) {
        set_error("physics: racket + ball runs with contacts on");
        return V2P_ERR_UNSUPPORTED;
    }
    LlSchedule& sc = env->sched;
    const bool paired = env_pairing_on(env);
    PhysArgs& a = L.a;
    a = {};
    const int buf = sc.pair_buf;
    a.pl_start = (paired && sc.pair_have) ? sc.pair_starts[buf] : nullptr;
    a.pl_list = sc.pair_list[buf];
    a.pl_list_next = sc.pair_list[1 - buf];
    a.pl_mix = env_pair_view(env).mix;
    a.pl_slot_env = sc.pair_slot_env;
    a.pair_key = sc.pair_key;
    a.pair_pos = sc.pair_pos;
    a.pair_hist = paired ? sc.pair_hist : nullptr;
    a.pair_start = sc.pair_starts[1 - buf];
    a.pair_done = sc.pair_done;
    a.model = env->model->dev;
    a.state = env->state;
    a.ctrl = env->ctrl;
    a.actions = actions;  // non-null: pre-physics runs in this kernel's prologue
    a.par_pack[0] = a.par_pack[1] = 0ull;
    for (int i = 0; i < NB; ++i) {
        const int par = env->model->host.parents[i] < 0 ? 0 : env->model->host.parents[i];
        a.par_pack[i / 12] |= (unsigned long long)par << (5 * (i % 12));
    }
    a.reset = env->buf.reset;
    a.pd_target = env->buf.pd_target;
    a.out = env->out;
    a.ws = env->ws;
    a.contact_ids = env->contact_ids;
    a.contact_ids_sub = env->contact_ids_sub;
    a.x_root = env->buf.root_states;
    a.x_dof = env->buf.dof_state;
    a.x_rb = env->buf.rb_state;
    a.x_contact = env->buf.contact_force;
    a.x_dof_force = env->buf.dof_force;
    a.prof = env->prof;
    a.prof_heavy = debug_env("V2P_PHASE_HEAVY") ? 1 : 0;  // diagnostics: sample the 8 heaviest waves instead of every 64th
    a.wave_times = env->wave_times;
    a.n = env->n;
    a.p = env->p;
    a.shapes = env->shapes_dev;
    a.env_shape = env->env_shape_dev;
    a.shape_aug = env->shape_aug_dev;
    if (env->ball) a.ball = *env->ball;
    a.job_blocks = (int)blocks;
    a.job_progress = sc.job_progress;
    a.job_hand = sc.job_hand;
    a.job_timeout_spins = sc.job_timeout_spins;
    a.job_interleave = sc.job_interleave;
    a.job_len = a.job_lead = 1;
    a.job_mono = (int)blocks;
    L.grid = blocks;
    L.diag = diag && env->p.enable_contact && env->p.solver_type != 1 && env->num_shapes <= 1 && !env->ball && !env->p.joint_limits && env->p.friction_frame == 0;
    if (L.diag) return V2P_OK;
    const JobPlan plan = job_plan(sc.job, blocks, env->p.nsub, env->ball != nullptr, sc.job_progress != nullptr);
    if (plan.cut) {
        a.job_epoch = ++sc.job_epoch;
        if (sc.job_epoch > (1 << 30) / (env->p.nsub + 1) - 2) sc.job_epoch = 0;  // (wraps before the progress words overflow; a wrap needs them cleared)
        if (sc.job_epoch == 0) {
            const int rc = check_hip(hipMemsetAsync(sc.job_progress, 0, sizeof(int) * (size_t)job_wave_slots(env->n), s), "hipMemsetAsync(job_progress)");  // (not the error word behind them)
            a.job_epoch = sc.job_epoch = 1;
            if (rc != V2P_OK) return rc;
        }
    }
    a.job_mono = plan.mono;
    a.job_len = plan.len;
    a.job_lead = plan.lead;
    L.grid = plan.grid;
    // every production instantiation is cut into substep jobs and runs post-physics in the epilogue of an env's last job (v2p_env_step)
    if (fused_post && actions && env->mlib) {
        a.post.b = env->buf;
        a.post.t = env->mlib->t;
        a.post.motion_id = env->motion_id;
        a.post.cur = env->cur_target;
        a.post.on = 1;
        *fused_post = 1;
    }
    return V2P_OK;
}

void ll_launch_done(v2p_env* env) {
    if (!env_pairing_on(env)) return;
    env->sched.pair_buf = 1 - env->sched.pair_buf;  // the tables this launch has filled are what the next one reads
    env->sched.pair_have = 1;
}

}  // namespace v2p
