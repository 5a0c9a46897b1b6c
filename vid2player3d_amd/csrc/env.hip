// The life of a batch (v2p_env), host code only: create and destroy, ball and racket attachment, the substep jobs' counters and the
// profiling events.  How a physics launch is scheduled is not decided here: ll_schedule.hpp, applied by physics_ll_host.hip.  Every
// allocation goes through the batch's DeviceOwner (e->own): nothing here frees by hand.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <new>
#include <vector>

#include "v2p_internal.hpp"
#include "phys_common.hpp"

using namespace v2p;

v2p_env::~v2p_env() { delete ball; }

// ---------------------------------------------------------------------------- create
// 1. check: pure host code.  Arguments first, then buffers, then sim parameters, then the enumerated config fields.
static int check_env_create(const v2p_model* const* shapes, int32_t num_shapes, const int32_t* env_shape_id, const v2p_mlib* mlib,
                            const v2p_sim_cfg* c, const int64_t* env_motion_id, int64_t n, const v2p_env_buffers* b, int device, v2p_env** out) {
    if (!shapes || num_shapes < 1 || !shapes[0]) { set_error("v2p_env_create: bad argument"); return V2P_ERR_INVALID; }
    const v2p_model* model = shapes[0];
    for (int32_t k = 1; k < num_shapes; ++k) {
        if (!shapes[k] || shapes[k]->device != device) { set_error("v2p_env_create_shapes: shape %d is null or lives on another device", k); return V2P_ERR_INVALID; }
        if (memcmp(shapes[k]->host.parents, model->host.parents, sizeof(model->host.parents))) {
            set_error("v2p_env_create_shapes: shape %d has a different body tree", k);
            return V2P_ERR_UNSUPPORTED;
        }
    }
    if (num_shapes > 1) {
        if (!env_shape_id) { set_error("v2p_env_create_shapes: env_shape_id is null"); return V2P_ERR_INVALID; }
        for (int64_t i = 0; i < n; ++i)
            if (env_shape_id[i] < 0 || env_shape_id[i] >= num_shapes) { set_error("v2p_env_create_shapes: env %lld has shape id %d", (long long)i, env_shape_id[i]); return V2P_ERR_INVALID; }
    }
    if (!mlib || !c || !env_motion_id || !b || !out || n <= 0) { set_error("v2p_env_create: bad argument"); return V2P_ERR_INVALID; }
    if (model->device != device || mlib->device != device) { set_error("v2p_env_create: model/motion-lib live on another device"); return V2P_ERR_INVALID; }
    const void* req[] = {b->root_states, b->dof_state, b->rb_state, b->contact_force, b->dof_force, b->pd_target, b->obs, b->rew,
                         b->sub_rewards, b->reset, b->terminate, b->progress, b->cur_time, b->reset_time, b->target[0], b->target[1]};
    for (const void* p : req)
        if (!p) { set_error("v2p_env_create: a required buffer is null"); return V2P_ERR_INVALID; }
    if (c->substeps < 1 || c->control_freq_inv < 1 || c->sim_dt <= 0.f || c->num_solver_iterations < 0 ||
        c->residual_hold_sims < 0 || c->residual_hold_sims > c->control_freq_inv) {
        set_error("v2p_env_create: bad sim parameters");
        return V2P_ERR_INVALID;
    }
    if (c->schedule != 0 && c->schedule != 1) { set_error("v2p_env_create: schedule must be 0 or 1"); return V2P_ERR_INVALID; }
    if (c->solver_type != 0 && c->solver_type != 1) { set_error("v2p_env_create: solver_type must be 0 (PGS) or 1 (TGS)"); return V2P_ERR_INVALID; }
    if (c->solver_type == 1 && c->schedule == 1) { set_error("v2p_env_create: the env-per-lane cross-check kernel solves PGS only"); return V2P_ERR_UNSUPPORTED; }
    if (c->kernel_build < 0 || c->kernel_build > 2) { set_error("v2p_env_create: kernel_build must be 0 (engine's choice), 1 (LDS-parked) or 2 (registers)"); return V2P_ERR_INVALID; }
    if (c->num_velocity_iterations != 0) {
        set_error("v2p_env_create: sim.physx.num_velocity_iterations = %d: the engine's contact solvers have no separate velocity pass (the reference's configs use 0)", c->num_velocity_iterations);
        return V2P_ERR_UNSUPPORTED;
    }
    if (!(c->bounce_threshold_velocity >= 0.f) || (c->enable_contact && !(c->rest_offset < c->contact_offset))) {
        set_error("v2p_env_create: bounce_threshold_velocity must be >= 0 and (with contacts on) rest_offset below contact_offset");
        return V2P_ERR_INVALID;
    }
    if (c->friction_frame != 0 && c->friction_frame != 1) { set_error("v2p_env_create: friction_frame must be 0 (world) or 1 (velocity)"); return V2P_ERR_INVALID; }
    if (c->friction_frame == 1 && c->schedule == 1) { set_error("v2p_env_create: the env-per-lane cross-check kernel solves in the world friction frame only"); return V2P_ERR_UNSUPPORTED; }
    if (c->joint_limits && (c->schedule == 1 || !c->enable_contact)) {
        set_error("v2p_env_create: joint_limits needs the link-per-lane schedule and contacts on");
        return V2P_ERR_UNSUPPORTED;
    }
    // (a share the engine picks is never out of range: only what the caller gave can be)
    if (c->pair_mix_permille > 500 || c->job_mono_permille > 1000) { set_error("v2p_env_create: pair_mix_permille <= 500, job_mono_permille <= 1000"); return V2P_ERR_INVALID; }
    return V2P_OK;
}

// joint-diagonal augmentation armature + h kd + h^2 kp per link of one body shape
static void joint_augmentation(const DevShape& sh, float h, float* aug) {
    aug[0] = 0.f;
    for (int b = 1; b < NB; ++b) aug[b] = sh.arm[b] + h * sh.kd[b] + h * h * sh.kp[b];
}

// 2. v2p_sim_cfg -> EnvParams
static void fill_env_params(const v2p_sim_cfg* c, const DevShape& shape, EnvParams& p) {
    p.h = c->sim_dt / (float)c->substeps;
    p.nsub = c->substeps * c->control_freq_inv;
    p.hold_sub = c->residual_hold_sims * c->substeps;
    p.n_iter = c->num_solver_iterations;
    p.enable_contact = c->enable_contact;
    p.gravity_z = c->gravity_z; p.mu = c->friction; p.contact_offset = c->contact_offset; p.max_depen = c->max_depenetration_velocity;
    p.erp = c->erp; p.ang_damp = c->angular_damping; p.max_ang_vel = c->max_angular_velocity;
    p.pd_tar_lim = c->pd_tar_lim; p.res_force_scale = c->residual_force_scale; p.res_torque_scale = c->residual_torque_scale;
    p.ground_tolerance = c->ground_tolerance; p.max_episode_length = c->max_episode_length;
    p.enable_early_termination = c->enable_early_termination;
    p.freeze_terminated = c->freeze_terminated_envs;
    p.solver_type = c->solver_type;
    p.joint_limits = c->joint_limits ? 1 : 0;
    p.limit_margin = c->limit_margin <= 0.f ? 0.05f : c->limit_margin;  // (a zero-initialised cfg gets the default)
    p.rest_offset = c->rest_offset;
    p.friction_frame = c->friction_frame;
    p.bounce_threshold = c->bounce_threshold_velocity;
    p.context_length = c->context_length; p.context_padding = c->context_padding;
    p.dt = (float)c->control_freq_inv * c->sim_dt;
    memcpy(p.term_heights, c->term_heights, sizeof(p.term_heights));
    memcpy(p.body_pos_weights, c->body_pos_weights, sizeof(p.body_pos_weights));
    memcpy(p.reward_specs, c->reward_specs, sizeof(p.reward_specs));
    joint_augmentation(shape, p.h, p.aug);
}

namespace v2p {
// out[N][525] + ws: only the env-per-lane cross-check schedule stages through global memory.  Both or neither.
int ensure_env_per_lane_buffers(v2p_env* e) {
    if (e->out && e->ws) return V2P_OK;
    const size_t N = (size_t)e->n;
    float *out = nullptr, *ws = nullptr;
    int rc = e->own.alloc(&out, OUT_SLOTS * N, "out", DeviceOwner::FILL_00);
    if (rc == V2P_OK) rc = e->own.alloc(&ws, (size_t)physics_ws_slots() * N, "ws", DeviceOwner::FILL_00);
    if (rc == V2P_OK) rc = check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize(env_per_lane buffers)");
    if (rc != V2P_OK) {
        e->own.release(ws);
        e->own.release(out);
        return rc;
    }
    e->out = out;
    e->ws = ws;
    return V2P_OK;
}
}  // namespace v2p

// 4. allocate: from here on a failure has one way out, the owner (delete e)
static int alloc_env(v2p_env* e, const v2p_model* const* shapes, const int32_t* env_shape_id, const v2p_sim_cfg* c) {
    const size_t N = (size_t)e->n, nsub = (size_t)e->p.nsub;
    DeviceOwner& own = e->own;
    const DeviceOwner::Fill Z = DeviceOwner::FILL_00, FF = DeviceOwner::FILL_FF, NONE = DeviceOwner::NO_FILL;
    int rc = own.alloc(&e->state, STATE_SLOTS * N, "state", Z);
    if (rc == V2P_OK) rc = own.alloc(&e->ctrl, CTRL_SLOTS * N, "ctrl", Z);
    if (rc == V2P_OK && c->debug_contacts >= 1) rc = own.alloc(&e->contact_ids, NB * 4 * N, "contact_ids", FF);
    if (rc == V2P_OK && e->schedule == 1) rc = ensure_env_per_lane_buffers(e);
    if (rc == V2P_OK && c->debug_contacts >= 2) rc = own.alloc(&e->contact_ids_sub, NB * 4 * N * nsub, "contact_ids_sub", FF);
    if (rc == V2P_OK && e->num_shapes > 1) {
        // per-env body shapes: the numeric tables of every shape + each shape's joint-diagonal augmentation, indexed by env_shape
        std::vector<float> aug((size_t)e->num_shapes * NB, 0.f);
        rc = own.alloc(&e->shapes_dev, (size_t)e->num_shapes, "shapes");
        for (int32_t k = 0; k < e->num_shapes && rc == V2P_OK; ++k) {
            const DevShape& sh = shapes[k]->host.shape;
            rc = check_hip(hipMemcpy(e->shapes_dev + k, &sh, sizeof(DevShape), hipMemcpyHostToDevice), "hipMemcpy(shape)");
            joint_augmentation(sh, e->p.h, &aug[(size_t)k * NB]);
        }
        if (rc == V2P_OK) rc = own.alloc(&e->shape_aug_dev, aug.size(), "shape_aug", NONE, aug.data());
        if (rc == V2P_OK) rc = own.alloc(&e->env_shape_dev, N, "env_shape", NONE, env_shape_id);
    }
    if (rc == V2P_OK && e->sched.job.on) {
        rc = own.alloc(&e->sched.job_progress, (size_t)job_wave_slots(e->n) + 2, "job_progress", Z);
        // the state as the jobs hand it over: 50 16-byte chunks per env (see physics_ll.hip)
        if (rc == V2P_OK) rc = own.alloc(&e->sched.job_hand, HAND_FLOATS * N * (nsub > 1 ? nsub - 1 : 1), "job_hand");
    }
    std::vector<int32_t> iota(N);
    for (size_t i = 0; i < N; ++i) iota[i] = (int32_t)i;
    if (rc == V2P_OK) rc = own.alloc(&e->sched.pair_key, N, "pair_key", Z);
    if (rc == V2P_OK) rc = own.alloc(&e->sched.pair_pos, N, "pair_pos", NONE, iota.data());
    if (rc == V2P_OK) rc = own.alloc(&e->sched.perm, N, "perm", NONE, iota.data());
    if (rc == V2P_OK) rc = own.alloc(&e->sched.pair_hist, (size_t)(4 * PAIR_BINS + 1), "pair_hist", Z);
    for (int k = 0; k < 2 && rc == V2P_OK; ++k) rc = own.alloc(&e->sched.pair_list[k], PAIR_BINS * N, "pair_list");
    if (rc == V2P_OK) rc = own.alloc(&e->sched.pair_slot_env, N, "pair_slot_env");
    if (rc == V2P_OK) {
        e->sched.pair_starts[0] = e->sched.pair_hist + PAIR_BINS;
        e->sched.pair_starts[1] = e->sched.pair_hist + 2 * PAIR_BINS;
        e->sched.pair_done = e->sched.pair_hist + 4 * PAIR_BINS;
        rc = check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize(env_create)");
    }
    // (one record per wave; per JOB in a V2P_LL_TIMELINE build: up to nsub per wave)
    if (rc == V2P_OK && debug_env("V2P_WAVE_TIMES")) rc = own.alloc(&e->wave_times, 4 * (N / 2 + 1) * nsub, "wave_times", Z);
    if (rc == V2P_OK && debug_env("V2P_PHASE_TIMING")) rc = own.alloc(&e->prof, (size_t)PROF_COUNT, "prof", Z);
    return rc;
}

static int env_create_impl(const v2p_model* const* shapes, int32_t num_shapes, const int32_t* env_shape_id, const v2p_mlib* mlib,
                           const v2p_sim_cfg* c, const int64_t* env_motion_id, int64_t n, const v2p_env_buffers* b, int device, v2p_env** out) {
    int rc = check_env_create(shapes, num_shapes, env_shape_id, mlib, c, env_motion_id, n, b, device, out);
    if (rc != V2P_OK) return rc;
    std::unique_ptr<v2p_env> e(new (std::nothrow) v2p_env());
    if (!e) { set_error("v2p_env_create: out of host memory"); return V2P_ERR_NOMEM; }
    e->model = shapes[0];
    e->num_shapes = num_shapes;
    e->mlib = mlib;
    e->buf = *b;
    e->n = n;
    e->ctx.ctx_dim = V2P_CONTEXT_DIM;  // no context transform: 378-float frames
    e->device = e->own.device = device;
    e->motion_id = env_motion_id;
    fill_env_params(c, shapes[0]->host.shape, e->p);
    DeviceGuard g(device);
    if (!g.ok) { set_error("v2p_env_create: cannot select device %d", device); return V2P_ERR_HIP; }
    fill_env_schedule(e.get(), c);  // 3. the schedule of the batch (physics_ll_host.hip)
    rc = alloc_env(e.get(), shapes, env_shape_id, c);
    if (rc != V2P_OK) return rc;
    count_resident_envs(e.get(), true);
    *out = e.release();
    return V2P_OK;
}

namespace v2p {
// the physics launch of either schedule, bracketed by events while a measurement is open
int env_physics_launch(v2p_env* e, hipStream_t s, float* actions, int* fused_post) {
    // (sampled: launch L of the measurement is bracketed when L % stride == (L / period) % stride - every position of a period-long
    // epoch is met once in `stride` epochs)
    bool rec = e->prof_ev && e->prof_n < e->prof_cap;
    if (e->prof_ev) {
        const int64_t L = e->prof_seen++;
        if (e->prof_stride > 1) rec = rec && (L % e->prof_stride) == (L / e->prof_period) % e->prof_stride;
    }
    choose_build(e);
    if (rec) (void)hipEventRecord(e->prof_ev[2 * e->prof_n], s);
    int rc = e->schedule != 0 ? launch_env_physics(e, s)
                              : (e->sched.ll_regs_build ? launch_env_physics_ll_regs(e, s, actions, fused_post) : launch_env_physics_ll(e, s, actions, fused_post));
    if (rec) { (void)hipEventRecord(e->prof_ev[2 * e->prof_n + 1], s); ++e->prof_n; }
    return rc;
}
}  // namespace v2p

static void profile_close(v2p_env* e) {
    e->own.release(e->prof_ev);
    e->prof_ev = nullptr;
    e->prof_cap = e->prof_n = 0;
}

extern "C" {

int v2p_env_create(const v2p_model* model, const v2p_mlib* mlib, const v2p_sim_cfg* c, const int64_t* env_motion_id, int64_t n,
                   const v2p_env_buffers* b, int device, v2p_env** out) {
    return env_create_impl(&model, 1, nullptr, mlib, c, env_motion_id, n, b, device, out);
}

int v2p_env_create_shapes(const v2p_model* const* shapes, int32_t num_shapes, const int32_t* env_shape_id, const v2p_mlib* mlib,
                          const v2p_sim_cfg* c, const int64_t* env_motion_id, int64_t n, const v2p_env_buffers* b, int device, v2p_env** out) {
    return env_create_impl(shapes, num_shapes, env_shape_id, mlib, c, env_motion_id, n, b, device, out);
}

void v2p_env_destroy(v2p_env* e) {
    if (!e) return;
    count_resident_envs(e, false);
    DeviceGuard g(e->device);
    if (e->wave_times) {
        const size_t nw = ((size_t)e->n / 2 + 1) * (size_t)e->p.nsub;  // (records that were never written stay zero and are skipped)
        std::vector<long long> h(nw * 4);
        FILE* f = fopen(debug_env("V2P_WAVE_TIMES") ? debug_env("V2P_WAVE_TIMES") : "wave_times.bin", "wb");
        if (f && hipMemcpy(h.data(), e->wave_times, sizeof(long long) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) fwrite(h.data(), sizeof(long long), h.size(), f);
        if (f) fclose(f);
    }
    if (e->prof) {
        long long h[PROF_COUNT];
        if (hipMemcpy(h, e->prof, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr,
                    "[v2p phase cycles, workgroup 0] link-per-lane: counter k = phase k-1 of {pass1, pass2, root+pass3, contacts, lambda, sweep, "
                    "integrate}; env-per-lane: {stage, pass1, pass2, root+pass3, contacts, lambda, sweep, integrate}: "
                    "%lld %lld %lld %lld %lld %lld %lld %lld | block updates %lld touched-sum %lld substeps %lld | "
                    "sweep: rows %lld up %lld contact-rounds %lld down %lld manifold-reductions %lld | contacts: cull %lld rounds %lld points %lld | null updates %lld | "
                    "sweep, the rest: close-up %lld close-pass %lld visit-head-tail %lld set-up %lld "
                    "(where these four are counted - the default build - `up` is without the closing move, `down` without the closing pass and `rows` "
                    "without the tail of a visit: not comparable with logs that lack them)\n",
                    h[PROF_HEAD], h[PROF_PASS1], h[PROF_PASS2], h[PROF_PASS3], h[PROF_CONTACTS], h[PROF_LAMBDA], h[PROF_SWEEP], h[PROF_INTEGRATE],
                    h[PROF_UPDATES], h[PROF_TOUCHED], h[PROF_SUBSTEPS], h[PROF_ROWS], h[PROF_UP], h[PROF_ROUNDS], h[PROF_DOWN], h[PROF_MANIFOLDS],
                    h[PROF_CULL], h[PROF_SCAN], h[PROF_POINTS], h[PROF_NULL_UPDATES], h[PROF_CLOSE_MOVE], h[PROF_CLOSE_PASS], h[PROF_VISIT_ENDS], h[PROF_SWEEP_SETUP]);
    }
    delete e;
}

int v2p_env_attach_ball(v2p_env* e, const v2p_ball_cfg* c, const v2p_ball_buffers* b) {
    if (!e || !c || !b) { set_error("v2p_env_attach_ball: null argument"); return V2P_ERR_INVALID; }
    if (!b->ball_state || !b->racket_state || !b->ball_per_sim || !b->racket_hit_per_sim || !b->ball_contact) { set_error("v2p_env_attach_ball: a buffer is null"); return V2P_ERR_INVALID; }
    if (c->racket_link < 1 || c->racket_link >= NB || c->num_cylinders < 0 || c->num_cylinders > 2 || !(c->radius > 0.f) || !(c->mass > 0.f) || !(c->inertia > 0.f)) {
        set_error("v2p_env_attach_ball: bad ball parameters");
        return V2P_ERR_INVALID;
    }
    {
        const int nflags = (b->has_bounce != nullptr) + (b->has_bounce_now != nullptr) + (b->bounce_pos != nullptr) + (b->has_racket_contact != nullptr) + (b->has_racket_contact_now != nullptr);
        if (nflags != 0 && nflags != 5) { set_error("v2p_env_attach_ball: give all five flag buffers or none"); return V2P_ERR_INVALID; }
    }
    if (e->schedule != 0 || !e->p.enable_contact) {
        set_error("v2p_env_attach_ball: racket + ball needs the link-per-lane schedule and contacts on");
        return V2P_ERR_UNSUPPORTED;
    }
    if (e->p.rest_offset != 0.f) {
        set_error("v2p_env_attach_ball: sim.physx.rest_offset != 0 is modelled for the hull x plane rows only, not for the ball's rows");
        return V2P_ERR_UNSUPPORTED;
    }
    // built aside and committed at the end: a failure leaves the batch as it was (with its earlier ball, or with none)
    std::unique_ptr<BallDev> fresh(e->ball ? nullptr : new (std::nothrow) BallDev());
    if (!e->ball && !fresh) { set_error("v2p_env_attach_ball: out of host memory"); return V2P_ERR_NOMEM; }
    BallDev d = e->ball ? *e->ball : *fresh;
    d.radius = c->radius; d.mass = c->mass; d.inv_mass = 1.f / c->mass; d.inv_inertia = 1.f / c->inertia;
    d.rest_ground = c->restitution_ground; d.fric_ground = c->friction_ground; d.rest_racket = c->restitution_racket; d.fric_racket = c->friction_racket;
    d.bounce_thr = c->bounce_threshold_velocity; d.ang_damp = c->angular_damping; d.max_ang_vel = c->max_angular_velocity; d.spin_scale = c->spin_scale;
    d.racket.racket_link = c->racket_link; d.racket.ncyl = c->num_cylinders;
    memcpy(d.racket.cyl, c->cylinders, sizeof(d.racket.cyl));
    memcpy(d.racket.racket_off, c->racket_offset, sizeof(d.racket.racket_off));
    d.sub_per_sim = e->substeps_per_sim;
    d.state = b->ball_state; d.racket_state = b->racket_state; d.per_sim = b->ball_per_sim; d.hit_per_sim = b->racket_hit_per_sim; d.contact = b->ball_contact;
    d.rest_body = c->restitution_body; d.fric_body = c->friction_body; d.body_contacts = c->body_contacts ? 1 : 0;
    d.bounce_height = c->bounce_height; d.poll_hits = c->poll_racket_hits ? 1 : 0;
    d.body_contact = b->ball_body_contact;
    d.has_bounce = b->has_bounce; d.has_bounce_now = b->has_bounce_now; d.bounce_pos = b->bounce_pos;
    d.has_hit = b->has_racket_contact; d.has_hit_now = b->has_racket_contact_now;
    d.contact_sum = b->contact_force_sum;
    // every shape carries the cfg's racket until v2p_env_set_racket_shapes says otherwise
    const std::vector<RacketDev> all((size_t)e->num_shapes, d.racket);
    float* new_part = nullptr;
    int rc = V2P_OK;
    if (d.contact_sum && !d.contact_part) {
        const size_t nsim = (size_t)(e->p.nsub / e->substeps_per_sim);
        rc = e->own.alloc(&new_part, (size_t)e->n * nsim * NB * 3, "contact_part");
        if (rc == V2P_OK) d.contact_part = new_part;
    }
    if (rc == V2P_OK && !d.rackets) rc = e->own.alloc(&d.rackets, all.size(), "rackets", DeviceOwner::NO_FILL, all.data());
    else if (rc == V2P_OK) rc = check_hip(hipMemcpy((void*)d.rackets, all.data(), sizeof(RacketDev) * all.size(), hipMemcpyHostToDevice), "hipMemcpy(rackets)");
    if (rc != V2P_OK) {
        e->own.release(new_part);
        return rc;
    }
    if (!e->ball) e->ball = fresh.release();
    *e->ball = d;
    apply_engine_defaults(e);
    return V2P_OK;
}

int v2p_env_set_racket_shapes(v2p_env* e, const v2p_racket_geom* per_shape, int32_t num_shapes) {
    if (!e || !per_shape) { set_error("v2p_env_set_racket_shapes: null argument"); return V2P_ERR_INVALID; }
    if (num_shapes != e->num_shapes) {
        set_error("v2p_env_set_racket_shapes: %d rackets for a batch of %d body shapes", num_shapes, e->num_shapes);
        return V2P_ERR_INVALID;
    }
    std::vector<RacketDev> all((size_t)num_shapes);
    for (int32_t k = 0; k < num_shapes; ++k) {
        const v2p_racket_geom& g = per_shape[k];
        if (g.racket_link < 1 || g.racket_link >= NB || g.num_cylinders < 0 || g.num_cylinders > 2) {
            set_error("v2p_env_set_racket_shapes: shape %d: racket_link %d (must be 1 .. %d) / num_cylinders %d (must be 0 .. 2)", k, g.racket_link, NB - 1, g.num_cylinders);
            return V2P_ERR_INVALID;
        }
        all[k].racket_link = g.racket_link; all[k].ncyl = g.num_cylinders;
        memcpy(all[k].cyl, g.cylinders, sizeof(all[k].cyl));
        memcpy(all[k].racket_off, g.racket_offset, sizeof(all[k].racket_off));
    }
    if (!e->ball || !e->ball->rackets) { set_error("v2p_env_set_racket_shapes: no ball attached (call v2p_env_attach_ball first)"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    return check_hip(hipMemcpy((void*)e->ball->rackets, all.data(), sizeof(RacketDev) * all.size(), hipMemcpyHostToDevice), "hipMemcpy(rackets)");
}

int v2p_env_check(v2p_env* e, void* stream) {
    if (!e) { set_error("v2p_env_check: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    int rc = V2P_OK;
    if (!e->own.guarded) rc = check_hip(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    else {  // (v2p_debug_guards was on when the batch was created; check_guards synchronises the stream itself)
        std::vector<DeviceOwner::GuardDamage> d;
        rc = e->own.check_guards((hipStream_t)stream, &d);
        if (rc == V2P_OK && !d.empty()) {
            set_error("v2p_env_check: %zu byte(s) written outside '%s' (%s %zu byte(s) %s), %zu damaged guard zone(s) in all", d[0].count, d[0].name,
                      d[0].behind ? "first" : "nearest", d[0].first, d[0].behind ? "behind its end" : "before its start", d.size());
            return V2P_ERR_INTERNAL;
        }
    }
    if (rc != V2P_OK || !e->sched.job_progress) return rc;
    int32_t count[2] = {0, 0};
    rc = check_hip(hipMemcpy(count, e->sched.job_progress + v2p::job_wave_slots(e->n), sizeof(count), hipMemcpyDeviceToHost), "hipMemcpy(job recovery counters)");
    if (rc == V2P_OK) { e->job_recoveries = count[0]; e->jobs_skipped = count[1]; }
    if (rc == V2P_OK && e->jobs_skipped > e->jobs_skipped_reported) {
        // a late job of a cut pair found its step complete and did not run: its substeps were replayed by its successors (results are the
        // same bits), but what only IT publishes - exposed PD targets, the in-place masking of dead envs' actions, the ball's per-call
        // records - is missing for that step
        set_error("v2p_env_check: %lld substep job(s) started after their env pair's step was complete and were skipped: the per-call records they own were not "
                  "published for those steps (dispatch far out of order; v2p_sim_cfg.substep_jobs = 0 avoids it)", (long long)(e->jobs_skipped - e->jobs_skipped_reported));
        e->jobs_skipped_reported = e->jobs_skipped;
        return V2P_ERR_INTERNAL;
    }
    return rc;
}

int v2p_env_check_async(v2p_env* e, void* stream) {
    if (!e) { set_error("v2p_env_check_async: bad argument"); return V2P_ERR_INVALID; }
    if (!e->sched.job_progress) return V2P_OK;
    DeviceGuard g(e->device);
    int rc = V2P_OK;
    if (!e->err_host) {
        int32_t* host = nullptr;
        rc = e->own.alloc_pinned(&host, 2, "job recovery counter");
        if (rc == V2P_OK) rc = e->own.events(&e->err_event, 1, hipEventDisableTiming, "job recovery counter");
        if (rc != V2P_OK) { e->own.release(host); return rc; }  // (no half-built pair: a later call starts over)
        e->err_host = host;
    } else if (e->err_pending && hipEventQuery(e->err_event[0]) == hipSuccess) {
        e->err_pending = 0;
        e->job_recoveries = e->err_host[0];
        e->jobs_skipped = e->err_host[1];
    }
    if (!e->err_pending) {  // fetch the counter as it stands behind everything enqueued so far; looked at by the next call
        rc = check_hip(hipMemcpyAsync(e->err_host, e->sched.job_progress + v2p::job_wave_slots(e->n), 2 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream),
                       "hipMemcpyAsync(job recovery counter)");
        if (rc == V2P_OK) rc = check_hip(hipEventRecord(e->err_event[0], (hipStream_t)stream), "hipEventRecord(job recovery counter)");
        if (rc == V2P_OK) e->err_pending = 1;
    }
    return rc;
}

int v2p_env_job_recoveries(v2p_env* e, int64_t* count) {
    if (!e || !count) { set_error("v2p_env_job_recoveries: bad argument"); return V2P_ERR_INVALID; }
    *count = e->job_recoveries;
    return V2P_OK;
}

int v2p_env_jobs_skipped(v2p_env* e, int64_t* count) {
    if (!e || !count) { set_error("v2p_env_jobs_skipped: bad argument"); return V2P_ERR_INVALID; }
    *count = e->jobs_skipped;
    return V2P_OK;
}

int v2p_env_profile_begin(v2p_env* e, int64_t max_launches) { return v2p_env_profile_begin_sampled(e, max_launches, 1, 1); }

int v2p_env_profile_begin_sampled(v2p_env* e, int64_t max_launches, int32_t stride, int32_t period) {
    if (!e || max_launches <= 0 || max_launches > (1 << 20) || stride < 1 || period < 1) { set_error("v2p_env_profile_begin: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    profile_close(e);
    e->prof_stride = stride;
    e->prof_period = period;
    e->prof_seen = 0;
    const int rc = e->own.events(&e->prof_ev, 2 * (size_t)max_launches, hipEventDefault, nullptr);
    if (rc == V2P_ERR_NOMEM) set_error("v2p_env_profile_begin: out of host memory");
    if (rc == V2P_OK) e->prof_cap = max_launches;
    return rc;
}

int v2p_env_profile_end(v2p_env* e, double* physics_ms_total, int64_t* launches) {
    if (!e || !physics_ms_total || !launches) { set_error("v2p_env_profile_end: bad argument"); return V2P_ERR_INVALID; }
    if (!e->prof_ev) { set_error("v2p_env_profile_end: no measurement is open"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    double total = 0.0;
    int rc = V2P_OK;
    for (int64_t k = 0; k < e->prof_n && rc == V2P_OK; ++k) {
        float ms = 0.f;
        rc = check_hip(hipEventSynchronize(e->prof_ev[2 * k + 1]), "hipEventSynchronize");
        if (rc == V2P_OK) rc = check_hip(hipEventElapsedTime(&ms, e->prof_ev[2 * k], e->prof_ev[2 * k + 1]), "hipEventElapsedTime");
        total += ms;
    }
    *physics_ms_total = total;
    *launches = e->prof_n;
    profile_close(e);
    return rc;
}

int v2p_env_guard_counts(const v2p_env* e, int64_t* guarded, int64_t* poisoned) {
    if (!e || !guarded || !poisoned) { set_error("v2p_env_guard_counts: bad argument"); return V2P_ERR_INVALID; }
    *guarded = e->own.guarded;
    *poisoned = e->own.poisoned;
    return V2P_OK;
}

int v2p_env_kernel_build(const v2p_env* e) {  // (the build the NEXT launch of the batch runs)
    if (!e) return V2P_ERR_INVALID;
    return next_kernel_build(e);
}

}  // extern "C"
