// C-ABI entry points of libv2p_rollout.so (declared in include/v2p_rollout.h).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "controller_actions.hpp"
#include "ctl_ppo.hpp"
#include "flag_reset.hpp"
#include "match_record.hpp"
#include "mvae_player.hpp"
#include "mvae_target.hpp"
#include "pair_reset.hpp"
#include "policy_io.hpp"
#include "tennis_eval.hpp"
#include "two_hand_fix.hpp"
#include "tennis_reset.hpp"
#include "tennis_task.hpp"
#include "v2p_internal.hpp"

namespace v2p {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return V2P_OK;
    set_error("%s: %s", what, hipGetErrorString(e));
    return V2P_ERR_HIP;
}

DeviceGuard::DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
}
DeviceGuard::~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
}

// Profiling switches (V2P_WAVE_TIMES, V2P_PHASE_TIMING, V2P_PHASE_HEAVY, V2P_ENVS_PER_BLOCK) are read from the environment ONLY in a
// process that sets V2P_DEBUG=1 (tools/*.sh do); every engine option is a field of v2p_sim_cfg.
const char* debug_env(const char* name) {
    const char* d = getenv("V2P_DEBUG");
    return (d && d[0] == '1' && d[1] == 0) ? getenv(name) : nullptr;
}

}  // namespace v2p

using namespace v2p;

extern "C" {

const char* v2p_last_error(void) { return g_err; }
int v2p_abi_version(void) { return V2P_ABI_VERSION; }

int v2p_model_create(const v2p_model_desc* d, int device, v2p_model** out) {
    if (!d || !out) { set_error("v2p_model_create: null argument"); return V2P_ERR_INVALID; }
    DevModel host;
    int rc = compile_model(*d, &host);
    if (rc != V2P_OK) return rc;
    v2p_model* m = new (std::nothrow) v2p_model();
    if (!m) { set_error("v2p_model_create: out of host memory"); return V2P_ERR_NOMEM; }
    m->host = host;
    m->device = m->own.device = device;
    DeviceGuard g(device);
    if (!g.ok) { set_error("v2p_model_create: cannot select device %d", device); rc = V2P_ERR_HIP; }
    if (rc == V2P_OK) rc = m->own.alloc(&m->dev, 1, "model", DeviceOwner::NO_FILL, &m->host);
    if (rc != V2P_OK) { delete m; return rc; }
    *out = m;
    return V2P_OK;
}

void v2p_model_destroy(v2p_model* m) { delete m; }

int v2p_mlib_create(const v2p_motion_tables* t, int device, v2p_mlib** out) {
    if (!t || !out) { set_error("v2p_mlib_create: null argument"); return V2P_ERR_INVALID; }
    if (t->num_motions <= 0 || t->num_frames_total <= 0) { set_error("v2p_mlib_create: empty motion library"); return V2P_ERR_INVALID; }
    const void* ptrs[] = {t->gts, t->grs, t->lrs, t->grvs, t->gravs, t->dvs, t->motion_lengths, t->motion_num_frames, t->motion_dt,
                          t->motion_min_verts_h, t->length_starts, t->motion_bodies};
    for (const void* p : ptrs)
        if (!p) { set_error("v2p_mlib_create: null table pointer"); return V2P_ERR_INVALID; }
    if (((uintptr_t)t->grs | (uintptr_t)t->lrs) & 15) { set_error("v2p_mlib_create: grs/lrs must be 16-byte aligned"); return V2P_ERR_INVALID; }
    for (int k = 0; k < 4; ++k)
        if (t->key_body_ids[k] < 0 || t->key_body_ids[k] >= NB) { set_error("v2p_mlib_create: key body id out of range"); return V2P_ERR_INVALID; }
    v2p_mlib* m = new (std::nothrow) v2p_mlib();
    if (!m) { set_error("v2p_mlib_create: out of host memory"); return V2P_ERR_NOMEM; }
    m->t = *t;
    m->device = device;
    *out = m;
    return V2P_OK;
}

void v2p_mlib_destroy(v2p_mlib* m) { delete m; }

int v2p_motion_state(const v2p_mlib* m, const int64_t* ids, const float* times, int64_t q, int adjust_height, float ground_tol,
                     float* const out[9], void* stream) {
    if (!m || !out || q < 0 || (q > 0 && (!ids || !times))) { set_error("v2p_motion_state: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(m->device);
    return launch_motion_state(m->t, ids, times, q, adjust_height, ground_tol, out, (hipStream_t)stream);
}

int v2p_reward(int64_t n, const float* body_pos, const float* body_rot, const float* tgt_pos, const float* tgt_rot, const float* dof_pos,
               const float* dof_vel, const float* tgt_dof_pos, const float* tgt_dof_vel, const float* w, const float specs[8], float* reward,
               float* sub, void* stream) {
    if (n < 0 || !w || !specs) { set_error("v2p_reward: bad argument"); return V2P_ERR_INVALID; }
    return launch_reward(n, body_pos, body_rot, tgt_pos, tgt_rot, dof_pos, dof_vel, tgt_dof_pos, tgt_dof_vel, w, specs, reward, sub,
                         (hipStream_t)stream);
}

int v2p_reset_flags(int64_t n, const int64_t* progress, const float* rb_pos, const float* heights, const float* cur_time,
                    const float* clip_len, float max_len, int early, int64_t* reset_out, int64_t* term_out, void* stream) {
    if (n < 0 || !heights) { set_error("v2p_reset_flags: bad argument"); return V2P_ERR_INVALID; }
    return launch_reset_flags(n, progress, rb_pos, heights, cur_time, clip_len, max_len, early, reset_out, term_out, (hipStream_t)stream);
}

int v2p_obs_imitation(int64_t n, const float* body_pos, const float* body_rot, const float* tgt_pos, const float* tgt_rot,
                      const float* dof_pos, const float* dof_vel, const float* tgt_dof_pos, const float* body_vel,
                      const float* body_ang_vel, const float* motion_bodies, const float* norm_mean, const float* norm_std, float norm_clip,
                      float* obs, void* stream) {
    if (n < 0 || ((norm_mean == nullptr) != (norm_std == nullptr))) { set_error("v2p_obs_imitation: bad argument"); return V2P_ERR_INVALID; }
    return launch_obs_imitation(n, body_pos, body_rot, tgt_pos, tgt_rot, dof_pos, dof_vel, tgt_dof_pos, body_vel, body_ang_vel,
                                motion_bodies, norm_mean, norm_std, norm_clip, obs, (hipStream_t)stream);
}

int v2p_obs_imitation_packed_w(int64_t rows, int64_t steps, const float* obs, const float* context_feat, int64_t ctx_frames, int64_t ctx_dim,
                               int64_t first_frame, const float* norm_mean, const float* norm_std, float norm_clip, float* out, void* stream) {
    if (rows < 0 || steps < 1 || rows % steps || !obs || !context_feat || !out || first_frame < 0 || first_frame + steps > ctx_frames ||
        ctx_dim < V2P_CONTEXT_DIM || ((norm_mean == nullptr) != (norm_std == nullptr))) {
        set_error("v2p_obs_imitation_packed: bad argument");
        return V2P_ERR_INVALID;
    }
    return launch_obs_imitation_packed(rows, steps, obs, context_feat, ctx_frames, ctx_dim, first_frame, norm_mean, norm_std, norm_clip, out,
                                       (hipStream_t)stream);
}

int v2p_obs_imitation_packed(int64_t rows, int64_t steps, const float* obs, const float* context_feat, int64_t ctx_frames, int64_t first_frame,
                             const float* norm_mean, const float* norm_std, float norm_clip, float* out, void* stream) {
    return v2p_obs_imitation_packed_w(rows, steps, obs, context_feat, ctx_frames, V2P_CONTEXT_DIM, first_frame, norm_mean, norm_std, norm_clip, out,
                                      stream);
}

int v2p_policy_head_w(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t ctx_dim, int64_t frame, const float* logstd,
                      const float* noise, float* action, float* sigma, float* neglogp, void* stream) {
    if (n < 0 || !mu || !context_feat || !logstd || !noise || !action || !neglogp || frame < 0 || frame >= ctx_frames || ctx_dim < V2P_CONTEXT_DIM) {
        set_error("v2p_policy_head: bad argument");
        return V2P_ERR_INVALID;
    }
    return launch_policy_head(n, mu, context_feat, ctx_frames, ctx_dim, frame, logstd, noise, action, sigma, neglogp, (hipStream_t)stream);
}

int v2p_policy_head(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t frame, const float* logstd, const float* noise,
                    float* action, float* sigma, float* neglogp, void* stream) {
    return v2p_policy_head_w(n, mu, context_feat, ctx_frames, V2P_CONTEXT_DIM, frame, logstd, noise, action, sigma, neglogp, stream);
}

int v2p_policy_head_record_w(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t ctx_dim, int64_t frame,
                             const float* logstd, const float* noise, float* action, float* sigma_row, float* neglogp_row, float* action_row,
                             float* mu_row, void* stream) {
    if (n < 0 || !mu || !context_feat || !logstd || !noise || !action || !neglogp_row || frame < 0 || frame >= ctx_frames ||
        ctx_dim < V2P_CONTEXT_DIM) {
        set_error("v2p_policy_head_record: bad argument");
        return V2P_ERR_INVALID;
    }
    return launch_policy_head(n, mu, context_feat, ctx_frames, ctx_dim, frame, logstd, noise, action, sigma_row, neglogp_row, (hipStream_t)stream,
                              action_row, mu_row);
}

int v2p_policy_head_record(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t frame, const float* logstd, const float* noise,
                           float* action, float* sigma_row, float* neglogp_row, float* action_row, float* mu_row, void* stream) {
    return v2p_policy_head_record_w(n, mu, context_feat, ctx_frames, V2P_CONTEXT_DIM, frame, logstd, noise, action, sigma_row, neglogp_row,
                                    action_row, mu_row, stream);
}

int v2p_gae(int64_t horizon, int64_t n, const float* fdones, const float* values, const float* rewards, const float* next_values, float gamma,
            float tau, float* advs, void* stream) {
    if (horizon < 0 || n < 0) { set_error("v2p_gae: bad argument"); return V2P_ERR_INVALID; }
    return launch_gae(horizon, n, fdones, values, rewards, next_values, gamma, tau, advs, (hipStream_t)stream);
}

int v2p_value_record(int64_t n, const float* value_raw, const double* running_mean, const double* running_var, float epsilon, const float* terminated,
                     float* values_row, float* next_values_row, void* stream) {
    if (n < 0 || (n > 0 && (!value_raw || ((running_mean == nullptr) != (running_var == nullptr)) || (next_values_row && !terminated)))) {
        set_error("v2p_value_record: bad argument");
        return V2P_ERR_INVALID;
    }
    return launch_value_record(n, value_raw, running_mean, running_var, epsilon, terminated, values_row, next_values_row, (hipStream_t)stream);
}

int v2p_rollout_record(int64_t n, const float* obs, int64_t obs_dim, const float* rew, const int64_t* reset, const int64_t* terminate, const float* sub_rewards,
                       float* next_obs_row, float* rewards_row, float* dones_row, float* dones, float* terminated, float* prev_dones, float* cur_rewards,
                       float* cur_lengths, double* acc, double* sub_acc, void* stream) {
    if (n < 0 || obs_dim < 0 || (n > 0 && (!rew || !reset || !terminate || !sub_rewards || !rewards_row || !dones_row || !dones || !terminated || !prev_dones ||
                                           !cur_rewards || !cur_lengths || !acc || !sub_acc || (next_obs_row && !obs)))) {
        set_error("v2p_rollout_record: bad argument");
        return V2P_ERR_INVALID;
    }
    return launch_rollout_record(n, obs, obs_dim, rew, reset, terminate, sub_rewards, next_obs_row, rewards_row, dones_row, dones, terminated, prev_dones, cur_rewards,
                                 cur_lengths, acc, sub_acc, (hipStream_t)stream);
}

int v2p_motion_tables_build(int64_t num_frames_total, int64_t num_clips, const double* local_rot, const double* root_trans, const int32_t* frame_clip,
                            const int64_t* clip_start, const int32_t* clip_frames, const double* clip_dt, const int32_t* parents, const double* local_pos,
                            int32_t per_clip_skeleton, float* gts, float* grs, float* lrs, float* grvs, float* gravs, float* dvs, void* stream) {
    if (num_frames_total < 0 || num_clips < 0 || !parents) { set_error("v2p_motion_tables_build: bad argument"); return V2P_ERR_INVALID; }
    if (num_frames_total > 0 && (!local_rot || !root_trans || !frame_clip || !clip_start || !clip_frames || !clip_dt || !local_pos || !gts || !grs || !lrs || !grvs || !gravs || !dvs)) {
        set_error("v2p_motion_tables_build: null buffer");
        return V2P_ERR_INVALID;
    }
    return launch_motion_tables_build(num_frames_total, local_rot, root_trans, frame_clip, clip_start, clip_frames, clip_dt, parents, local_pos, per_clip_skeleton ? 1 : 0,
                                      gts, grs, lrs, grvs, gravs, dvs, (hipStream_t)stream);
}

int v2p_shapes_compile(int32_t num_jobs, const double* points, const int32_t* job_offsets, int32_t max_points, const double* dirs, const int32_t* dir_offsets,
                       int32_t num_dir_tables, double density, int32_t max_verts, double eps_rel, double* mass, double* com, double* inertia, int32_t* num_verts,
                       int32_t* vert_ids, double* verts, int32_t* status, void* stream) {
    if (num_jobs < 0 || max_points < 0 || max_verts < 4 || max_verts > 64 || num_dir_tables < 1 || !(density > 0.0) || !(eps_rel >= 0.0)) { set_error("v2p_shapes_compile: bad argument"); return V2P_ERR_INVALID; }
    if (num_jobs > 0 && (!points || !job_offsets || !dirs || !dir_offsets || !mass || !com || !inertia || !num_verts || !vert_ids || !verts || !status)) {
        set_error("v2p_shapes_compile: null buffer");
        return V2P_ERR_INVALID;
    }
    return launch_shape_compile(num_jobs, points, job_offsets, max_points, dirs, dir_offsets, num_dir_tables, density, max_verts, eps_rel, mass, com, inertia,
                                num_verts, vert_ids, verts, status, (hipStream_t)stream);
}

int v2p_ball_rollout(const v2p_ball_sim* c, int64_t n, const float* launch_pos, const float* launch_vel, const float* launch_vspin,
                     const v2p_ball_rollout_out* out, void* stream) {
    // every refusal comes before the first HIP call
    if (!c || !out) { set_error("v2p_ball_rollout: null cfg / out"); return V2P_ERR_INVALID; }
    if (n < 0) { set_error("v2p_ball_rollout: n %lld < 0", (long long)n); return V2P_ERR_INVALID; }
    if (n > 0 && (!launch_pos || !launch_vel || !launch_vspin)) { set_error("v2p_ball_rollout: null launch array"); return V2P_ERR_INVALID; }
    if (c->substeps < 1 || c->control_freq_inv < 1 || c->num_iterations < 1 || c->num_frames < 1) {
        set_error("v2p_ball_rollout: substeps %d, control_freq_inv %d, num_iterations %d and num_frames %d must all be >= 1", c->substeps, c->control_freq_inv,
                  c->num_iterations, c->num_frames);
        return V2P_ERR_INVALID;
    }
    if (c->solver_type != 0 && c->solver_type != 1) { set_error("v2p_ball_rollout: solver_type %d is neither 0 (PGS) nor 1 (TGS)", c->solver_type); return V2P_ERR_INVALID; }
    if (!(c->mass > 0.f) || !(c->inertia > 0.f) || !(c->radius > 0.f)) {
        set_error("v2p_ball_rollout: mass %g, inertia %g and radius %g must be > 0", (double)c->mass, (double)c->inertia, (double)c->radius);
        return V2P_ERR_INVALID;
    }
    if (!(c->sim_dt > 0.f)) { set_error("v2p_ball_rollout: sim_dt %g <= 0", (double)c->sim_dt); return V2P_ERR_INVALID; }
    if (c->resample) {
        if (c->enable_ground) { set_error("v2p_ball_rollout: resample needs enable_ground = 0 (the outgoing tables are flights without a bounce)"); return V2P_ERR_INVALID; }
        if (!(c->grid_x[2] > 0.0) || !(c->grid_y[2] > 0.0)) { set_error("v2p_ball_rollout: resample with a non-positive grid step"); return V2P_ERR_INVALID; }
        if (ball_grid_cells(c->grid_x) < 1 || ball_grid_cells(c->grid_y) < 1) { set_error("v2p_ball_rollout: resample needs both grids (lo < hi, at most 1e6 cells)"); return V2P_ERR_INVALID; }
        if (n > 0 && (!out->traj_x || !out->traj_y)) { set_error("v2p_ball_rollout: resample needs traj_x and traj_y"); return V2P_ERR_INVALID; }
    }
    if (n == 0) return V2P_OK;
    return launch_ball_rollout(*c, n, launch_pos, launch_vel, launch_vspin, *out, (hipStream_t)stream);
}

// what both tennis entry points refuse; `step`: the buffers only the whole step touches are required too
static int tennis_check(const char* fn, const v2p_tennis_cfg* c, int64_t n, const v2p_tennis_buffers* b, bool step) {
    if (!c || !b) { set_error("%s: null cfg / buffers", fn); return V2P_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %lld < 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (c->obs_ball_traj_length < 1 || c->obs_ball_traj_length > V2P_TENNIS_TRAJ_FRAMES) {
        set_error("%s: obs_ball_traj_length %d outside 1..%d", fn, c->obs_ball_traj_length, V2P_TENNIS_TRAJ_FRAMES);
        return V2P_ERR_INVALID;
    }
    if (c->reward_type < V2P_TENNIS_REWARD_REACH || c->reward_type > V2P_TENNIS_REWARD_RETURN_W_ESTIMATE) {
        set_error("%s: unknown reward type %d", fn, c->reward_type);
        return V2P_ERR_INVALID;
    }
    if (n == 0) return V2P_OK;
    bool ok = b->rb_state && b->root_states && b->racket_state && b->ball_state && b->wrist_link && b->obs && b->racket_pos && b->racket_normal;
    ok = ok && (c->use_history_ball_obs ? b->ball_obs != nullptr : (b->ball_traj && b->traj_cursor));
    ok = ok && (!c->use_random_ball_target || b->target_bounce_pos);
    if (step) {
        ok = ok && b->has_bounce && b->has_bounce_now && b->bounce_pos && b->phase_pred && b->traj_out_x && b->traj_out_y && b->tar_time_total &&
             b->tar_action && b->target_bounce_pos && b->has_racket_contact && b->has_racket_contact_now && b->tar_time && b->progress && b->prev_ball_vy &&
             b->bounce_in && b->est_bounce_pos && b->est_bounce_time && b->est_max_height && b->est_bounce_in && b->distance && b->vel_x_overflow &&
             b->rew && b->sub_rewards && b->reset && b->terminate && b->reset_reaction && b->reset_recovery;
        ok = ok && (c->reward_type == V2P_TENNIS_REWARD_RETURN_W_ESTIMATE ? b->swing_type_cycle != nullptr : b->swing_type != nullptr);
    }
    if (!ok) { set_error("%s: null buffer", fn); return V2P_ERR_INVALID; }
    if (step) {
        if (c->table_rows < 1 || c->table_nx < 1 || c->table_ny < 1) { set_error("%s: the estimator tables have no cells", fn); return V2P_ERR_INVALID; }
        for (int g = 0; g < 5; ++g)
            if (!(c->grid[g][2] > 0.0) || !(c->grid[g][1] > c->grid[g][0])) { set_error("%s: grid %d is not (lo < hi, step > 0)", fn, g); return V2P_ERR_INVALID; }
    }
    return V2P_OK;
}

int v2p_tennis_task_step(const v2p_tennis_cfg* c, int64_t n, const v2p_tennis_buffers* b, const char** names, void* stream) {
    const int rc = tennis_check("v2p_tennis_task_step", c, n, b, true);
    if (rc != V2P_OK) return rc;
    if (names) *names = c->reward_type == V2P_TENNIS_REWARD_REACH ? "pos_reward" : "pos_reward,ball_pos_reward";
    if (n == 0) return V2P_OK;
    return launch_tennis_task_step(*c, n, *b, (hipStream_t)stream);
}

int v2p_tennis_task_obs(const v2p_tennis_cfg* c, int64_t num_envs, const v2p_tennis_buffers* b, const int64_t* env_ids, int64_t n_ids, void* stream) {
    const int rc = tennis_check("v2p_tennis_task_obs", c, n_ids, b, false);
    if (rc != V2P_OK) return rc;
    if (num_envs < 0 || (n_ids > 0 && !env_ids)) { set_error("v2p_tennis_task_obs: num_envs %lld < 0 or null env_ids", (long long)num_envs); return V2P_ERR_INVALID; }
    if (n_ids == 0 || num_envs == 0) return V2P_OK;
    return launch_tennis_task_obs(*c, num_envs, *b, env_ids, n_ids, (hipStream_t)stream);
}

int v2p_tennis_eval_step(const v2p_tennis_cfg* c, const v2p_tennis_eval_cfg* ec, int64_t n, const v2p_tennis_buffers* b, const v2p_tennis_eval_buffers* x, int64_t frame,
                         const char** names, void* stream) {
    const char* fn = "v2p_tennis_eval_step";
    if (!ec || !x) { set_error("%s: null eval cfg / eval buffers", fn); return V2P_ERR_INVALID; }
    if (n <= 0) { set_error("%s: n %lld <= 0", fn, (long long)n); return V2P_ERR_INVALID; }
    const int rc = tennis_check(fn, c, n, b, true);
    if (rc != V2P_OK) return rc;
    if (!b->swing_type_cycle) { set_error("%s: null swing_type_cycle (the fh_ratio meter reads it under every reward law)", fn); return V2P_ERR_INVALID; }
    for (int m = 0; m < V2P_TENNIS_METERS; ++m)
        if (!x->meter_sum[m] || !x->meter_count[m] || !x->meter_avg[m] || !x->meter_max[m]) { set_error("%s: null array of meter %d", fn, m); return V2P_ERR_INVALID; }
    const int given = (x->dof_state != nullptr) + (x->joint_rot != nullptr) + (x->root_pos != nullptr) + (x->ball_pos != nullptr) + (x->target_pos != nullptr) +
                      (x->phase != nullptr) + (x->swing_type_cycle != nullptr);
    if (given != 0 && given != 7) { set_error("%s: a record needs dof_state and all six of its arrays (%d of 7 given)", fn, given); return V2P_ERR_INVALID; }
    if (given) {
        if (frame < 0 || frame >= ec->num_frames) { set_error("%s: frame %lld outside [0, %lld)", fn, (long long)frame, (long long)ec->num_frames); return V2P_ERR_INVALID; }
        uint32_t seen = 0;
        for (int s = 0; s < V2P_NUM_BODIES; ++s) {
            const int body = ec->body_of_smpl[s];
            if (body < 0 || body >= V2P_NUM_BODIES || (seen >> body & 1u)) { set_error("%s: body_of_smpl[%d] = %d: not a permutation of 0..%d", fn, s, body, V2P_NUM_BODIES - 1); return V2P_ERR_INVALID; }
            seen |= 1u << body;
        }
        if (ec->body_of_smpl[0] != 0) { set_error("%s: body_of_smpl[0] = %d: SMPL joint 0 must be the root body", fn, ec->body_of_smpl[0]); return V2P_ERR_INVALID; }
    }
    if (names) *names = c->reward_type == V2P_TENNIS_REWARD_REACH ? "pos_reward" : "pos_reward,ball_pos_reward";
    return launch_tennis_eval_step(*c, *ec, n, *b, *x, frame, (hipStream_t)stream);
}

// what both entry points of the two-player batch refuse
static int tennis_dual_check(const char* fn, const v2p_tennis_cfg* c, const v2p_tennis_dual_cfg* dc, int64_t n, const v2p_tennis_buffers* b) {
    if (!c || !dc || !b) { set_error("%s: null cfg / dual cfg / buffers", fn); return V2P_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %lld < 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (n % 2) { set_error("%s: n %lld is odd (envs 2k and 2k+1 are opponents)", fn, (long long)n); return V2P_ERR_INVALID; }
    if (c->obs_ball_traj_length < 1 || c->obs_ball_traj_length > V2P_TENNIS_TRAJ_FRAMES) {
        set_error("%s: obs_ball_traj_length %d outside 1..%d", fn, c->obs_ball_traj_length, V2P_TENNIS_TRAJ_FRAMES);
        return V2P_ERR_INVALID;
    }
    if (c->reward_type < V2P_TENNIS_REWARD_REACH || c->reward_type > V2P_TENNIS_REWARD_RETURN_W_ESTIMATE) {
        set_error("%s: unknown reward type %d", fn, c->reward_type);
        return V2P_ERR_INVALID;
    }
    if (n == 0) return V2P_OK;
    // the observation's buffers, which both launches write
    bool ok = b->rb_state && b->root_states && b->racket_state && b->ball_state && b->wrist_link && b->obs && b->racket_pos && b->racket_normal;
    ok = ok && (c->use_history_ball_obs ? b->ball_obs != nullptr : (b->ball_traj && b->traj_cursor));
    ok = ok && (!c->use_random_ball_target || b->target_bounce_pos);
    ok = ok && b->reset_reaction && b->reset_recovery && b->has_racket_contact && b->tar_time && b->prev_ball_vy && b->bounce_in;
    ok = ok && (c->reward_type != V2P_TENNIS_REWARD_RETURN_W_ESTIMATE || (b->est_bounce_pos && b->est_bounce_time && b->est_max_height && b->est_bounce_in));
    if (!ok) { set_error("%s: null buffer", fn); return V2P_ERR_INVALID; }
    return V2P_OK;
}

int v2p_tennis_dual_step(const v2p_tennis_cfg* c, const v2p_tennis_dual_cfg* dc, int64_t n, const v2p_tennis_buffers* b, const char** names, void* stream) {
    const char* fn = "v2p_tennis_dual_step";
    const int rc = tennis_dual_check(fn, c, dc, n, b);
    if (rc != V2P_OK) return rc;
    if (names) *names = c->reward_type == V2P_TENNIS_REWARD_REACH ? "pos_reward" : "pos_reward,ball_pos_reward";
    if (n == 0) return V2P_OK;
    bool ok = b->has_bounce && b->has_bounce_now && b->bounce_pos && b->phase_pred && b->tar_action && b->target_bounce_pos && b->has_racket_contact_now &&
              b->progress && b->est_bounce_pos && b->est_bounce_time && b->est_max_height && b->est_bounce_in && b->distance && b->rew && b->sub_rewards && b->reset;
    ok = ok && (c->reward_type == V2P_TENNIS_REWARD_RETURN_W_ESTIMATE ? b->swing_type_cycle != nullptr : b->swing_type != nullptr);
    if (!ok) { set_error("%s: null buffer", fn); return V2P_ERR_INVALID; }
    return launch_tennis_dual_step(*c, *dc, n, *b, (hipStream_t)stream);
}

int v2p_tennis_dual_handover(const v2p_tennis_cfg* c, const v2p_tennis_dual_cfg* dc, int64_t n, const v2p_tennis_buffers* b, const v2p_tennis_dual_buffers* db,
                             void* stream) {
    const char* fn = "v2p_tennis_dual_handover";
    const int rc = tennis_dual_check(fn, c, dc, n, b);
    if (rc != V2P_OK) return rc;
    if (!db) { set_error("%s: null dual buffers", fn); return V2P_ERR_INVALID; }
    if (dc->in_frames < 1 || dc->in_frames > V2P_TENNIS_TRAJ_FRAMES) { set_error("%s: in_frames %d outside 1..%d", fn, dc->in_frames, V2P_TENNIS_TRAJ_FRAMES); return V2P_ERR_INVALID; }
    if (dc->in_rows < 1 || dc->in_rows > INT32_MAX) { set_error("%s: the in-estimator's table has %lld rows (1..2^31-1)", fn, (long long)dc->in_rows); return V2P_ERR_INVALID; }
    for (int g = 0; g < 4; ++g)
        if (!(dc->in_grid[g][2] > 0.0) || !(dc->in_grid[g][1] > dc->in_grid[g][0])) { set_error("%s: in_grid %d is not (lo < hi, step > 0)", fn, g); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    if (c->use_random_ball_target && !db->target_draw) { set_error("%s: use_random_ball_target needs target_draw", fn); return V2P_ERR_INVALID; }
    bool ok = db->traj_in && db->ball_state && db->has_bounce && db->bounce_pos && db->tar_action && db->num_reset_reaction;
    ok = ok && (c->use_history_ball_obs || db->ball_traj) && (!c->use_random_ball_target || db->target_bounce_pos);
    if (!ok) { set_error("%s: null dual buffer", fn); return V2P_ERR_INVALID; }
    return launch_tennis_dual_handover(*c, *dc, n, *b, *db, (hipStream_t)stream);
}

int v2p_controller_actions(const v2p_controller_actions_cfg* c, int64_t n, const v2p_controller_actions_buffers* b, void* stream) {
    const char* fn = "v2p_controller_actions";
    if (!c || !b) { set_error("%s: null cfg / buffers", fn); return V2P_ERR_INVALID; }
    if (n < 0 || n > INT32_MAX) { set_error("%s: n %lld outside 0..2^31-1", fn, (long long)n); return V2P_ERR_INVALID; }
    if (c->num_res_dof < 0 || c->num_res_root < 0 || c->num_res_dof > 1024 || c->num_res_root > 1024) {
        set_error("%s: num_res_dof %d / num_res_root %d outside 0..1024", fn, c->num_res_dof, c->num_res_root);
        return V2P_ERR_INVALID;
    }
    const int64_t width = V2P_MVAE_LATENT + c->num_res_dof + c->num_res_root;
    if (b->actions_stride < width) { set_error("%s: actions_stride %lld below the %lld columns of a row", fn, (long long)b->actions_stride, (long long)width); return V2P_ERR_INVALID; }
    if (!(c->clamp >= 0.f)) { set_error("%s: clamp %g is negative or NaN", fn, (double)c->clamp); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    bool ok = b->actions && b->actions_out && b->mvae_actions && (!c->random_walk || b->tar_action);
    ok = ok && (c->num_res_dof == 0 || b->res_dof_actions) && (c->num_res_root == 0 || b->res_root_actions);
    if (!ok) { set_error("%s: null buffer", fn); return V2P_ERR_INVALID; }
    return launch_controller_actions(*c, n, *b, (hipStream_t)stream);
}

int v2p_tennis_task_reset(const v2p_tennis_cfg* c, const v2p_tennis_reset_cfg* rc, int64_t n, const v2p_tennis_buffers* b, const v2p_tennis_reset_buffers* r, void* stream) {
    const char* fn = "v2p_tennis_task_reset";
    if (!c || !rc || !b || !r) { set_error("%s: null cfg / reset cfg / buffers / reset buffers", fn); return V2P_ERR_INVALID; }
    if (n < 0 || n > INT32_MAX) { set_error("%s: n %lld outside 0..2^31-1", fn, (long long)n); return V2P_ERR_INVALID; }
    if (c->obs_ball_traj_length < 1 || c->obs_ball_traj_length > V2P_TENNIS_TRAJ_FRAMES) {
        set_error("%s: obs_ball_traj_length %d outside 1..%d", fn, c->obs_ball_traj_length, V2P_TENNIS_TRAJ_FRAMES);
        return V2P_ERR_INVALID;
    }
    if (rc->pool_rows < 1 || rc->pool_rows > INT32_MAX) { set_error("%s: the pool has %lld rows (1..2^31-1)", fn, (long long)rc->pool_rows); return V2P_ERR_INVALID; }
    if (rc->pool_frames < 1 || rc->pool_frames > V2P_TENNIS_TRAJ_FRAMES) { set_error("%s: pool_frames %d outside 1..%d", fn, rc->pool_frames, V2P_TENNIS_TRAJ_FRAMES); return V2P_ERR_INVALID; }
    if (rc->pool_stride < 7 + 3 * (int64_t)rc->pool_frames) { set_error("%s: pool_stride %lld below 7 + 3 x %d frames", fn, (long long)rc->pool_stride, rc->pool_frames); return V2P_ERR_INVALID; }
    if (rc->target_mode < V2P_TENNIS_TARGET_OFF || rc->target_mode > V2P_TENNIS_TARGET_CONTINUOUS) { set_error("%s: unknown target mode %d", fn, rc->target_mode); return V2P_ERR_INVALID; }
    if (rc->pool_rule != V2P_TENNIS_POOL_RANDOM && rc->pool_rule != V2P_TENNIS_POOL_ROUND_ROBIN) { set_error("%s: unknown pool rule %d", fn, rc->pool_rule); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    bool ok = b->rb_state && b->root_states && b->racket_state && b->wrist_link && b->reset_reaction && b->reset_recovery && b->tar_time && b->prev_ball_vy && b->traj_cursor;
    ok = ok && b->bounce_in && b->est_bounce_pos && b->est_bounce_time && b->est_max_height && b->est_bounce_in && b->racket_pos && b->racket_normal && b->obs;
    ok = ok && (!c->use_history_ball_obs || b->ball_obs) && (c->use_history_ball_obs || b->ball_traj) && (!c->use_random_ball_target || b->target_bounce_pos);
    if (!ok) { set_error("%s: null buffer", fn); return V2P_ERR_INVALID; }
    ok = r->pool && r->ball_state && r->has_bounce && r->bounce_pos && r->has_racket_contact && r->ball_traj && r->tar_time_total && r->tar_action && r->num_reset_reaction;
    ok = ok && r->swing_type_cycle && (rc->pool_rule != V2P_TENNIS_POOL_ROUND_ROBIN || r->sample_idx) && (rc->target_mode == V2P_TENNIS_TARGET_OFF || r->target_bounce_pos);
    if (!ok) { set_error("%s: null reset buffer", fn); return V2P_ERR_INVALID; }
    // the observation reads the window and the target through v2p_tennis_buffers: they must be the memory this launch writes
    if ((!c->use_history_ball_obs && b->ball_traj != r->ball_traj) || (c->use_random_ball_target && rc->target_mode != V2P_TENNIS_TARGET_OFF && b->target_bounce_pos != r->target_bounce_pos)) {
        set_error("%s: ball_traj / target_bounce_pos of the two buffer structs are not the same memory", fn);
        return V2P_ERR_INVALID;
    }
    return launch_tennis_task_reset(*c, *rc, n, *b, *r, (hipStream_t)stream);
}

// what both motion-generator entry points refuse; `step`: the decoder's weights are required too
static int mvae_check(const char* fn, const v2p_mvae_cfg* c, int64_t n, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, bool step) {
    if (!c || !w || !b) { set_error("%s: null cfg / weights / buffers", fn); return V2P_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %lld < 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (c->frame_size != V2P_MVAE_FRAME || c->latent_size != V2P_MVAE_LATENT || c->hidden_size != V2P_MVAE_HIDDEN || c->num_experts != V2P_MVAE_EXPERTS ||
        c->gate_hidden_size != V2P_MVAE_GATE || c->num_condition_frames != 1 || c->num_future_predictions != 1 || c->predict_phase != 1) {
        set_error("%s: only the shipped architecture is built (frame 288, latent 32, hidden 256, 6 experts, gate 64, 1 condition frame, 1 prediction, predicted phase); "
                  "got frame %d, latent %d, hidden %d, %d experts, gate %d, %d condition frames, %d predictions, predict_phase %d", fn, c->frame_size, c->latent_size,
                  c->hidden_size, c->num_experts, c->gate_hidden_size, c->num_condition_frames, c->num_future_predictions, c->predict_phase);
        return V2P_ERR_INVALID;
    }
    if (c->player < V2P_MVAE_PLAYER_DJOKOVIC || c->player > V2P_MVAE_PLAYER_NADAL) { set_error("%s: unknown player %d", fn, c->player); return V2P_ERR_INVALID; }
    bool ok = w->avg && w->std && b->conditions && b->root_pos && b->root_vel && b->joint_rot6d && b->joint_rotmat && b->phase_pred && b->swing_type && b->swing_type_cycle &&
              (c->is_train || b->joint_rot);
    if (step) ok = ok && w->w0 && w->b0 && w->w1 && w->b1 && w->w2 && w->b2 && w->gate_w0 && w->gate_b0 && w->gate_w1 && w->gate_b1 && w->gate_w2 && w->gate_b2;
    else ok = ok && b->racket_pos && b->racket_normal;
    if (!ok) { set_error("%s: null weight / buffer", fn); return V2P_ERR_INVALID; }
    return V2P_OK;
}

int v2p_mvae_step(const v2p_mvae_cfg* c, int64_t n, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, const float* latents, const float* residual, void* stream) {
    const int rc = mvae_check("v2p_mvae_step", c, n, w, b, true);
    if (rc != V2P_OK) return rc;
    if (n > 0 && !latents) { set_error("v2p_mvae_step: null latents"); return V2P_ERR_INVALID; }
    if (residual && !c->add_residual_dof) { set_error("v2p_mvae_step: a residual without add_residual_dof"); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    return launch_mvae_step(*c, n, *w, *b, latents, residual, (hipStream_t)stream);
}

int v2p_mvae_reset(const v2p_mvae_cfg* c, int64_t num_envs, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, const int64_t* env_ids, int64_t n_ids,
                   const float* init_feature, const float* root_xy, const float* joint_pos_bind_rel, void* stream) {
    const int rc = mvae_check("v2p_mvae_reset", c, n_ids, w, b, false);
    if (rc != V2P_OK) return rc;
    if (num_envs < 0) { set_error("v2p_mvae_reset: num_envs %lld < 0", (long long)num_envs); return V2P_ERR_INVALID; }
    if (n_ids > 0 && (!env_ids || !init_feature || !root_xy || !joint_pos_bind_rel)) {
        set_error("v2p_mvae_reset: null env_ids / init_feature / root_xy / joint_pos_bind_rel");
        return V2P_ERR_INVALID;
    }
    if (n_ids == 0 || num_envs == 0) return V2P_OK;
    return launch_mvae_reset(*c, num_envs, *w, *b, env_ids, n_ids, init_feature, root_xy, joint_pos_bind_rel, (hipStream_t)stream);
}

int v2p_mvae_reset_flagged(const v2p_mvae_cfg* c, int64_t num_envs, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, const int64_t* flags, const float* init_feature,
                           const float* root_xy, const v2p_mvae_root_rule* rule, const float* joint_pos_bind_rel, void* stream) {
    const char* fn = "v2p_mvae_reset_flagged";
    const int rc = mvae_check(fn, c, num_envs, w, b, false);
    if (rc != V2P_OK) return rc;
    if (num_envs > INT32_MAX) { set_error("%s: num_envs %lld above 2^31-1 (the generator's counter holds the env in 32 bits)", fn, (long long)num_envs); return V2P_ERR_INVALID; }
    if (!flags || !init_feature || !joint_pos_bind_rel) { set_error("%s: null flags / init_feature / joint_pos_bind_rel", fn); return V2P_ERR_INVALID; }
    if (!root_xy && !rule) { set_error("%s: neither root_xy nor a rule for the start", fn); return V2P_ERR_INVALID; }
    if (rule && rule->rule != V2P_MVAE_ROOT_CENTRE && rule->rule != V2P_MVAE_ROOT_DRAW) { set_error("%s: unknown root rule %d", fn, rule->rule); return V2P_ERR_INVALID; }
    if (num_envs == 0) return V2P_OK;
    const v2p_mvae_root_rule none = {V2P_MVAE_ROOT_CENTRE, 0, 0};
    return launch_mvae_reset_flagged(*c, num_envs, *w, *b, flags, init_feature, root_xy, rule ? *rule : none, joint_pos_bind_rel, (hipStream_t)stream);
}

// what both two-player entry points refuse: each side's own refusals, and sides that disagree on what the batch shares
static int mvae_dual_check(const char* fn, const v2p_mvae_cfg* c, int64_t n, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, bool step) {
    if (!c || !w || !b) { set_error("%s: null cfg / weights / buffers", fn); return V2P_ERR_INVALID; }
    for (int side = 0; side < 2; ++side) {
        const int rc = mvae_check(fn, c + side, n, w + side, b, step);
        if (rc != V2P_OK) return rc;
    }
    if (c[0].is_train != c[1].is_train || c[0].add_residual_dof != c[1].add_residual_dof) {
        set_error("%s: the two sides disagree on is_train (%d, %d) or add_residual_dof (%d, %d)", fn, c[0].is_train, c[1].is_train, c[0].add_residual_dof, c[1].add_residual_dof);
        return V2P_ERR_INVALID;
    }
    return V2P_OK;
}

int v2p_mvae_dual_step(const v2p_mvae_cfg* c, int64_t n, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, const float* latents, const float* residual, int32_t mapping,
                       void* stream) {
    const int rc = mvae_dual_check("v2p_mvae_dual_step", c, n, w, b, true);
    if (rc != V2P_OK) return rc;
    if (n & 1) { set_error("v2p_mvae_dual_step: n %lld is odd (envs 2k and 2k+1 are a pair)", (long long)n); return V2P_ERR_INVALID; }
    if (mapping != V2P_MVAE_DUAL_MAP_PARITY && mapping != V2P_MVAE_DUAL_MAP_HALVES) { set_error("v2p_mvae_dual_step: unknown mapping %d", mapping); return V2P_ERR_INVALID; }
    if (n > 0 && !latents) { set_error("v2p_mvae_dual_step: null latents"); return V2P_ERR_INVALID; }
    if (residual && !c[0].add_residual_dof) { set_error("v2p_mvae_dual_step: a residual without add_residual_dof"); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    const v2p_mvae_cfg (&c2)[2] = *reinterpret_cast<const v2p_mvae_cfg(*)[2]>(c);
    const v2p_mvae_weights (&w2)[2] = *reinterpret_cast<const v2p_mvae_weights(*)[2]>(w);
    return launch_mvae_dual_step(c2, n, w2, *b, latents, residual, mapping, (hipStream_t)stream);
}

int v2p_mvae_dual_reset(const v2p_mvae_cfg* c, int64_t num_envs, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, const v2p_mvae_racket* racket, const int64_t* env_ids,
                        int64_t n_ids, const float* init_feature, const float* root_xy, const float* joint_pos_bind_rel, int64_t bind_rows, void* stream) {
    const int rc = mvae_dual_check("v2p_mvae_dual_reset", c, n_ids, w, b, false);
    if (rc != V2P_OK) return rc;
    if (!racket) { set_error("v2p_mvae_dual_reset: null racket"); return V2P_ERR_INVALID; }
    if (num_envs < 0) { set_error("v2p_mvae_dual_reset: num_envs %lld < 0", (long long)num_envs); return V2P_ERR_INVALID; }
    if (n_ids > 0 && (!env_ids || !init_feature || !root_xy || !joint_pos_bind_rel)) {
        set_error("v2p_mvae_dual_reset: null env_ids / init_feature / root_xy / joint_pos_bind_rel");
        return V2P_ERR_INVALID;
    }
    if (bind_rows < 1 || (bind_rows > 1 && 2 * bind_rows < n_ids)) {
        set_error("v2p_mvae_dual_reset: joint_pos_bind_rel has %lld rows; the pair at list positions 2i, 2i+1 reads row i: 1 row or at least %lld", (long long)bind_rows,
                  (long long)((n_ids + 1) / 2));
        return V2P_ERR_INVALID;
    }
    if (n_ids == 0 || num_envs == 0) return V2P_OK;
    const v2p_mvae_cfg (&c2)[2] = *reinterpret_cast<const v2p_mvae_cfg(*)[2]>(c);
    const v2p_mvae_weights (&w2)[2] = *reinterpret_cast<const v2p_mvae_weights(*)[2]>(w);
    return launch_mvae_dual_reset(c2, num_envs, w2, *b, *racket, env_ids, n_ids, init_feature, root_xy, joint_pos_bind_rel, bind_rows, (hipStream_t)stream);
}

// what the three imitation-target entry points refuse (cfg and buffers common to them); `fn` names the call
static int mvae_target_check(const char* fn, const v2p_mvae_target_cfg* c, int64_t n, const v2p_mvae_target_buffers* b) {
    if (!c || !b) { set_error("%s: null cfg / buffers", fn); return V2P_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %lld < 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (!(c->dt > 0.f)) { set_error("%s: dt %g <= 0", fn, (double)c->dt); return V2P_ERR_INVALID; }
    if (c->head_body < 0 || c->head_body >= NB || c->smpl_head < 0 || c->smpl_head >= NB || c->smpl_neck < 0 || c->smpl_neck >= NB) {
        set_error("%s: head body %d / SMPL head %d / SMPL neck %d outside 0..%d", fn, c->head_body, c->smpl_head, c->smpl_neck, NB - 1);
        return V2P_ERR_INVALID;
    }
    for (int k = 0; k < 4; ++k)
        if (c->key_bodies[k] < 0 || c->key_bodies[k] >= NB) { set_error("%s: key body %d outside 0..%d", fn, c->key_bodies[k], NB - 1); return V2P_ERR_INVALID; }
    unsigned seen = 0;
    for (int s = 0; s < NB; ++s) {
        const int par = c->smpl_parents[s], body = c->smpl_of_body[s];
        if (s == 0 ? par != -1 : (par < 0 || par >= s)) { set_error("%s: smpl_parents[%d] = %d is no tree with parents before children", fn, s, par); return V2P_ERR_INVALID; }
        if (body < 0 || body >= NB || (seen >> body & 1u)) { set_error("%s: smpl_of_body[%d] = %d: not a permutation of 0..%d", fn, s, body, NB - 1); return V2P_ERR_INVALID; }
        seen |= 1u << body;
    }
    if (c->smpl_of_body[0] != 0) { set_error("%s: smpl_of_body[0] = %d: body 0 must be the root joint", fn, c->smpl_of_body[0]); return V2P_ERR_INVALID; }
    if (c->smpl_of_body[c->head_body] != c->smpl_head) { set_error("%s: head body %d is not SMPL joint %d", fn, c->head_body, c->smpl_head); return V2P_ERR_INVALID; }
    if (c->num_shapes < 1) { set_error("%s: num_shapes %d < 1", fn, c->num_shapes); return V2P_ERR_INVALID; }
    return V2P_OK;
}

int v2p_mvae_target_step(const v2p_mvae_target_cfg* c, int64_t n, const v2p_mvae_target_buffers* b, void* stream) {
    const int rc = mvae_target_check("v2p_mvae_target_step", c, n, b);
    if (rc != V2P_OK) return rc;
    if (!b->root_pos || !b->joint_rotmat || !b->joint_pos_bind || !b->target || !b->prev_target) {
        set_error("v2p_mvae_target_step: null root_pos / joint_rotmat / joint_pos_bind / target / prev_target");
        return V2P_ERR_INVALID;
    }
    if (b->target == b->prev_target) { set_error("v2p_mvae_target_step: target and prev_target are the same buffer"); return V2P_ERR_INVALID; }
    if (c->fix_head_orientation && (!b->ball_state || !b->rb_state)) { set_error("v2p_mvae_target_step: fix_head_orientation needs ball_state and rb_state"); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    return launch_mvae_target_step(*c, n, *b, (hipStream_t)stream);
}

int v2p_mvae_target_reset(const v2p_mvae_target_cfg* c, int64_t num_envs, const v2p_mvae_target_buffers* b, const int64_t* env_ids, int64_t n_ids, void* stream) {
    const int rc = mvae_target_check("v2p_mvae_target_reset", c, n_ids, b);
    if (rc != V2P_OK) return rc;
    if (num_envs < 0) { set_error("v2p_mvae_target_reset: num_envs %lld < 0", (long long)num_envs); return V2P_ERR_INVALID; }
    if (!b->root_pos || !b->joint_rotmat || !b->joint_pos_bind || !b->target) { set_error("v2p_mvae_target_reset: null root_pos / joint_rotmat / joint_pos_bind / target"); return V2P_ERR_INVALID; }
    if (n_ids > 0 && !env_ids) { set_error("v2p_mvae_target_reset: null env_ids"); return V2P_ERR_INVALID; }
    if (n_ids == 0 || num_envs == 0) return V2P_OK;
    return launch_mvae_target_reset(*c, num_envs, *b, env_ids, n_ids, (hipStream_t)stream);
}

int v2p_mvae_target_reset_flagged(const v2p_mvae_target_cfg* c, int64_t num_envs, const v2p_mvae_target_buffers* b, const int64_t* flags, void* stream) {
    const char* fn = "v2p_mvae_target_reset_flagged";
    const int rc = mvae_target_check(fn, c, num_envs, b);
    if (rc != V2P_OK) return rc;
    if (!b->root_pos || !b->joint_rotmat || !b->joint_pos_bind || !b->target) { set_error("%s: null root_pos / joint_rotmat / joint_pos_bind / target", fn); return V2P_ERR_INVALID; }
    if (!flags) { set_error("%s: null flags", fn); return V2P_ERR_INVALID; }
    if (num_envs == 0) return V2P_OK;
    return launch_mvae_target_reset_flagged(*c, num_envs, *b, flags, (hipStream_t)stream);
}

// what the two bookkeeping entry points of the reset by flags refuse; `begin`: which of the buffers the call writes
static int ctl_reset_check(const char* fn, int64_t n, const int64_t* flags, const v2p_ctl_reset_buffers* b, bool begin) {
    if (n < 0) { set_error("%s: n %lld < 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (!flags || !b) { set_error("%s: null flags / buffers", fn); return V2P_ERR_INVALID; }
    const bool ok = begin ? (b->progress && b->terminate && b->num_reset_reaction && b->num_reset && b->distance) : (b->reset_reaction && b->reset_recovery);
    if (!ok) { set_error(begin ? "%s: null progress / terminate / num_reset_reaction / num_reset / distance" : "%s: null reset_reaction / reset_recovery", fn); return V2P_ERR_INVALID; }
    return V2P_OK;
}

int v2p_ctl_reset_begin(int64_t n, const int64_t* flags, const v2p_ctl_reset_buffers* b, void* stream) {
    const int rc = ctl_reset_check("v2p_ctl_reset_begin", n, flags, b, true);
    if (rc != V2P_OK || n == 0) return rc;
    return launch_ctl_reset_begin(n, flags, *b, (hipStream_t)stream);
}

int v2p_ctl_reset_end(int64_t n, int64_t* flags, const v2p_ctl_reset_buffers* b, void* stream) {
    const int rc = ctl_reset_check("v2p_ctl_reset_end", n, flags, b, false);
    if (rc != V2P_OK || n == 0) return rc;
    return launch_ctl_reset_end(n, flags, *b, (hipStream_t)stream);
}

// ---- the two-player controller's pair reset by flags (pair_reset.hip, mvae_player_dual_flagged.hip)
static int pair_check(const char* fn, int64_t n, int32_t serve_from) {
    if (n < 0) { set_error("%s: n %lld < 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (n & 1) { set_error("%s: n %lld is odd (envs 2k and 2k+1 are a pair)", fn, (long long)n); return V2P_ERR_INVALID; }
    if (serve_from != V2P_SERVE_FROM_NEAR && serve_from != V2P_SERVE_FROM_FAR) { set_error("%s: unknown serve_from %d", fn, serve_from); return V2P_ERR_INVALID; }
    return V2P_OK;
}

int v2p_ctl_pair_reset_begin(int64_t n, int64_t* flags, const v2p_ctl_reset_buffers* b, int32_t serve_from, void* stream) {
    const char* fn = "v2p_ctl_pair_reset_begin";
    const int rc = pair_check(fn, n, serve_from);
    if (rc != V2P_OK) return rc;
    if (!flags || !b) { set_error("%s: null flags / buffers", fn); return V2P_ERR_INVALID; }
    if (!b->progress || !b->terminate || !b->num_reset_reaction || !b->num_reset || !b->distance || !b->reset_reaction || !b->reset_recovery) {
        set_error("%s: null progress / terminate / num_reset_reaction / num_reset / distance / reset_reaction / reset_recovery", fn);
        return V2P_ERR_INVALID;
    }
    if (n == 0) return V2P_OK;
    return launch_ctl_pair_reset_begin(n, flags, *b, serve_from, (hipStream_t)stream);
}

int v2p_ctl_pair_reset_end(int64_t n, int64_t* flags, void* stream) {
    const char* fn = "v2p_ctl_pair_reset_end";
    const int rc = pair_check(fn, n, V2P_SERVE_FROM_NEAR);
    if (rc != V2P_OK) return rc;
    if (!flags) { set_error("%s: null flags", fn); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    return launch_ctl_pair_reset_end(n, flags, (hipStream_t)stream);
}

int v2p_tennis_dual_serve_flagged(int64_t n, const int64_t* flags, int32_t serve_from, const float* racket_pos, float* ball_state, const float* draws,
                                  const v2p_serve_rule* rule, void* stream) {
    const char* fn = "v2p_tennis_dual_serve_flagged";
    const int rc = pair_check(fn, n, serve_from);
    if (rc != V2P_OK) return rc;
    if (n > INT32_MAX) { set_error("%s: n %lld above 2^31-1 (the generator's counter holds the env in 32 bits)", fn, (long long)n); return V2P_ERR_INVALID; }
    if (!flags || !racket_pos || !ball_state) { set_error("%s: null flags / racket_pos / ball_state", fn); return V2P_ERR_INVALID; }
    if (!draws && !rule) { set_error("%s: neither draws nor a rule for the serve velocity", fn); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    const v2p_serve_rule none = {0, 0};
    return launch_tennis_dual_serve_flagged(n, flags, serve_from, racket_pos, ball_state, draws, rule ? *rule : none, (hipStream_t)stream);
}

int v2p_mvae_dual_reset_flagged(const v2p_mvae_cfg* c, int64_t num_envs, const v2p_mvae_weights* w, const v2p_mvae_buffers* b, const v2p_mvae_racket* racket,
                                const int64_t* flags, const float* init_feature, const float* root_xy, const v2p_mvae_root_rule* rule, const float* joint_pos_bind_rel,
                                int64_t bind_rows, void* stream) {
    const char* fn = "v2p_mvae_dual_reset_flagged";
    const int rc = mvae_dual_check(fn, c, num_envs, w, b, false);
    if (rc != V2P_OK) return rc;
    if (num_envs & 1) { set_error("%s: num_envs %lld is odd (envs 2k and 2k+1 are a pair)", fn, (long long)num_envs); return V2P_ERR_INVALID; }
    if (num_envs > INT32_MAX) { set_error("%s: num_envs %lld above 2^31-1 (the generator's counter holds the env in 32 bits)", fn, (long long)num_envs); return V2P_ERR_INVALID; }
    if (!racket) { set_error("%s: null racket", fn); return V2P_ERR_INVALID; }
    if (!flags || !init_feature || !joint_pos_bind_rel) { set_error("%s: null flags / init_feature / joint_pos_bind_rel", fn); return V2P_ERR_INVALID; }
    if (!root_xy && !rule) { set_error("%s: neither root_xy nor a rule for the start", fn); return V2P_ERR_INVALID; }
    if (rule && rule->rule != V2P_MVAE_ROOT_CENTRE && rule->rule != V2P_MVAE_ROOT_DRAW) { set_error("%s: unknown root rule %d", fn, rule->rule); return V2P_ERR_INVALID; }
    if (bind_rows < 1) { set_error("%s: joint_pos_bind_rel has %lld rows", fn, (long long)bind_rows); return V2P_ERR_INVALID; }
    if (bind_rows > 1) {
        set_error("%s: joint_pos_bind_rel has %lld rows: the id-list reset reads the row of a pair's position in the list, which without a list is a prefix count of the "
                  "flagged pairs - not built; one [24,3] row", fn, (long long)bind_rows);
        return V2P_ERR_UNSUPPORTED;
    }
    if (num_envs == 0) return V2P_OK;
    const v2p_mvae_root_rule none = {V2P_MVAE_ROOT_CENTRE, 0, 0};
    const v2p_mvae_cfg (&c2)[2] = *reinterpret_cast<const v2p_mvae_cfg(*)[2]>(c);
    const v2p_mvae_weights (&w2)[2] = *reinterpret_cast<const v2p_mvae_weights(*)[2]>(w);
    return launch_mvae_dual_reset_flagged(c2, num_envs, w2, *b, *racket, flags, init_feature, root_xy, rule ? *rule : none, joint_pos_bind_rel, (hipStream_t)stream);
}

// ---- the record of a match run (match_record.hip)
static int match_record_check(const char* fn, const v2p_match_record_cfg* c, int64_t n, const v2p_match_record_buffers* b) {
    if (!c || !b) { set_error("%s: null cfg / buffers", fn); return V2P_ERR_INVALID; }
    if (n <= 0) { set_error("%s: n %lld <= 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (n & 1) { set_error("%s: n %lld is odd (envs 2k and 2k+1 are a pair)", fn, (long long)n); return V2P_ERR_INVALID; }
    if (n > INT32_MAX) { set_error("%s: n %lld above 2^31-1 (best_pair holds the pair in 32 bits)", fn, (long long)n); return V2P_ERR_INVALID; }
    if (c->record_length < 1 || c->record_length > V2P_MATCH_RECORD_MAX_LENGTH) {
        set_error("%s: record_length %lld outside 1..%d", fn, (long long)c->record_length, V2P_MATCH_RECORD_MAX_LENGTH);
        return V2P_ERR_INVALID;
    }
    if (c->num_best < 1 || c->num_best > V2P_MATCH_RECORD_MAX_BEST) { set_error("%s: num_best %d outside 1..%d", fn, c->num_best, V2P_MATCH_RECORD_MAX_BEST); return V2P_ERR_INVALID; }
    const int fault = match_record_body_fault(*c);
    if (fault >= 0) {
        set_error("%s: body_of_smpl[%d] = %d: not a permutation of 0..%d with the root body first", fn, fault, c->body_of_smpl[fault], V2P_NUM_BODIES - 1);
        return V2P_ERR_INVALID;
    }
    const void* arrays[] = {b->rb_state, b->dof_state, b->ball_state, b->phase_pred, b->swing_type_cycle, b->tar_action, b->progress, b->reset, b->distance,
                            b->joint_rot_all, b->root_pos_all, b->ball_pos_all, b->phase_all, b->swing_type_all, b->tar_action_all, b->overflow,
                            b->best_distance, b->best_pair, b->best_nframes, b->best_slot, b->best_count, b->decision,
                            b->best_joint_rot, b->best_root_pos, b->best_ball_pos, b->best_phase, b->best_swing_type, b->best_tar_action};
    for (size_t i = 0; i < sizeof(arrays) / sizeof(arrays[0]); ++i)
        if (!arrays[i]) { set_error("%s: null array (field %d of v2p_match_record_buffers)", fn, (int)i); return V2P_ERR_INVALID; }
    return V2P_OK;
}

int v2p_match_record_frame(const v2p_match_record_cfg* c, int64_t n, const v2p_match_record_buffers* b, void* stream) {
    const int rc = match_record_check("v2p_match_record_frame", c, n, b);
    if (rc != V2P_OK) return rc;
    return launch_match_record_frame(*c, n, *b, (hipStream_t)stream);
}

int v2p_match_record_select(const v2p_match_record_cfg* c, int64_t n, const v2p_match_record_buffers* b, void* stream) {
    const int rc = match_record_check("v2p_match_record_select", c, n, b);
    if (rc != V2P_OK) return rc;
    return launch_match_record_select(*c, n, *b, (hipStream_t)stream);
}

// ---- the two-hand backhand fix of a record (two_hand_fix.hip)
int v2p_two_hand_fix(const v2p_two_hand_fix_cfg* c, int64_t num_tracks, int64_t track_length, const v2p_two_hand_fix_buffers* b, void* stream) {
    const char* fn = "v2p_two_hand_fix";
    if (!c || !b) { set_error("%s: null cfg / buffers", fn); return V2P_ERR_INVALID; }
    if (num_tracks < 0 || num_tracks > INT32_MAX) { set_error("%s: num_tracks %lld outside 0..2^31-1", fn, (long long)num_tracks); return V2P_ERR_INVALID; }
    if (track_length < 1 || track_length > INT32_MAX) { set_error("%s: track_length %lld outside 1..2^31-1", fn, (long long)track_length); return V2P_ERR_INVALID; }
    if (c->num_iters < 0) { set_error("%s: num_iters %d < 0", fn, c->num_iters); return V2P_ERR_INVALID; }
    if (c->num_bind < 1) { set_error("%s: num_bind %d < 1", fn, c->num_bind); return V2P_ERR_INVALID; }
    if (const char* why = two_hand_fix_cfg_fault(*c)) { set_error("%s: %s", fn, why); return V2P_ERR_INVALID; }
    const void* arrays[] = {b->joint_rot, b->phase, b->swing_type, b->nframes, b->righthand, b->bind, b->out, b->overflow};
    for (size_t i = 0; i < sizeof(arrays) / sizeof(arrays[0]); ++i)
        if (!arrays[i]) { set_error("%s: null array (field %d of v2p_two_hand_fix_buffers)", fn, (int)i); return V2P_ERR_INVALID; }
    if (b->out == b->joint_rot) { set_error("%s: out is joint_rot (the fix works on a copy)", fn); return V2P_ERR_INVALID; }
    if (num_tracks == 0) return V2P_OK;
    {   // the rows of `out` are the frames' workspace during the steps: no byte of it may be one of joint_rot's
        const uintptr_t bytes = (uintptr_t)num_tracks * (uintptr_t)track_length * 24u * 3u * sizeof(float);
        const uintptr_t in0 = (uintptr_t)b->joint_rot, out0 = (uintptr_t)b->out;
        if (in0 < out0 + bytes && out0 < in0 + bytes) { set_error("%s: out overlaps joint_rot (the fix works on a copy)", fn); return V2P_ERR_INVALID; }
    }
    return launch_two_hand_fix(*c, num_tracks, track_length, *b, (hipStream_t)stream);
}

int v2p_mvae_target_actions(const v2p_mvae_target_cfg* c, int64_t n, const float* actions_in, const v2p_mvae_target_buffers* b, float* actions_out, void* stream) {
    const int rc = mvae_target_check("v2p_mvae_target_actions", c, n, b);
    if (rc != V2P_OK) return rc;
    if (c->pd_target_base != V2P_PD_BASE_TARGET_POS && c->pd_target_base != V2P_PD_BASE_CURRENT_POS && c->pd_target_base != V2P_PD_BASE_NONE) {
        set_error("v2p_mvae_target_actions: unknown pd_target_base %d", c->pd_target_base);
        return V2P_ERR_INVALID;
    }
    const void* base = c->pd_target_base == V2P_PD_BASE_TARGET_POS ? (const void*)b->target : (c->pd_target_base == V2P_PD_BASE_CURRENT_POS ? (const void*)b->dof_state : (const void*)b->pd_action_offset);
    if (!base || (!c->no_scale_action && !b->pd_action_scale)) { set_error("v2p_mvae_target_actions: null base buffer / pd_action_scale"); return V2P_ERR_INVALID; }
    if (n > 0 && (!actions_in || !actions_out)) { set_error("v2p_mvae_target_actions: null actions"); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    return launch_mvae_target_actions(*c, n, actions_in, *b, actions_out, (hipStream_t)stream);
}

// what the two policy-input entry points refuse; `fn` names the call
static int policy_input_check(const char* fn, const v2p_policy_input_cfg* c, int64_t n, int64_t dim) {
    if (!c) { set_error("%s: null cfg", fn); return V2P_ERR_INVALID; }
    if (n < 0) { set_error("%s: n %lld < 0", fn, (long long)n); return V2P_ERR_INVALID; }
    if (dim < 1) { set_error("%s: dim %lld < 1", fn, (long long)dim); return V2P_ERR_INVALID; }
    if (c->sides != 1 && c->sides != 2) { set_error("%s: sides %d is neither 1 nor 2", fn, c->sides); return V2P_ERR_INVALID; }
    if (c->sides == 2 && (n & 1)) { set_error("%s: n %lld is odd with two sides", fn, (long long)n); return V2P_ERR_INVALID; }
    if (!(c->clip_obs > 0.f)) { set_error("%s: clip_obs %g is not > 0", fn, (double)c->clip_obs); return V2P_ERR_INVALID; }
    for (int s = 0; s < c->sides; ++s) {
        const v2p_policy_norm& nm = c->norm[s];
        if (nm.kind != V2P_NORM_NONE && nm.kind != V2P_NORM_RUNNING && nm.kind != V2P_NORM_MEAN_VAR) {
            set_error("%s: unknown normaliser kind %d of side %d", fn, nm.kind, s);
            return V2P_ERR_INVALID;
        }
        if (nm.kind == V2P_NORM_NONE) continue;
        if (!nm.mean || !nm.spread) { set_error("%s: null mean / spread of side %d's normaliser", fn, s); return V2P_ERR_INVALID; }
        if (!(nm.clip > 0.f)) { set_error("%s: side %d's normaliser clip %g is not > 0", fn, s, (double)nm.clip); return V2P_ERR_INVALID; }
        if (nm.kind == V2P_NORM_MEAN_VAR && !(nm.eps >= 0.f)) { set_error("%s: side %d's normaliser eps %g < 0", fn, s, (double)nm.eps); return V2P_ERR_INVALID; }
    }
    return V2P_OK;
}

int v2p_policy_input(const v2p_policy_input_cfg* c, int64_t n, int64_t dim, const float* obs, float* x, void* stream) {
    const int rc = policy_input_check("v2p_policy_input", c, n, dim);
    if (rc != V2P_OK) return rc;
    if (!obs || !x) { set_error("v2p_policy_input: null obs / x"); return V2P_ERR_INVALID; }
    if (c->sides == 2 && obs == x) { set_error("v2p_policy_input: x must not be obs with two sides"); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    return launch_policy_input(*c, n, dim, obs, x, (hipStream_t)stream);
}

int v2p_ll_policy_input(const v2p_policy_input_cfg* c, int64_t n, int64_t dim, const v2p_ll_policy_src* src, float* raw_obs, float* x, void* stream) {
    const int rc = policy_input_check("v2p_ll_policy_input", c, n, dim);
    if (rc != V2P_OK) return rc;
    if (dim != POLICY_LL_OBS) { set_error("v2p_ll_policy_input: dim %lld is not %d", (long long)dim, POLICY_LL_OBS); return V2P_ERR_INVALID; }
    if (!src || !x) { set_error("v2p_ll_policy_input: null src / x"); return V2P_ERR_INVALID; }
    if (!src->rb_state || !src->dof_state || !src->target || !src->motion_bodies) {
        set_error("v2p_ll_policy_input: null rb_state / dof_state / target / motion_bodies");
        return V2P_ERR_INVALID;
    }
    if (src->target_stride < MSD) { set_error("v2p_ll_policy_input: target_stride %lld < %d", (long long)src->target_stride, MSD); return V2P_ERR_INVALID; }
    if (raw_obs == x) { set_error("v2p_ll_policy_input: raw_obs and x are the same buffer"); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    return launch_ll_policy_input(*c, n, *src, raw_obs, x, (hipStream_t)stream);
}

int v2p_ctl_policy_head(int64_t n, int32_t num_actions, const float* mu, const float* logstd, const float* sigma, const float* noise, float clip_actions,
                        float* actions_row, float* mus_row, float* sigmas_row, float* neglogp_row, float* actions_clamped, void* stream) {
    if (n < 0) { set_error("v2p_ctl_policy_head: n %lld < 0", (long long)n); return V2P_ERR_INVALID; }
    if (num_actions < 1 || num_actions > V2P_CTL_MAX_ACTIONS) {
        set_error("v2p_ctl_policy_head: num_actions %d is outside [1, %d]", num_actions, V2P_CTL_MAX_ACTIONS);
        return V2P_ERR_INVALID;
    }
    if (!(clip_actions > 0.f)) { set_error("v2p_ctl_policy_head: clip_actions %g is not > 0", (double)clip_actions); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    if (!mu || !logstd || !sigma || !noise || !neglogp_row || !actions_clamped) {
        set_error("v2p_ctl_policy_head: null mu / logstd / sigma / noise / neglogp_row / actions_clamped");
        return V2P_ERR_INVALID;
    }
    return launch_ctl_policy_head(n, num_actions, mu, logstd, sigma, noise, clip_actions, actions_row, mus_row, sigmas_row, neglogp_row, actions_clamped,
                                  (hipStream_t)stream);
}

int v2p_ctl_rollout_record(int64_t n, int64_t obs_dim, int32_t num_sub, float clip_obs, const float* obs, const float* rew, const int64_t* reset,
                           const int64_t* terminate, const float* sub_rewards, float* next_obs_row, float* rewards_row, float* dones_row, float* terminated,
                           float* cur_rewards, float* cur_lengths, double* acc, double* sub_acc, void* stream) {
    if (n < 0) { set_error("v2p_ctl_rollout_record: n %lld < 0", (long long)n); return V2P_ERR_INVALID; }
    if (obs_dim < 1) { set_error("v2p_ctl_rollout_record: obs_dim %lld < 1", (long long)obs_dim); return V2P_ERR_INVALID; }
    if (num_sub < 0 || num_sub > V2P_CTL_MAX_SUB_REWARDS) {
        set_error("v2p_ctl_rollout_record: num_sub %d is outside [0, %d]", num_sub, V2P_CTL_MAX_SUB_REWARDS);
        return V2P_ERR_INVALID;
    }
    if (!(clip_obs > 0.f)) { set_error("v2p_ctl_rollout_record: clip_obs %g is not > 0", (double)clip_obs); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    if (!obs || !rew || !reset || !terminate || !next_obs_row || !rewards_row || !dones_row || !terminated || !cur_rewards || !cur_lengths || !acc ||
        (num_sub > 0 && (!sub_rewards || !sub_acc))) {
        set_error("v2p_ctl_rollout_record: null buffer");
        return V2P_ERR_INVALID;
    }
    return launch_ctl_rollout_record(n, obs_dim, num_sub, clip_obs, obs, rew, reset, terminate, sub_rewards, next_obs_row, rewards_row, dones_row, terminated,
                                     cur_rewards, cur_lengths, acc, sub_acc, (hipStream_t)stream);
}

int v2p_ppo_loss(const v2p_ppo_loss_cfg* c, int64_t B, const v2p_ppo_loss_buffers* b, void* stream) {
    if (!c || !b) { set_error("v2p_ppo_loss: null cfg / buffers"); return V2P_ERR_INVALID; }
    if (B < 0) { set_error("v2p_ppo_loss: B %lld < 0", (long long)B); return V2P_ERR_INVALID; }
    if (c->num_actions < 1 || c->num_actions > V2P_CTL_MAX_ACTIONS) {
        set_error("v2p_ppo_loss: num_actions %d is outside [1, %d]", c->num_actions, V2P_CTL_MAX_ACTIONS);
        return V2P_ERR_INVALID;
    }
    if (c->c0 < 0 || c->c0 > c->c1 || c->c1 > c->num_actions) {
        set_error("v2p_ppo_loss: columns [%d, %d) are not inside [0, %d]", c->c0, c->c1, c->num_actions);
        return V2P_ERR_INVALID;
    }
    if (!(c->e_clip > 0.0)) { set_error("v2p_ppo_loss: e_clip %g is not > 0", c->e_clip); return V2P_ERR_INVALID; }
    if (!b->idx && c->dataset_rows < B) { set_error("v2p_ppo_loss: dataset_rows %lld < B %lld without idx", (long long)c->dataset_rows, (long long)B); return V2P_ERR_INVALID; }
    if (B == 0) return V2P_OK;
    if (!b->mu || !b->value || !b->old_neglogp || !b->advantages || !b->returns || !b->actions || !b->old_mu || !b->old_sigma || !b->logstd || !b->sigma ||
        !b->grad_mu || !b->grad_value || !b->stats || !b->partials) {
        set_error("v2p_ppo_loss: null buffer");
        return V2P_ERR_INVALID;
    }
    return launch_ppo_loss(*c, B, *b, (hipStream_t)stream);
}

int v2p_ll_policy_actions(const v2p_mvae_target_cfg* c, int64_t n, int32_t sides, float clip_actions, const float* mu, const v2p_mvae_target_buffers* b,
                          float* actions_out, void* stream) {
    const int rc = mvae_target_check("v2p_ll_policy_actions", c, n, b);
    if (rc != V2P_OK) return rc;
    if (sides != 1 && sides != 2) { set_error("v2p_ll_policy_actions: sides %d is neither 1 nor 2", sides); return V2P_ERR_INVALID; }
    if (sides == 2 && (n & 1)) { set_error("v2p_ll_policy_actions: n %lld is odd with two sides", (long long)n); return V2P_ERR_INVALID; }
    if (!(clip_actions > 0.f)) { set_error("v2p_ll_policy_actions: clip_actions %g is not > 0", (double)clip_actions); return V2P_ERR_INVALID; }
    if (c->pd_target_base != V2P_PD_BASE_TARGET_POS && c->pd_target_base != V2P_PD_BASE_CURRENT_POS && c->pd_target_base != V2P_PD_BASE_NONE) {
        set_error("v2p_ll_policy_actions: unknown pd_target_base %d", c->pd_target_base);
        return V2P_ERR_INVALID;
    }
    const void* base = c->pd_target_base == V2P_PD_BASE_TARGET_POS ? (const void*)b->target : (c->pd_target_base == V2P_PD_BASE_CURRENT_POS ? (const void*)b->dof_state : (const void*)b->pd_action_offset);
    if (!base || (!c->no_scale_action && !b->pd_action_scale)) { set_error("v2p_ll_policy_actions: null base buffer / pd_action_scale"); return V2P_ERR_INVALID; }
    if (!mu || !actions_out) { set_error("v2p_ll_policy_actions: null mu / actions_out"); return V2P_ERR_INVALID; }
    if (sides == 2 && mu == actions_out) { set_error("v2p_ll_policy_actions: actions_out must not be mu with two sides"); return V2P_ERR_INVALID; }
    if (n == 0) return V2P_OK;
    return launch_ll_policy_actions(*c, n, sides, clip_actions, mu, *b, actions_out, (hipStream_t)stream);
}

int v2p_env_reset(v2p_env* e, const int64_t* env_ids, int64_t n, const float* motion_times, void* stream) {
    if (!e || !motion_times || n < 0 || n > e->n) { set_error("v2p_env_reset: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    if (!env_ids || n == e->n) e->sched.build_latched = 0;  // an epoch boundary: the next launch may choose its build anew (kernel_build 0)
    if (e->buf.context_feat) e->context_built = 1;
    return launch_env_reset(e, env_ids, env_ids ? n : e->n, motion_times, (hipStream_t)stream);
}

int v2p_env_context(v2p_env* e, const int64_t* env_ids, int64_t n, const float* motion_times, void* stream) {
    if (!e || !motion_times || n < 0 || n > e->n) { set_error("v2p_env_context: bad argument"); return V2P_ERR_INVALID; }
    if (!e->buf.context_feat) { set_error("v2p_env_context: the env was created without a context buffer"); return V2P_ERR_INVALID; }
    e->context_built = 1;
    DeviceGuard g(e->device);
    return launch_env_context(e, env_ids, env_ids ? n : e->n, motion_times, (hipStream_t)stream);
}

int v2p_env_set_context_transform(v2p_env* e, const v2p_context_transform* t, float* draws) {
    // the transform first: its refusals do not need a batch (or a GPU)
    if (!t) { set_error("v2p_env_set_context_transform: null transform"); return V2P_ERR_INVALID; }
    if (t->num_ops < 0 || t->num_ops > 3) { set_error("v2p_env_set_context_transform: num_ops %d not in [0, 3]", t->num_ops); return V2P_ERR_INVALID; }
    bool seen[4] = {false, false, false, false};
    for (int k = 0; k < t->num_ops; ++k) {
        const int op = t->ops[k];
        if (op < V2P_CTX_MASK_JOINTS || op > V2P_CTX_MASK_RANDOM_JOINTS) {
            set_error("v2p_env_set_context_transform: unknown op %d", op);
            return V2P_ERR_INVALID;
        }
        if (seen[op]) { set_error("v2p_env_set_context_transform: op %d repeated", op); return V2P_ERR_INVALID; }
        seen[op] = true;
    }
    if (t->mask_joints >> V2P_NUM_BODIES) { set_error("v2p_env_set_context_transform: mask_joints names bodies above 23"); return V2P_ERR_INVALID; }
    const bool noisy = seen[V2P_CTX_NOISY_JOINTS], drop = seen[V2P_CTX_MASK_RANDOM_JOINTS];
    if (noisy && !(t->noise_prob >= 0.f && t->noise_prob <= 1.f)) {
        set_error("v2p_env_set_context_transform: noisy_joints prob %g not in [0, 1]", (double)t->noise_prob);
        return V2P_ERR_INVALID;
    }
    if (noisy && !(t->conf_std > 0.f)) { set_error("v2p_env_set_context_transform: conf_std %g <= 0", (double)t->conf_std); return V2P_ERR_INVALID; }
    if (drop && !(t->drop_prob >= 0.f && t->drop_prob <= 1.f)) {
        set_error("v2p_env_set_context_transform: mask_random_joints prob %g not in [0, 1]", (double)t->drop_prob);
        return V2P_ERR_INVALID;
    }
    if ((noisy || drop) && !draws) { set_error("v2p_env_set_context_transform: a random op needs the draws buffer"); return V2P_ERR_INVALID; }
    if (!e) { set_error("v2p_env_set_context_transform: null env"); return V2P_ERR_INVALID; }
    if (!e->buf.context_feat) { set_error("v2p_env_set_context_transform: the env was created without a context buffer"); return V2P_ERR_INVALID; }
    if (e->context_built) { set_error("v2p_env_set_context_transform: must be called before the first reset / context call"); return V2P_ERR_INVALID; }
    CtxTransform& x = e->ctx;
    x.ctx_dim = V2P_CONTEXT_DIM_CONF;
    x.num_ops = t->num_ops;
    for (int k = 0; k < 3; ++k) x.ops[k] = k < t->num_ops ? t->ops[k] : 0;
    x.mask_joints = t->mask_joints;
    x.noise_prob = t->noise_prob;
    x.noise_std = t->noise_std;
    x.conf_div = noisy ? (float)(1.7320508075688772 * (double)t->conf_std) : 1.f;  // np.sqrt(3) * conf_std (:578)
    x.min_conf = t->min_conf;
    x.drop_prob = t->drop_prob;
    x.draws = (noisy || drop) ? draws : nullptr;
    return V2P_OK;
}

int v2p_env_pre_physics(v2p_env* e, float* actions, void* stream) {
    if (!e || !actions) { set_error("v2p_env_pre_physics: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    return launch_env_pre(e, actions, (hipStream_t)stream);
}

int v2p_env_physics(v2p_env* e, void* stream) {
    if (!e) { set_error("v2p_env_physics: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    if (e->schedule != 0) { int rc = ensure_env_per_lane_buffers(e); if (rc != V2P_OK) return rc; }
    return env_physics_launch(e, (hipStream_t)stream, nullptr);
}

int v2p_env_export(v2p_env* e, void* stream) {
    if (!e) { set_error("v2p_env_export: bad argument"); return V2P_ERR_INVALID; }
    if (e->schedule == 0) return V2P_OK;  // the link-per-lane kernel writes the exposed tensors itself
    DeviceGuard g(e->device);
    return launch_env_export(e, (hipStream_t)stream);
}

int v2p_env_post_physics(v2p_env* e, void* stream) {
    if (!e) { set_error("v2p_env_post_physics: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    return launch_env_post(e, (hipStream_t)stream);
}

int v2p_env_step(v2p_env* e, float* actions, void* stream) {
    if (e && actions && e->schedule == 0) {
        // link-per-lane schedule: pre-physics runs in the physics kernel's prologue (lane = link owns its joint's action components)
        DeviceGuard g(e->device);
        // ... and post-physics in the epilogue of every env's last job, where the kernel instantiation has it (else its own kernel)
        int fused = 0;
        int rc = env_physics_launch(e, (hipStream_t)stream, actions, &fused);
        if (rc == V2P_OK && fused) e->cur_target = 1 - e->cur_target;
        else if (rc == V2P_OK) rc = launch_env_post(e, (hipStream_t)stream);
        return rc;
    }
    int rc = v2p_env_pre_physics(e, actions, stream);
    if (rc == V2P_OK) rc = v2p_env_physics(e, stream);
    if (rc == V2P_OK) rc = v2p_env_export(e, stream);
    if (rc == V2P_OK) rc = v2p_env_post_physics(e, stream);
    return rc;
}

int v2p_env_push_state(v2p_env* e, const int64_t* env_ids, int64_t n, int with_rb_state, void* stream) {
    if (!e || n < 0 || n > e->n) { set_error("v2p_env_push_state: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    return launch_env_push_state(e, env_ids, env_ids ? n : e->n, with_rb_state, (hipStream_t)stream);
}

int v2p_env_push_state_flagged(v2p_env* e, const int64_t* flags, int /*with_rb_state*/, void* stream) {
    if (!e || !flags) { set_error("v2p_env_push_state_flagged: null batch / flags"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    return launch_env_push_state_flagged(e, flags, (hipStream_t)stream);
}

int v2p_env_set_schedule(v2p_env* e, int schedule) {
    if (!e || (schedule != 0 && schedule != 1)) { set_error("v2p_env_set_schedule: bad argument"); return V2P_ERR_INVALID; }
    if (schedule == 1 && e->num_shapes > 1) { set_error("v2p_env_set_schedule: the env-per-lane kernel handles single-shape batches only"); return V2P_ERR_UNSUPPORTED; }
    if (schedule == 1 && e->p.solver_type == 1) { set_error("v2p_env_set_schedule: the env-per-lane cross-check kernel solves PGS only"); return V2P_ERR_UNSUPPORTED; }
    if (schedule == 1 && e->p.friction_frame == 1) { set_error("v2p_env_set_schedule: the env-per-lane cross-check kernel solves in the world friction frame only"); return V2P_ERR_UNSUPPORTED; }
    if (schedule == 1 && e->p.joint_limits) { set_error("v2p_env_set_schedule: the env-per-lane cross-check kernel has no joint limits"); return V2P_ERR_UNSUPPORTED; }
    if (schedule == 1) {
        DeviceGuard g(e->device);
        int rc = ensure_env_per_lane_buffers(e);
        if (rc != V2P_OK) return rc;
    }
    e->schedule = schedule;
    return V2P_OK;
}

int v2p_env_target_index(const v2p_env* e) { return e ? e->cur_target : V2P_ERR_INVALID; }

int v2p_env_debug_contacts(v2p_env* e, int32_t* out, void* stream) {
    if (!e || !out) { set_error("v2p_env_debug_contacts: bad argument"); return V2P_ERR_INVALID; }
    if (!e->contact_ids) { set_error("v2p_env_debug_contacts: the batch was created with v2p_sim_cfg.debug_contacts = 0"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    return check_hip(hipMemcpyAsync(out, e->contact_ids, sizeof(int32_t) * NB * 4 * (size_t)e->n, hipMemcpyDeviceToDevice, (hipStream_t)stream),
                     "hipMemcpyAsync(contact_ids)");
}

int v2p_env_debug_contacts_substeps(v2p_env* e, int32_t* out, void* stream) {
    if (!e || !out) { set_error("v2p_env_debug_contacts_substeps: bad argument"); return V2P_ERR_INVALID; }
    if (!e->contact_ids_sub) { set_error("v2p_env_debug_contacts_substeps: the batch was created with v2p_sim_cfg.debug_contacts < 2"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    return check_hip(hipMemcpyAsync(out, e->contact_ids_sub, sizeof(int32_t) * NB * 4 * (size_t)e->n * (size_t)e->p.nsub, hipMemcpyDeviceToDevice, (hipStream_t)stream),
                     "hipMemcpyAsync(contact_ids_sub)");
}

int v2p_env_debug_pairing(v2p_env* e, int32_t* perm, int32_t* key, void* stream) {
    if (!e || !perm || !key) { set_error("v2p_env_debug_pairing: bad argument"); return V2P_ERR_INVALID; }
    DeviceGuard g(e->device);
    int rc = V2P_OK;
    if (env_pairing_on(e) && e->sched.pair_have) rc = launch_env_pairing(e, (hipStream_t)stream);
    if (rc == V2P_OK) rc = check_hip(hipMemcpyAsync(perm, e->sched.perm, sizeof(int32_t) * (size_t)e->n, hipMemcpyDeviceToDevice, (hipStream_t)stream), "hipMemcpyAsync(perm)");
    if (rc == V2P_OK) rc = check_hip(hipMemcpyAsync(key, e->sched.pair_key, sizeof(int32_t) * (size_t)e->n, hipMemcpyDeviceToDevice, (hipStream_t)stream), "hipMemcpyAsync(pair_key)");
    return rc;
}

}  // extern "C"
