/*
 * v2p_rollout.h -- C ABI of the MI355X-native rollout engine for vid2player3d's
 * embodied_pose SMPL-humanoid imitation task.
 *
 * This is the drop-in boundary.  The reference's task object
 * (embodied_pose/env/tasks/humanoid_smpl_im.py) talks to Isaac Gym through ~25 gym.* calls;
 * the entry points below are what a reference-side binding would call instead.  Each entry
 * point names the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, no torch types.  Every `float*`/`int64_t*` is a DEVICE pointer owned by the
 *     caller (PyTorch-ROCm tensors on the Python side); the library never frees them.
 *   - row-major, fp32 data, int64 flags/indices (reference buffer dtypes, base_task.py:62-74),
 *     quaternions xyzw.
 *   - every call returns 0 on success or a negative v2p_status; v2p_last_error() returns a
 *     thread-local message.  The Python shim turns non-zero codes into RuntimeError (the
 *     reference's error convention is Python exceptions).
 *   - calls are asynchronous on the hipStream_t passed as `void* stream` (NULL = default
 *     stream); a handle is single-threaded; handles on different GPUs are independent.
 *   - B = 24 bodies, D = 69 dofs, A = 75 actions, OBS = 461.
 */
#ifndef V2P_ROLLOUT_H
#define V2P_ROLLOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V2P_NUM_BODIES 24
#define V2P_NUM_DOF 69
#define V2P_NUM_ACTIONS 75
#define V2P_NUM_OBS 461
#define V2P_MOTION_STATE_DIM 331  /* root_pos3 root_rot4 dof_pos69 root_vel3 root_ang_vel3 dof_vel69 key_pos12 rb_pos72 rb_rot96 */
#define V2P_CONTEXT_DIM 378       /* body_pos72 body_rot96 dof_pos69 body_pos_gt72 dof_pos_gt69 (humanoid_smpl_im.py:202) */
#define V2P_CONTEXT_DIM_CONF 402  /* ... + joint_conf24: the frame of a batch with a context transform (humanoid_smpl_im.py:202-205) */
#define V2P_ABI_VERSION 15

typedef enum {
    V2P_OK = 0,
    V2P_ERR_INVALID = -1,     /* bad argument */
    V2P_ERR_UNSUPPORTED = -2, /* valid in the reference, not built yet (e.g. anisotropic joint gains) */
    V2P_ERR_HIP = -3,         /* HIP runtime error */
    V2P_ERR_NOMEM = -4,
    V2P_ERR_INTERNAL = -5     /* the engine noticed that a launch did not do all it should have (v2p_env_check: skipped substep jobs),
                               * or that its own device memory was written outside an array (v2p_env_check under v2p_debug_guards) */
} v2p_status;

typedef struct v2p_model v2p_model; /* body model (host copy + device constants) */
typedef struct v2p_mlib v2p_mlib;   /* reference-motion tables (device pointers, not owned) */
typedef struct v2p_env v2p_env;     /* a batch of environments on one GPU */

/* ---- body model -------------------------------------------------------------------------
 * Replaces gym.load_asset / create_actor / get+set_actor_dof_properties /
 * get_actor_rigid_body_properties (humanoid_smpl_im.py:273-287, 356-389): the caller hands
 * over the compiled model (HOST pointers; copied). */
typedef struct {
    int32_t num_bodies;          /* must be 24 */
    const int32_t* parents;      /* [B]   -1 for the root */
    const float* local_pos;      /* [B,3] joint offset in the parent frame */
    const float* mass;           /* [B] */
    const float* com;            /* [B,3] body frame */
    const float* inertia;        /* [B,9] about COM, body axes */
    const float* kp;             /* [D] already scaled by body mass (humanoid_smpl_im.py:376-385) */
    const float* kd;             /* [D] */
    const float* armature;       /* [D] */
    const int32_t* hull_offsets; /* [B+1] */
    const float* hull_verts;     /* [V,3] body frame */
    /* ---- ABI 7 */
    const float* limit_lower;    /* [D] nullable: per-DOF range of the exponential-map coordinate, radians (the MJCF `range` that */
    const float* limit_upper;    /* [D] nullable   gym.get_actor_dof_properties reports, humanoid_smpl.py:318-337); NULL = unlimited */
} v2p_model_desc;

int v2p_model_create(const v2p_model_desc* desc, int device, v2p_model** out);
void v2p_model_destroy(v2p_model* m);

/* ---- reference-motion tables ------------------------------------------------------------
 * Replaces the tensor attributes of utils/motion_lib.py:MotionLib (motion_lib.py:78-99,
 * 370-384).  DEVICE pointers, borrowed for the lifetime of the handle. */
typedef struct {
    int64_t num_motions;
    int64_t num_frames_total;
    const float* gts;               /* [F,24,3] global translations */
    const float* grs;               /* [F,24,4] global rotations */
    const float* lrs;               /* [F,24,4] local rotations */
    const float* grvs;              /* [F,3]  root linear velocity */
    const float* gravs;             /* [F,3]  root angular velocity */
    const float* dvs;               /* [F,69] dof velocities */
    const float* motion_lengths;    /* [C] seconds */
    const int64_t* motion_num_frames; /* [C] */
    const float* motion_dt;         /* [C] */
    const float* motion_min_verts_h; /* [C] */
    const int64_t* length_starts;   /* [C] first row of each clip */
    const float* motion_bodies;     /* [C,11] gender + 10 betas */
    int32_t key_body_ids[4];        /* amass_im.yaml:17 -> R_Ankle, L_Ankle, L_Hand, R_Hand */
} v2p_motion_tables;

int v2p_mlib_create(const v2p_motion_tables* tables, int device, v2p_mlib** out);
void v2p_mlib_destroy(v2p_mlib* m);

/* MotionLib.get_motion_state(..., return_rigid_body=True) (motion_lib.py:164-266).
 * `out` points to 9 device arrays in the order root_pos[Q,3] root_rot[Q,4] dof_pos[Q,69]
 * root_vel[Q,3] root_ang_vel[Q,3] dof_vel[Q,69] key_pos[Q,4,3] rb_pos[Q,24,3] rb_rot[Q,24,4];
 * NULL entries are skipped. */
int v2p_motion_state(const v2p_mlib* m, const int64_t* motion_ids, const float* motion_times, int64_t num_queries,
                     int adjust_height, float ground_tolerance, float* const out[9], void* stream);

/* ---- stand-alone task ops (op-level parity tests; also usable by an unmodified task) -----
 * compute_humanoid_reward (humanoid_smpl_im.py:918-953); specs = k_dof,k_vel,k_pos,k_rot,
 * w_dof,w_vel,w_pos,w_rot. */
int v2p_reward(int64_t n, const float* body_pos, const float* body_rot, const float* tgt_pos, const float* tgt_rot,
               const float* dof_pos, const float* dof_vel, const float* tgt_dof_pos, const float* tgt_dof_vel,
               const float* body_pos_weights /*[24]*/, const float specs[8], float* reward /*[n]*/, float* sub_rewards /*[n,4]*/,
               void* stream);
/* compute_humanoid_reset (humanoid_smpl_im.py:956-987); contact bodies are excluded through
 * `term_heights_masked` = termination heights with -inf at the contact bodies. */
int v2p_reset_flags(int64_t n, const int64_t* progress, const float* rb_pos, const float* term_heights_masked /*[24]*/,
                    const float* cur_time, const float* clip_len, float max_episode_length, int enable_early_termination,
                    int64_t* reset_out, int64_t* terminated_out, void* stream);
/* compute_humanoid_observations_imitation, the 734-d in-network observation
 * (humanoid_smpl_im.py:773-850 == models/im_network_builder.py:262-338), local_root_obs =
 * root_height_obs = True. */
int v2p_obs_imitation(int64_t n, const float* body_pos, const float* body_rot, const float* tgt_pos, const float* tgt_rot,
                      const float* dof_pos, const float* dof_vel, const float* tgt_dof_pos, const float* body_vel,
                      const float* body_ang_vel, const float* motion_bodies /*[n,11]*/,
                      const float* norm_mean /*[734] nullable*/, const float* norm_std /*[734] nullable*/, float norm_clip,
                      float* obs /*[n,734]*/, void* stream);
/* ... with RunningNorm.forward in eval mode fused when norm_mean/norm_std are given: clamp((x-mean)/(std+1e-8), +-clip)
 * (models/running_norm.py:32-43). */

/* The same features straight from what the policy network is handed (models/im_network_builder.py:150-189, preprocess_input +
 * compute_humanoid_obs): `obs` rows [rows,461] as the task packs them (humanoid_smpl_im.py:198) and the context frames
 * [envs,ctx_frames,378] (humanoid_smpl_im.py:202, body_pos | body_rot | dof_pos | ...).  rows = envs * steps; row env*steps + k is
 * paired with context frame first_frame + k: rollout (eval) = steps 1, first_frame = context_padding + t; training minibatches
 * (flatten=True) = steps T, first_frame = context_padding.  No split / view / cat of the inputs is materialised. */
int v2p_obs_imitation_packed(int64_t rows, int64_t steps, const float* obs /*[rows,461]*/, const float* context_feat /*[rows/steps,ctx_frames,378]*/,
                             int64_t ctx_frames, int64_t first_frame, const float* norm_mean /*nullable*/, const float* norm_std /*nullable*/,
                             float norm_clip, float* out /*[rows,734]*/, void* stream);

/* Policy head of the rollout (ABI 9): what the reference does between the actor MLP and the env step.
 *   models/im_network_builder.py:219-228 (eval_actor, residual_action = True): mu[:, :69] += cur_context['dof_pos'] - the target DOF
 *     positions of context frame `frame` (= context_padding + t in the rollout), read straight from context_feat [n,ctx_frames,378];
 *   models/im_models.py:45-48: action = Normal(mu, sigma).sample() = mu + sigma * noise, neglogp (rl_games ModelA2CContinuousLogStd):
 *     0.5 sum(((a - mu) / sigma)^2) + 0.5 log(2 pi) * 75 + sum(logstd), sigma = exp(logstd) (fixed_sigma, cfg/amass_im.yaml:76-81).
 * mu [n,75]: the actor MLP's output on entry, the residual mean on exit; noise [n,75] standard normal (the caller's generator);
 * action [n,75], sigma [n,75] (nullable), neglogp [n] are written. */
int v2p_policy_head(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t frame, const float* logstd /*[75]*/,
                    const float* noise, float* action, float* sigma, float* neglogp, void* stream);

/* v2p_policy_head with the experience buffer's rows as additional destinations (the rollout: ExperienceBuffer.update_data of actions / mus /
 * sigmas / neglogpacs, im_agent.py:348-352, without the four copy kernels): sigma_row [n,75] and neglogp_row [n] are written in place of
 * `sigma` / `neglogp`, action_row / mu_row [n,75] (nullable) receive copies of `action` / the residual mean.  `action` stays a tensor of
 * its own - env.step masks the rows of finished envs in place, the buffer keeps the sampled actions. */
int v2p_policy_head_record(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t frame, const float* logstd,
                           const float* noise, float* action, float* sigma_row, float* neglogp_row, float* action_row, float* mu_row, void* stream);

/* The three calls above with the width of a context frame given (ctx_dim floats, >= V2P_CONTEXT_DIM): the frames of a batch with a
 * context transform are V2P_CONTEXT_DIM_CONF wide (v2p_env_set_context_transform).  Only the first V2P_CONTEXT_DIM floats of a frame are
 * read - the network reads body_pos / body_rot / dof_pos of the context, never joint_conf.  The calls without `_w` are these with
 * ctx_dim = V2P_CONTEXT_DIM. */
int v2p_obs_imitation_packed_w(int64_t rows, int64_t steps, const float* obs, const float* context_feat /*[rows/steps,ctx_frames,ctx_dim]*/,
                               int64_t ctx_frames, int64_t ctx_dim, int64_t first_frame, const float* norm_mean, const float* norm_std,
                               float norm_clip, float* out, void* stream);
int v2p_policy_head_w(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t ctx_dim, int64_t frame, const float* logstd,
                      const float* noise, float* action, float* sigma, float* neglogp, void* stream);
int v2p_policy_head_record_w(int64_t n, float* mu, const float* context_feat, int64_t ctx_frames, int64_t ctx_dim, int64_t frame,
                             const float* logstd, const float* noise, float* action, float* sigma_row, float* neglogp_row, float* action_row,
                             float* mu_row, void* stream);

/* The critic's output of a rollout step into the experience buffer (im_agent.py:292-303, 355, 398): value_raw [n] (the network's output) is
 * un-normalised with the value normaliser (running_mean / running_var: DEVICE float64 scalars of rl_games' RunningMeanStd; both NULL = no
 * normaliser) - sqrt(var + epsilon) * clamp(x, -5, 5) + mean - and written to values_row [n] (nullable) and, times (1 - terminated [n]), to
 * next_values_row [n] (nullable): one launch instead of ~9 elementwise kernels and two copies. */
int v2p_value_record(int64_t n, const float* value_raw, const double* running_mean, const double* running_var, float epsilon,
                     const float* terminated, float* values_row, float* next_values_row, void* stream);

/* Bookkeeping of one rollout step after env.step (ImitatorAgent.play_steps, agents/im_agent.py:380-409) in one launch: rewards / dones /
 * next_obses rows of the experience buffer, dones / terminate as floats, running episode returns and lengths, and the episode statistics
 * the reference collects through .nonzero() on the host - here float64 device accumulators:
 *   acc[0] += #episodes finished at this step, acc[1] += their returns, acc[2] += their lengths, acc[3] += #envs not done before the
 *   step, acc[4] += their rewards; sub_acc[k] += their sub-rewards k.  prev_dones / cur_rewards / cur_lengths [n] are updated in place.
 * obs [n,obs_dim] -> next_obs_row (nullable: no copy); rew [n], reset / terminate [n] int64, sub_rewards [n,4]; all DEVICE pointers. */
int v2p_rollout_record(int64_t n, const float* obs, int64_t obs_dim, const float* rew, const int64_t* reset, const int64_t* terminate,
                       const float* sub_rewards, float* next_obs_row, float* rewards_row, float* dones_row, float* dones, float* terminated,
                       float* prev_dones, float* cur_rewards, float* cur_lengths, double* acc /*[>=5]*/, double* sub_acc /*[4]*/, void* stream);

/* GAE reverse scan of the PPO rollout, CommonAgent.discount_values (learning/common_agent.py:423-435):
 * fdones [T,N], values / rewards / next_values / advs [T,N,1] (device). */
int v2p_gae(int64_t horizon, int64_t n, const float* fdones, const float* values, const float* rewards, const float* next_values,
            float gamma, float tau, float* advs, void* stream);

/* ---- reference-motion tables from clips ----------------------------------------------------
 * What the reference computes offline per clip with poselib (uhc/utils/convert_amass_isaac.py:134-153: SkeletonState.from_rotation_and_
 * root_translation -> SkeletonMotion.from_skeleton_state, poselib/poselib/skeleton/skeleton3d.py:409-431 forward kinematics, :1226-1249
 * finite-difference + Gaussian velocities) and MotionLib flattens (embodied_pose/utils/motion_lib.py:370-384, 443-458 dof velocities),
 * for all frames of all clips in two launches.  DEVICE pointers: local_rot [F,24,4] xyzw and root_trans [F,3] (float64, the clips
 * concatenated), frame_clip [F], clip_start [C] (= length_starts), clip_frames [C], clip_dt [C], local_pos [24,3] - or [C,24,3] with
 * per_clip_skeleton (every clip of the reference carries its own SMPL shape).  parents [24]: HOST array.  Out (float32, the layout of
 * v2p_motion_tables): gts [F,24,3] grs [F,24,4] lrs [F,24,4] grvs [F,3] gravs [F,3] dvs [F,69]. */
int v2p_motion_tables_build(int64_t num_frames_total, int64_t num_clips, const double* local_rot, const double* root_trans,
                            const int32_t* frame_clip, const int64_t* clip_start, const int32_t* clip_frames, const double* clip_dt,
                            const int32_t* parents, const double* local_pos, int32_t per_clip_skeleton, float* gts, float* grs, float* lrs,
                            float* grvs, float* gravs, float* dvs, void* stream);

/* ---- per-clip body assets ---------------------------------------------------------------
 * The geometry half of the reference's per-clip asset build (humanoid_smpl_im.py:255-296 -> uhc/smpllib/smpl_local_robot.py:79-143
 * `get_joint_geometries`: ConvexHull of every body's vertex cloud -> decimated mesh; Isaac Gym then integrates the mass properties at
 * the geom density), for thousands of (shape, body) JOBS in one launch, one wavefront per job, float64:
 *   cloud -> convex hull -> at most max_verts (<= 64) support vertices (the Fibonacci-direction tables `dirs`, tried in order until
 *   the distinct support points fit) -> hull of those -> mass, centre of mass, inertia about it.
 * All pointers are DEVICE pointers.  points [total,3]; job_offsets [num_jobs+1] (first point of every job); max_points = the
 * largest cloud (sizes the LDS arrays: ~48 B per point x 2; up to ~1600 points); dirs [.,3] + dir_offsets [num_dir_tables+1].
 * Out per job: mass, com [3], inertia [9], num_verts, vert_ids [max_verts] (indices into the job's cloud, ascending), verts
 * [max_verts,3], status (0 ok, 1 fewer than 4 points, 2 coplanar cloud, 3 face capacity, 4 reduction failed,
 * 7 the job's point count - job_off[j + 1] - job_off[j] - is negative or exceeds max_points).
 * vid2player3d_amd/body_shapes.py holds the host-side wrapper and the numpy statement of the same algorithm (the checker). */
int v2p_shapes_compile(int32_t num_jobs, const double* points, const int32_t* job_offsets, int32_t max_points, const double* dirs,
                       const int32_t* dir_offsets, int32_t num_dir_tables, double density, int32_t max_verts, double eps_rel, double* mass,
                       double* com, double* inertia, int32_t* num_verts, int32_t* vert_ids, double* verts, int32_t* status, void* stream);

/* ---- environments -----------------------------------------------------------------------
 * Simulation + task parameters (cfg/amass_im.yaml:3-52, utils/config.py:190-222). */
typedef struct {
    float sim_dt;               /* 1/60 (config.py:20) */
    int32_t substeps;           /* 2   (amass_im.yaml:38) */
    int32_t control_freq_inv;   /* 2   (amass_im.yaml:11)  -> control dt = 1/30, 4 physics substeps of 1/120 */
    int32_t num_solver_iterations; /* 4 (num_position_iterations) */
    int32_t enable_contact;     /* 0 = BASELINE config 2 (PD only) */
    int32_t residual_hold_sims; /* simulate() calls during which the residual wrench acts: 1 (first_sim) .. control_freq_inv (all) */
    float gravity_z;            /* -9.81 */
    float friction;             /* 1.0 */
    float contact_offset;       /* 0.02 */
    float max_depenetration_velocity; /* 10 */
    float erp;                  /* 0.2 */
    float angular_damping;      /* 0.01 (humanoid_smpl_im.py:274) */
    float max_angular_velocity; /* 100  (humanoid_smpl_im.py:275) */
    float pd_tar_lim;           /* 0.5*pi (humanoid_smpl_im.py:73) */
    float residual_force_scale; /* 31.85 */
    float residual_torque_scale;
    float ground_tolerance;     /* 0 */
    float max_episode_length;   /* 300 */
    int32_t enable_early_termination;
    int32_t context_length;     /* 32 */
    int32_t context_padding;    /* 8 */
    float term_heights[24];     /* per body; contact bodies get -inf (humanoid_smpl_im.py:217-224, 956-987) */
    float body_pos_weights[24]; /* humanoid_smpl_im.py:109-115 */
    float reward_specs[8];      /* k_dof,k_vel,k_pos,k_rot,w_dof,w_vel,w_pos,w_rot (humanoid_smpl_im.py:682) */
    int32_t freeze_terminated_envs; /* 0 (reference behaviour): envs whose reset flag is set keep being simulated as ragdolls until the
                                     * epoch reset, although nothing downstream reads them (zero reward, masked by `dones` in
                                     * im_agent.py:392-414).  1: their physics state is frozen instead (link-per-lane schedule). */
    /* ---- ABI 3 */
    int32_t schedule;           /* kernel schedule a batch starts with (v2p_env_set_schedule changes it): 0 = one link per lane (default),
                                 * 1 = one env per lane (cross-check) */
    int32_t pair_envs_by_load;  /* 1 (default): envs are handed to waves in descending order of their contact load; 0: in index order.
                                 * Results do not depend on it (tests), only the launch duration does. */
    int32_t solver_type;        /* contact solver: 0 = projected Gauss-Seidel (default), 1 = temporal Gauss-Seidel with frozen Jacobians
                                 * (sim.physx.solver_type of amass_im.yaml:41 is 1 = TGS in PhysX; see oracle/phys/v2p_phys_oracle.c for
                                 * what either means here).  Link-per-lane schedule only. */
    int32_t substep_jobs;       /* 1 (when the env pairs do not fit the GPU's wave slots in one round: > CUs x 8 pairs) or 2 (always): the
                                 * physics launch of the link-per-lane schedule is cut into (substep, env pair) jobs that hand the
                                 * state over through memory - 4x finer load balancing of the launch; results are bit-identical to 0
                                 * (one workgroup per env pair runs all substeps).  Every solver / contact setting of the link-per-lane schedule. */
    int32_t job_mono_permille;  /* substep_jobs: share of the env pairs (the heaviest) whose substeps stay in one workgroup; -1 = default (60; 250 above
                                 * 12288 envs, with joint limits or with a ball attached) */
    int32_t pair_mix_permille;  /* pair_envs_by_load: share of the envs (the heaviest) that share their wave with one of the lightest envs
                                 * instead of with an equally heavy one (a wave costs the union of its two envs' contact structure, and the
                                 * heaviest envs are the critical path of the launch); 0 = pairs of equals only; -1 = default (150, 500 with the register build - kernel_build; 0 above 12288 envs,
                                 * with joint limits or with a ball: measured) */
    int32_t debug_contacts;     /* diagnostics, off (0) by default: 1 = keep the contact vertex ids of the last substep
                                 * (v2p_env_debug_contacts; 384 B of extra stores per env-step), 2 = of EVERY substep as well
                                 * (v2p_env_debug_contacts_substeps) */
    /* ---- ABI 7 */
    int32_t joint_limits;       /* 1: every DOF whose range (v2p_model_desc.limit_lower/upper) is narrower than a full turn carries a
                                 * limit row in the contact solver (the racket arm of the player MJCFs; the amass MJCF has none).
                                 * Link-per-lane schedule, contacts on, either solver (under TGS the distance to the limit advances slice by
                                 * slice with the joint rate).  0 (default): ranges are ignored. */
    /* ---- ABI 9 */
    float limit_margin;         /* radians; <= 0 = default (0.05).  A limit row exists in a substep only while its DOF is within reach of the
                                 * limit: C < limit_margin + h * max(0, rate of approach after the unconstrained update v*), C = distance to
                                 * the nearer limit - the speculative activation every other row of the model has (contact_offset for hull
                                 * vertices, the closing distance of a substep for the ball), PhysX's `contactDistance` of a joint limit.
                                 * A joint far from its limits costs nothing; one that is pushed across by an impulse of the same substep
                                 * is caught in the next (C < 0 is always active) and corrected with erp.  1e9 = rows always on (ABI 8). */
    /* ---- ABI 11: the rest of the reference's sim.physx block (cfg/amass_im.yaml:39-48, utils/config.py:190-222) reaches the engine
     * instead of being parsed and dropped on the Python side */
    float rest_offset;          /* 0.0 (amass_im.yaml:45): distance at which a hull vertex rests on the plane - the gap of a hull-vertex row
                                 * is z - rest_offset (PhysX: contacts exist below contact_offset and come to rest at rest_offset) */
    float bounce_threshold_velocity; /* 0.2 (amass_im.yaml:46): approach speed below which a contact does not bounce.  The humanoid's
                                 * contacts have restitution 0 (plane.restitution 0.0), so nothing bounces at any speed; the ball rows take
                                 * their own copy (v2p_ball_cfg.bounce_threshold_velocity).  Must be >= 0. */
    int32_t num_velocity_iterations; /* 0 (amass_im.yaml:43).  The engine's solvers have no separate velocity pass: any other value is
                                 * REFUSED (V2P_ERR_UNSUPPORTED) rather than ignored. */
    /* ---- ABI 12 */
    int32_t kernel_build;       /* the library holds two builds of the link-per-lane physics kernel (same source, same results to float32
                                 * rounding): 1 = three waves per SIMD with the contact records parked in LDS (fastest where the launch is
                                 * bound by instruction issue: BASELINE's 8192 envs), 2 = two waves per SIMD with everything in registers
                                 * (5 - 7 % faster where a launch is as long as its heaviest env pair: small batches).  0 = the engine
                                 * chooses by the number of envs RESIDENT on the device - the sum over the live batches of this
                                 * process, so that rollout groups sharing a GPU are judged together (2 at <= 5120 envs: measured,
                                 * profiles/r04e_dual_build.txt).  The choice is taken at the first launch after v2p_env_create and
                                 * after every whole-batch v2p_env_reset (an epoch boundary) and holds in between: a batch does not
                                 * change build mid-epoch because another batch was created or destroyed.  v2p_env_kernel_build tells
                                 * which one the next launch of a batch runs (read-only). */
    /* ---- ABI 13: the A/B and test switches of the substep jobs (environment variables until ABI 12).  A zero-initialised block = the
     * engine's defaults.  The library reads NO engine option from the environment; its profiling switches (V2P_WAVE_TIMES,
     * V2P_PHASE_TIMING, V2P_PHASE_HEAVY, V2P_ENVS_PER_BLOCK) are honoured only in a process that sets V2P_DEBUG=1. */
    int32_t job_timeout_spins;  /* substep_jobs: polls (with back-off) a job waits for its predecessor before it recomputes the earlier
                                 * substeps itself; 0 = default (50000, ~20 ms), < 0 = give up at once (tests of the recovery path) */
    int32_t job_len;            /* substeps per job; 0 = the engine decides (1, or 2 for launches of >= CUs x 32 env pairs) */
    int32_t job_lead;           /* substeps of the FIRST job of a cut pair; 0 = the engine decides, < 0 = like the other jobs */
    int32_t job_no_interleave;  /* 1: the jobs of a pair are not interleaved with those of other pairs in dispatch order (A/B) */
    /* ---- ABI 14 */
    int32_t friction_frame;     /* tangent directions of the hull x ground rows.  0 (default) = world: t1 = x, t2 = y, each clamped to mu x the
                                 * normal impulse on its own - the friction limit is a box aligned with the world axes (a body pushed along the
                                 * diagonal holds up to sqrt(2) mu).  1 = velocity: t1 along the tangential velocity the contact point has under
                                 * the unconstrained velocity of the substep (where it would slide without contact impulses), t2 = n x t1; world
                                 * frame below 1e-6 m/s - the limit along the direction of sliding is mu whatever that direction is.  The
                                 * reference hands mu = 1 to PhysX (humanoid_smpl.py:175-182, amass_im.yaml:32-35), whose friction directions
                                 * follow the relative velocity at the contact; which of the two agrees with an Isaac Gym trace is for
                                 * tools/replay_trace.py --friction-frame to show.  Link-per-lane schedule (both solvers, ball, joint limits). */
} v2p_sim_cfg;

/* Caller-owned DEVICE buffers the engine reads/writes; these are the tensors the reference
 * task exposes (humanoid_smpl.py:66-113, base_task.py:62-74, humanoid_smpl_im.py:594-636). */
typedef struct {
    float* root_states;    /* [N,13] pos3 quat4 linvel3 angvel3 */
    float* dof_state;      /* [N,69,2] (pos, vel) interleaved like gym's dof state tensor */
    float* rb_state;       /* [N,24,13] */
    float* contact_force;  /* [N,24,3] net contact force per body */
    float* dof_force;      /* [N,69] */
    float* pd_target;      /* [N,69] clamped PD targets of the last step */
    float* obs;            /* [N,461] */
    float* rew;            /* [N] */
    float* sub_rewards;    /* [N,4] */
    int64_t* reset;        /* [N] */
    int64_t* terminate;    /* [N] */
    int64_t* progress;     /* [N] */
    float* cur_time;       /* [N] _cur_ref_motion_times */
    float* reset_time;     /* [N] _reset_ref_motion_times */
    float* target[2];      /* 2 x [N,331]: current / previous target motion state, flipped every step */
    float* context_feat;   /* [N,48,378] (nullable) */
    uint8_t* context_mask; /* [N,48]     (nullable) */
} v2p_env_buffers;

/* Replaces create_sim/add_ground/create_env/create_actor/prepare_sim/acquire_*_tensor
 * (humanoid_smpl.py:66-134, humanoid_smpl_im.py:231-389).  env_motion_id [N] is a DEVICE
 * array (each env is bound to one clip, humanoid_smpl_im.py:247-254). */
int v2p_env_create(const v2p_model* model, const v2p_mlib* mlib, const v2p_sim_cfg* cfg, const int64_t* env_motion_id,
                   int64_t num_envs, const v2p_env_buffers* buffers, int device, v2p_env** out);
/* The same with one body SHAPE per env: the reference builds one humanoid asset per sampled clip from its SMPL betas and
 * scale (humanoid_smpl_im.py:255-296, _create_smpl_humanoid_xml) and gives env i the asset of its clip.  `shapes` are
 * models with identical body trees, `env_shape_id` [N] is a HOST array of indices into `shapes` (copied). */
int v2p_env_create_shapes(const v2p_model* const* shapes, int32_t num_shapes, const int32_t* env_shape_id, const v2p_mlib* mlib,
                          const v2p_sim_cfg* cfg, const int64_t* env_motion_id, int64_t num_envs, const v2p_env_buffers* buffers,
                          int device, v2p_env** out);
void v2p_env_destroy(v2p_env* e);

/* HumanoidSMPL.reset(env_ids) with reference-state init (humanoid_smpl.py:136-173,
 * humanoid_smpl_im.py:442-563).  env_ids NULL = all envs.  motion_times [n] (device) are the
 * RSI phases; the caller draws them (MotionLib.sample_time, motion_lib.py:138-159) so that
 * the RNG stays on the Python side.  Fills state, target, obs, context. */
int v2p_env_reset(v2p_env* e, const int64_t* env_ids, int64_t n, const float* motion_times, void* stream);
/* HumanoidSMPLIM._init_context(motion_ids, motion_times) on its own (humanoid_smpl_im.py:530-563): the context window of the given envs
 * rebuilt around motion_times [n] (device) - frames motion_times + dt + dt * (-padding .. length + padding - 1) of each env's own clip -
 * into context_feat / context_mask, nothing else touched.  The reference's player calls it every context_length steps with the
 * current clip times (players/im_player.py:238-240): an evaluation rollout runs past the 32-step window without a reset.
 * V2P_ERR_INVALID when the env was created without a context buffer. */
int v2p_env_context(v2p_env* e, const int64_t* env_ids, int64_t n, const float* motion_times, void* stream);

/* Context transform (cfg env.transform_specs; HumanoidSMPLIM._transform_target, humanoid_smpl_im.py:565-592): the policy's context
 * window is corrupted the way a pose estimated from video is - joints dropped, joints noised - and carries a joint_conf channel.
 * The ops run in the yaml's key order, on each (env, frame, body) of the window, AFTER the clean sample and before anything is stored:
 *   V2P_CTX_MASK_JOINTS   (:569-573)  the ORIGINAL ones tensor is zeroed at the bodies of `mask_joints` (bit b = body b) and
 *                                     body_pos *= it.  After noisy_joints, the reported confidence is another tensor and stays.
 *   V2P_CTX_NOISY_JOINTS  (:574-586)  noised = u_noise < noise_prob (root included); body_pos += z * (noised ? noise_std : 0);
 *                                     conf = 2 (1 - Phi(|noise| / (sqrt(3) conf_std))) for EVERY body (un-noised: exactly 1);
 *                                     conf < min_conf: conf = 0, body_pos = 0.
 *   V2P_CTX_MASK_RANDOM_JOINTS (:587-591)  dropped = u_drop < drop_prob, never the root: conf = 0, body_pos = 0.
 * Only body_pos [0,72) and joint_conf [378,402) of a frame change: body_rot, dof_pos, the _gt blocks and context_mask are the clean
 * window's.  The draws stay on the caller's side (the reference draws with torch.bernoulli / torch.randn_like): `draws` [N,W,24,5]
 * (device, W = context_length + 2 context_padding) holds per (env id, frame, body) u_noise, z.xyz, u_drop, and is read by every
 * v2p_env_reset / v2p_env_context for the envs it touches - the caller refills it before each such call.  A Bernoulli(p) is u < p. */
enum { V2P_CTX_MASK_JOINTS = 1, V2P_CTX_NOISY_JOINTS = 2, V2P_CTX_MASK_RANDOM_JOINTS = 3 };
typedef struct {
    int32_t num_ops;       /* 0..3 (0: no corruption, the joint_conf column is all ones: `transform_specs: {}`) */
    int32_t ops[3];        /* V2P_CTX_* in the order they run; each at most once */
    uint32_t mask_joints;  /* mask_joints.joints: bit b = body b (24 bits) */
    float noise_prob;      /* noisy_joints.prob, in [0,1] */
    float noise_std;       /* noisy_joints.noise_std */
    float conf_std;        /* noisy_joints.conf_std, > 0 */
    float min_conf;        /* noisy_joints.min_conf */
    float drop_prob;       /* mask_random_joints.prob, in [0,1] */
} v2p_context_transform;
/* Attaches the transform to the batch and switches it to V2P_CONTEXT_DIM_CONF-float frames (the caller's context_feat must be
 * [N,W,402]); must be called before the first v2p_env_reset / v2p_env_context.  Refused (V2P_ERR_INVALID, nothing changed): unknown
 * or repeated ops, bits above body 23, probabilities outside [0,1], conf_std <= 0, draws NULL when noisy_joints or
 * mask_random_joints is present, a batch without a context buffer, or one that has already built a window.  The transform is
 * checked before the batch, so a NULL `e` reports what is wrong with `t` first. */
int v2p_env_set_context_transform(v2p_env* e, const v2p_context_transform* t, float* draws /*[N,W,24,5] device, nullable*/);

/* BaseTask.step(actions) (base_task.py:147-165) = pre_physics_step + _physics_step +
 * post_physics_step.  actions [N,75] is masked IN PLACE for envs whose reset flag is set
 * (humanoid_smpl_im.py:126). */
int v2p_env_step(v2p_env* e, float* actions, void* stream);
/* The stages separately (trace replay / profiling). */
int v2p_env_pre_physics(v2p_env* e, float* actions, void* stream);   /* humanoid_smpl_im.py:125-157 */
int v2p_env_physics(v2p_env* e, void* stream);                        /* base_task.py:450-454: the 2 x gym.simulate */
int v2p_env_export(v2p_env* e, void* stream);                         /* the 6 gym.refresh_*_tensor calls, humanoid_smpl_im.py:452-468 */
int v2p_env_post_physics(v2p_env* e, void* stream);                   /* humanoid_smpl_im.py:398-418 */

/* set_actor_root_state_tensor_indexed + set_dof_state_tensor_indexed (+ rigid-body state for
 * teacher-forced replay): pushes the caller-edited root_states/dof_state (and rb_state when
 * `with_rb_state`) buffers into the engine's internal structure-of-arrays state. */
int v2p_env_push_state(v2p_env* e, const int64_t* env_ids, int64_t n, int with_rb_state, void* stream);
/* v2p_env_push_state for every env of the batch whose flags[env] is not 0 (device, [N]; only read), indexed by env: no id list.  The
 * engine's state of every other env keeps every bit.  Refused before any HIP call (V2P_ERR_INVALID): a null batch or null flags. */
int v2p_env_push_state_flagged(v2p_env* e, const int64_t* flags /*[N]*/, int with_rb_state, void* stream);

/* Two schedules of the same physics model are built: 0 = one LINK per lane (default: 32 lanes per env, state in
 * registers, level-synchronous tree recursions), 1 = one ENV per lane (LDS-resident workspace).  They agree to float32
 * rounding; the second one is kept as an independent cross-check (tests) and for A/B profiling. */
int v2p_env_set_schedule(v2p_env* e, int schedule);

/* index (0/1) of the CURRENT target inside v2p_env_buffers.target; the other one is the previous target */
int v2p_env_target_index(const v2p_env* e);

/* which build of the link-per-lane kernel the batch runs (v2p_sim_cfg.kernel_build): 1 = LDS-parked / 3 waves per SIMD, 2 = registers / 2 */
int v2p_env_kernel_build(const v2p_env* e);

/* diagnostics for tests: contact vertex ids chosen in the last substep, [N,24,4] int32, body*64+vertex or -1
 * (needs v2p_sim_cfg.debug_contacts >= 1) */
int v2p_env_debug_contacts(v2p_env* e, int32_t* out, void* stream);

/* the same for every substep of the last control step, [N,substeps*control_freq_inv,24,4] (needs v2p_sim_cfg.debug_contacts == 2) */
int v2p_env_debug_contacts_substeps(v2p_env* e, int32_t* out, void* stream);

/* diagnostics for tests: the wave-slot -> env order the NEXT physics launch will look up (`perm`, [N] int32, written out here from the
 * tables the last launch left; envs are handed to waves in descending order of their contact load, see DESIGN.md "pairing") and the
 * load key it is built from (`key`, [N]) */
int v2p_env_debug_pairing(v2p_env* e, int32_t* perm, int32_t* key, void* stream);

/* ---- racket + ball (vid2player/env/tasks/humanoid_smpl_im_mvae.py:367-442 actors, :711-783 physics step; data/assets/
 * smpl_mesh_humanoid_djokovic.xml:188-190, tennis_ball.urdf).  The racket is welded to a link: its mass belongs to that link of the
 * body model handed to v2p_model_create (vid2player3d_amd/racket.py builds it), its two solid cylinders are given here in the link's
 * frame for the ball contacts.  The ball is a free sphere simulated alongside the humanoid (same substeps): gravity, the reference's
 * drag + Magnus force re-evaluated before every simulate() call (apply_external_force_to_ball), ball x ground and ball x racket
 * contacts with restitution and friction (material values combined by averaging, PhysX's default), and - body_contacts - the ball
 * against the convex hulls of the humanoid's links (the ball actor collides with every shape of its env, :367-372, 432): one point per
 * substep, against the nearest hull; the racket's link is left to its cylinders.  Link-per-lane schedule, contacts on, either solver
 * (TGS: the two-body rows' gaps advance slice by slice; a row's restitution target is taken once, at the start of the substep).
 * The reference's flag bookkeeping around simulate() (bounce test on the ball height at the start of every call, :731-737; racket-hit
 * poll after it, :773-779) runs inside the step when the flag buffers are given. */
typedef struct {
    float radius, mass, inertia;                     /* 0.032, 0.057, 4e-5 */
    float restitution_ground, friction_ground;       /* 0.5, 0.9 */
    float restitution_racket, friction_racket;       /* 1.0, 0.8 */
    float bounce_threshold_velocity;                 /* 0.2 (sim.physx) */
    float angular_damping, max_angular_velocity;     /* gymapi.AssetOptions defaults: 0.5, 64 */
    float spin_scale;                                /* cfg_v2p spin_scale, 1.0 */
    int32_t racket_link;                             /* 22 = R_Wrist */
    int32_t num_cylinders;                           /* <= 2 */
    float cylinders[2][8];                           /* centre 3, unit axis 3, half length, radius; racket_link's frame */
    float racket_offset[3];                          /* origin of the racket rigid body (index 24 of the reference's tensor) in that frame */
    float restitution_body, friction_body;           /* ball x a link's hull: 0.5, 0.9 */
    int32_t body_contacts;                           /* 1: ball x hull contacts on */
    float bounce_height;                             /* ball height at the start of a simulate() call at or below which the ball "has bounced" (:733) */
    int32_t poll_racket_hits;                        /* 1: the racket-hit flags are kept (the reference does so when sim.substeps <= 2, :769) */
} v2p_ball_cfg;
typedef struct {                  /* caller-owned DEVICE buffers */
    float* ball_state;            /* [N,13] the ball actor's root state (pos quat linvel angvel): read at the start of every step, written at
                                   * its end - edit it in place to launch a ball (set_actor_root_state_tensor_indexed) */
    float* racket_state;          /* [N,13] rigid-body state of the racket */
    float* ball_per_sim;          /* [N,control_freq_inv,13] ball state after each simulate() call (what refresh_actor_root_state_tensor shows) */
    int32_t* racket_hit_per_sim;  /* [N,control_freq_inv] racket-ball contact force non-zero after the call (the reference's poll, :773-779) */
    float* ball_contact;          /* [N,2,3] contact force on the ball from the racket / from the ground after the last call */
    float* ball_body_contact;     /* [N,3] nullable: contact force on the ball from the humanoid's links after the last call */
    /* the reference's flags, all five or none (nullable): sticky `has_*` (cleared by the caller when it relaunches a ball), `*_now` = set by
     * this step; bounce_pos = ball position at the start of the call that saw the bounce */
    uint8_t* has_bounce;          /* [N] */
    uint8_t* has_bounce_now;      /* [N] */
    float* bounce_pos;            /* [N,3] */
    uint8_t* has_racket_contact;      /* [N] */
    uint8_t* has_racket_contact_now;  /* [N] */
    /* ---- ABI 9 */
    float* contact_force_sum;     /* [N,24,3] nullable: `_contact_forces_sum` (humanoid_smpl_im_mvae.py:186, 690, 781) - the net contact force of
                                   * every link (the racket's link carries the reaction of the ball) after each simulate() call, summed over the
                                   * calls of the control step; overwritten by every step */
} v2p_ball_buffers;
int v2p_env_attach_ball(v2p_env* e, const v2p_ball_cfg* cfg, const v2p_ball_buffers* buffers);
/* Per-shape rackets (ABI 14): in a batch of several body shapes (v2p_env_create_shapes) every shape may hold its racket on a link of its
 * own - the reference's two-player batches (cfg_v2p dual_mode `different`: env 2k player 0, env 2k+1 player 1, one left-handed) weld it
 * to L_Wrist (17) for one player and R_Wrist (22) for the other.  An env's racket link, cylinders and racket rigid body are then its
 * shape's: the ball x racket rows, the ball x hull rows (which skip the racket's link), the racket-hit flags, the racket's reaction in
 * the link's net contact force and the exported racket state all follow it.  v2p_env_attach_ball gives every shape the cfg's racket
 * (again, when it is called again); this call, made after it, replaces them: `num_shapes` must equal the batch's shape count.
 * Refused (V2P_ERR_INVALID, nothing changed): a count that differs, racket_link outside 1..23, num_cylinders outside 0..2, a batch
 * without a ball. */
typedef struct {
    int32_t racket_link;        /* the link the racket is welded to: 22 = R_Wrist, 17 = L_Wrist */
    int32_t num_cylinders;      /* <= 2 */
    float cylinders[2][8];      /* centre 3, unit axis 3, half length, radius; racket_link's frame (as v2p_ball_cfg) */
    float racket_offset[3];     /* origin of the racket rigid body in that frame */
} v2p_racket_geom;
int v2p_env_set_racket_shapes(v2p_env* e, const v2p_racket_geom* per_shape, int32_t num_shapes);

/* ---- free balls on their own (vid2player/utils/tennis_ball.py:113-218 `simulate`, tennis_ball_out_estimator.py:21-121
 * `simulate_without_bounce`): n balls, one per lane, each simulated alone for num_frames control steps of control_freq_inv simulate()
 * calls of `substeps` substeps, in one launch.  The ball is the engine's own (the ball of v2p_env_attach_ball without racket and
 * humanoid: gravity, drag + Magnus force re-evaluated before every call, the ball x ground rows under either solver, angular damping
 * and cap), so that the pool of incoming launches and the estimator tables the reference makes offline with Isaac Gym describe the
 * ball a racket + ball batch really simulates.  Added to `simulate`'s side of it: the SIGN of the launch spin (the spin fed to the
 * lift is sign x |w| / 2 pi until the call that detects the bounce, + afterwards, :163-176, 190-195; launch angular velocity =
 * vspin x 2 pi x normalize(launch_vel x (0,0,-1)), :135-136), and the bookkeeping at the start of every call (:167-187).
 * No handle, no state between calls; asynchronous on `stream` on the CURRENT device. */
typedef struct {
    float radius, mass, inertia;                     /* 0.032, 0.057, 4e-5 (tennis_ball.urdf) */
    float restitution_ground, friction_ground;       /* ball x plane, already combined */
    float bounce_threshold_velocity;
    float angular_damping, max_angular_velocity;     /* 0.5, 64 */
    float spin_scale;
    float sim_dt;                                    /* length of one simulate() call */
    int32_t substeps, control_freq_inv, num_iterations, solver_type; /* all >= 1; solver_type 0 PGS, 1 TGS */
    float gravity_z, contact_offset, erp, max_depenetration_velocity;
    int32_t enable_ground;                           /* 0: no ground rows (the outgoing tables) */
    int32_t num_frames;                              /* control steps recorded */
    float net_height;                                /* pass_net: height the ball must exceed at the first call that sees y < 0 */
    float bounce_height;                             /* height at the start of a call at or below which the ball "has bounced" */
    int32_t resample;                                /* 1: no trajectory; the positions at the start of all (num_frames + 1) x control_freq_inv
                                                      * calls are resampled online onto the two grids below (needs enable_ground = 0) */
    double grid_x[3];                                /* (lo, hi, step) of the horizontal distance y: int((hi - lo) / step) cells, cell k at lo + k step */
    double grid_y[3];                                /* (lo, hi, step) of the drop below the launch height */
} v2p_ball_sim;
typedef struct {                 /* DEVICE buffers, each nullable */
    float* traj;                 /* [n,num_frames,3] position at the start of control step t (resample = 0) */
    float* bounce_pos;           /* [n,3] position at the start of the call that saw z <= bounce_height first, else 0 */
    int64_t* bounce_idx;         /* [n] frame of that call, else num_frames - 1 */
    uint8_t* pass_net;           /* [n] at the first call that saw y < 0: not yet bounced and z > net_height */
    float* peak_after_bounce;    /* [n] largest recorded height over frames bounce_idx .. num_frames - 1 (resample = 0) */
    float* final_state;          /* [n,13] pos quat vel angvel after the last call */
    float* traj_x;               /* [n,nx] resample: height relative to the launch height at every distance of grid_x */
    float* traj_y;               /* [n,ny,2] resample: (distance, time in seconds) at every drop of grid_y */
} v2p_ball_rollout_out;
/* Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): NULL cfg / out; NULL launch arrays with n > 0; n < 0;
 * substeps, control_freq_inv, num_iterations or num_frames < 1; solver_type outside 0 / 1; mass, inertia or radius <= 0; resample
 * with enable_ground, without both grids (a grid with no cell), or with a non-positive step.  n = 0 is a no-op. */
int v2p_ball_rollout(const v2p_ball_sim* cfg, int64_t n, const float* launch_pos /*[n,3]*/, const float* launch_vel /*[n,3]*/,
                     const float* launch_vspin /*[n] revolutions per second, signed*/, const v2p_ball_rollout_out* out, void* stream);

/* ---- the tennis controller's task step (vid2player/env/tasks/physics_mvae_controller.py: PhysicsMVAEController) on top of a racket +
 * ball batch: everything the controller does after the physics of a control step - racket hit, true and estimated bounce bookkeeping
 * (_update_state, :271-314), one of the three reward laws (:368-406, 492-602), the actor + task observation (:316-360), the reaction /
 * recovery / termination flags (_compute_reset, :408-436) and the roll of the ball-trajectory window (physics_step, :365-366) - for all
 * envs in ONE launch without a host synchronisation (the reference has two: has_contact_now.sum() > 0, has_valid_contact.sum() > 0).
 * One wavefront per env: lanes stride the columns of the observation row.  Stateless like v2p_reward: every buffer is the caller's. */
enum { V2P_TENNIS_REWARD_REACH = 0, V2P_TENNIS_REWARD_RETURN = 1, V2P_TENNIS_REWARD_RETURN_W_ESTIMATE = 2 };
#define V2P_TENNIS_ACTOR_OBS 225   /* root_pos3 root_vel3 (bodies 1..24 - root)72 rot6d(bodies 0..23)144 racket_normal3 (:333-342) */
#define V2P_TENNIS_TRAJ_FRAMES 100 /* frames of an env's ball trajectory (`_ball_traj`, :64) */
typedef struct {
    int32_t reward_type;            /* V2P_TENNIS_REWARD_* (cfg_v2p reward_type) */
    int32_t obs_ball_traj_length;   /* L, 1..100: the task observation holds 3 L columns */
    int32_t use_history_ball_obs;   /* 1: the window is the rolled history of ball positions, 0: frames cursor .. cursor + L - 1 of ball_traj */
    int32_t use_random_ball_target; /* 1: two more columns, target xy - root xy */
    int32_t contact_by_velocity;    /* 1 (sim.substeps > 2): the racket hit is read from the ball's velocity change
                                     * (humanoid_smpl_im_mvae.py:800-808) and WRITTEN to has_racket_contact(_now); 0: the flags are read */
    int32_t enable_early_termination;
    int64_t max_episode_length;     /* episodeLength */
    float grip_normal[3];           /* racket normal in the wrist frame: eastern (0,1,0), semi_western (0,1/sqrt2,1/sqrt2) (:835-838) */
    float court_min[2], court_max[2]; /* cfg_v2p court_min / court_max: the player leaves the court outside them (:482-490) */
    float scale_pos, scale_phase, scale_bounce_pos, scale_bounce_time; /* reward_scales: 5, 10, 0.05, 0.1 */
    float weight_pos, weight_ball_pos; /* reward_weights `pos` (default 1 for reach, 0 else) and `ball_pos` (0) */
    /* the out-estimator (utils/tennis_ball_out_estimator.py:13-18, 124-205): grids as (lo, hi, step) in the order VEL_X, VEL_Y, VSPIN,
     * TRAJ_X, TRAJ_Y, and the shape of the two tables */
    double grid[5][3];
    int64_t table_rows;             /* B */
    int32_t table_nx, table_ny;     /* cells of a row of traj_out_x / traj_out_y */
} v2p_tennis_cfg;
typedef struct {                    /* DEVICE buffers; bool tensors are bytes */
    /* read only: the racket + ball batch's tensors */
    const float* rb_state;          /* [N,24,13] */
    const float* root_states;       /* [N,13] */
    const float* racket_state;      /* [N,13] rigid body 24 */
    const float* ball_state;        /* [N,13] */
    const int64_t* wrist_link;      /* [N] the link the env's racket is welded to */
    const uint8_t* has_bounce;      /* [N] */
    const uint8_t* has_bounce_now;  /* [N] */
    const float* bounce_pos;        /* [N,3] */
    /* read only: what the motion generator supplies */
    const float* phase_pred;        /* [N] */
    const int64_t* swing_type;      /* [N] (reach, return) */
    const int64_t* swing_type_cycle; /* [N] (return_w_estimate) */
    /* read only: the outgoing tables */
    const float* traj_out_x;        /* [B,nx] */
    const float* traj_out_y;        /* [B,ny,2] */
    /* read only: the controller's targets */
    const int64_t* tar_time_total;  /* [N] */
    const int64_t* tar_action;      /* [N] 1 swing, 0 recovery */
    const float* target_bounce_pos; /* [N,3] */
    const float* ball_traj;         /* [N,100,3] (nullable with use_history_ball_obs) */
    /* read and written */
    uint8_t* has_racket_contact;    /* [N] written with contact_by_velocity only */
    uint8_t* has_racket_contact_now; /* [N] */
    int64_t* tar_time;              /* [N] */
    int64_t* progress;              /* [N] */
    float* prev_ball_vy;            /* [N] the ball's vy at the previous task step (`_ball_vel[:, 1]` before its update) */
    int32_t* traj_cursor;           /* [N] first frame of the env's window inside ball_traj; frames past 100 read as zero */
    float* ball_obs;                /* [N,L,3] history of ball positions, rolled by every observation (nullable without use_history_ball_obs) */
    uint8_t* bounce_in;             /* [N] */
    float* est_bounce_pos;          /* [N,3] */
    float* est_bounce_time;         /* [N] */
    float* est_max_height;          /* [N] */
    uint8_t* est_bounce_in;         /* [N] */
    float* distance;                /* [N] */
    int64_t* vel_x_overflow;        /* [1] 'velocity X overflow' counter (tennis_ball_out_estimator.py:180) */
    /* written */
    float* racket_pos;              /* [N,3] */
    float* racket_normal;           /* [N,3] */
    float* obs;                     /* [N, 225 + 3 L (+ 2)] */
    float* rew;                     /* [N] */
    float* sub_rewards;             /* [N,1] reach, [N,2] else */
    int64_t* reset;                 /* [N] */
    int64_t* terminate;             /* [N] */
    uint8_t* reset_reaction;        /* [N] */
    uint8_t* reset_recovery;        /* [N] */
} v2p_tennis_buffers;
/* One control step of the task for envs 0 .. n-1, in the reference's order: tar_time / progress += 1; racket hit; _update_state; reward;
 * observation; _compute_reset; the window advances one frame.  sub_rewards_names (HOST, nullable) receives the reward law's names string.
 * Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): n < 0, a null required pointer, L outside 1..100, an
 * unknown reward type, tables without cells.  n = 0 is a no-op. */
int v2p_tennis_task_step(const v2p_tennis_cfg* cfg, int64_t n, const v2p_tennis_buffers* buffers, const char** sub_rewards_names, void* stream);
/* `_compute_observations(env_ids)` alone (:198-199, at reset time), the history roll of those envs included: racket_pos, racket_normal,
 * ball_obs and obs rows of env_ids [n_ids] (device; ids outside 0 .. num_envs-1 are skipped) are written, nothing else. */
int v2p_tennis_task_obs(const v2p_tennis_cfg* cfg, int64_t num_envs, const v2p_tennis_buffers* buffers, const int64_t* env_ids, int64_t n_ids,
                        void* stream);

/* ---- the controller's evaluation step (vid2player/env/tasks/mvae_controller_vis.py: MVAEControllerVis, what `run.py --test` runs):
 * v2p_tennis_task_step with the test-mode episode law (`_compute_reset`, :64-79) in place of the training law, the four per-env meters
 * of `_compute_stats` (:81-95, AverageMeterUnSync of utils/common.py:34-63) and one frame of the record the evaluation hands on
 * (:140-146) - in the same ONE launch, without a host read (the reference: a nonzero(), up to eight .cpu() copies for the meters, six
 * more and a growing torch.cat for the record).  v2p_tennis_cfg / v2p_tennis_buffers are the step's, unchanged; of the cfg
 * max_episode_length, enable_early_termination, court_min and court_max are not read, of the buffers `distance` is neither read nor
 * written.
 *   terminate = reset = progress > episode_length (after the increment); in_time = tar_time >= tar_time_total
 *   reaction = (hit & tar_action == 0 & has_bounce & in_time) | (~hit & in_time)
 *   recovery = tar_action == 1 & (hit | ball_y < root_y - 1 | |ball_vy| < 2);   where reset: reaction = 1, recovery = 0
 * A NaN in the observation row, a root outside the court end nothing.  An env whose recovery flag is up updates its meters with hit,
 * swing_type_cycle == 1, est_bounce_in and - only where est_bounce_in - ||est_bounce_pos - target_bounce_pos||, est_* being this
 * step's: sum += v, count += 1, avg = sum / float(count), max = v > max ? v : max.  An env owns its meters: no atomics, one order. */
enum { V2P_TENNIS_METER_HIT_RATE = 0, V2P_TENNIS_METER_FH_RATIO = 1, V2P_TENNIS_METER_BOUNCE_IN_RATE = 2, V2P_TENNIS_METER_BOUNCE_IN_POS_ERROR = 3 };
#define V2P_TENNIS_METERS 4
typedef struct {
    int64_t episode_length;         /* cfg env.episodeLength (the reference's default: 600); the test is strict */
    int64_t num_frames;             /* F of the record's arrays (not read without a record) */
    int32_t body_of_smpl[24];       /* `_mujoco_2_smpl`: the engine's body of SMPL joint s; [0] = 0, a permutation (not read without a record) */
} v2p_tennis_eval_cfg;
typedef struct {                    /* DEVICE buffers */
    /* the meters, read and written, in the order V2P_TENNIS_METER_*: before the first update avg is 1, sum, count and max are 0 */
    float* meter_sum[V2P_TENNIS_METERS];     /* each [N] */
    int64_t* meter_count[V2P_TENNIS_METERS];
    float* meter_avg[V2P_TENNIS_METERS];
    float* meter_max[V2P_TENNIS_METERS];
    /* the record: all six arrays and dof_state, or none (all NULL: nothing is written).  Frame-major, so that a step's stores are
     * contiguous; the reference's [N, F, ...] is a permuted view */
    const float* dof_state;         /* [N,69,2] read only: the engine's DoF (position, velocity) pairs, body order; the positions are read */
    float* joint_rot;               /* [F,N,24,3] `_joint_rot` of `_update_state_from_sim` with `_is_train` false (humanoid_smpl_im_mvae.py:813-820):
                                     * joint 0 = quaternion_to_angle_axis of the root link's (x,y,z,w) as (w,x,y,z), joints 1..23 = the DoF positions */
    float* root_pos;                /* [F,N,3] */
    float* ball_pos;                /* [F,N,3] */
    float* target_pos;              /* [F,N,3] */
    float* phase;                   /* [F,N] */
    int64_t* swing_type_cycle;      /* [F,N] */
} v2p_tennis_eval_buffers;
/* One evaluation step of envs 0 .. n-1; with a record, frame `frame` (a count the caller keeps on the host) of its arrays is written.
 * Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): n <= 0, a null meter array, null swing_type_cycle, a
 * record with some of its seven pointers null, a frame outside [0, num_frames), body_of_smpl that is no permutation with [0] = 0, and
 * what v2p_tennis_task_step refuses. */
int v2p_tennis_eval_step(const v2p_tennis_cfg* cfg, const v2p_tennis_eval_cfg* eval_cfg, int64_t n, const v2p_tennis_buffers* buffers,
                         const v2p_tennis_eval_buffers* eval_buffers, int64_t frame, const char** sub_rewards_names, void* stream);

/* ---- the two-player rally (vid2player/env/tasks/physics_mvae_controller_dual.py: PhysicsMVAEControllerDual; envs 2k and 2k+1 are
 * opponents, utils/common.py:111-115): the task step with the dual reset law, and the ball hand-over that turns one player's hit into
 * the other's incoming ball (humanoid_smpl_im_mvae_dual.py:65-79 `_reset_balls`, utils/tennis_ball_in_estimator.py:48-79 `estimate`).
 * Both reuse v2p_tennis_cfg / v2p_tennis_buffers; what the hand-over writes of buffers that the step only reads comes again, writable,
 * in v2p_tennis_dual_buffers (the same memory). */
typedef struct {
    float grip_normal[2][3];        /* racket normal in the wrist frame of even / odd envs (the reference's `grip` list,
                                     * humanoid_smpl_im_mvae.py:839-842); v2p_tennis_cfg.grip_normal is not read */
    /* the in-estimator: grids as (lo, hi, step) in the order HEIGHT, VEL_X, VEL_Y, VSPIN (tennis_ball_in_estimator.py:10-14) and the
     * shape of its table [B,F,2] (distance along the launch direction, height) */
    double in_grid[4][3];
    int64_t in_rows;                /* B */
    int32_t in_frames;              /* F, 1..100 */
} v2p_tennis_dual_cfg;
typedef struct {                    /* DEVICE buffers of the hand-over */
    const float* traj_in;           /* [B,F,2] read only */
    const float* target_draw;       /* [N] read only: the caller's uniform draws of the three-way target (use_random_ball_target), else nullable */
    float* ball_state;              /* [N,13] */
    uint8_t* has_bounce;            /* [N] */
    float* bounce_pos;              /* [N,3] */
    int64_t* tar_action;            /* [N] */
    float* target_bounce_pos;       /* [N,3] (use_random_ball_target) */
    float* ball_traj;               /* [N,100,3] (nullable with use_history_ball_obs: the window is then not kept) */
    int64_t* num_reset_reaction;    /* [N] */
} v2p_tennis_dual_buffers;
/* One control step of the task for the n (even) envs of a two-player batch: v2p_tennis_task_step - counters, racket-hit rule,
 * _update_state, reward, observation, window advance - with three differences.  No out-estimator (physics_mvae_controller.py:73, 299):
 * est_* and vel_x_overflow are neither read for a lookup nor written, traj_out_x / _y and cfg->grid are not read; return_w_estimate
 * rewards with what est_* hold.  The racket normal uses dual->grip_normal[env & 1].  The reset law is the dual one (:96-121):
 * reset_recovery = tar_action==1 & (hit | ball_y < root_y-1 | (has_bounce & ball_z < 0.05)); reset_reaction = the opponent's
 * reset_recovery; terminate = (reset_recovery & ~hit) | (tar_action==0 & has_bounce & ~bounce_in), OR-ed over the pair; terminated envs
 * get reset = 1 and both flags 0; reset is otherwise left alone, `terminate`, tar_time_total, court_min / _max, max_episode_length and
 * enable_early_termination are not used.  No host synchronisation (the reference has terminate.sum() > 0).
 * Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): odd n, null dual, and what v2p_tennis_task_step refuses
 * of what is read here. */
int v2p_tennis_dual_step(const v2p_tennis_cfg* cfg, const v2p_tennis_dual_cfg* dual, int64_t n, const v2p_tennis_buffers* buffers,
                         const char** sub_rewards_names, void* stream);
/* The flag-driven half of the dual `_reset_envs` (:42-64, training mode) for all n / 2 pairs in one launch, without an id list, a host
 * synchronisation or an allocation; one wavefront per pair.  For every env whose reset_reaction is set, in the reference's order: the
 * in-estimator on the OPPONENT's ball state; the table row's F frames, transformed and mirrored, become frames 0..F-1 of the env's
 * ball_traj in front of frames F..99 of its current window, traj_cursor = 0; ball_state = ball_states_in, the opponent's =
 * ball_states_out (where both react, out wins, and - the reference sorts its opponent list, utils/common.py:111-115 - each flies the
 * table row of its OWN state); has_bounce, bounce_pos, has_racket_contact cleared, prev_ball_vy = the new vy.  Then
 * _reset_recovery_tasks of envs with reset_recovery (tar_action = 0, has_bounce, bounce_pos cleared), the dual _reset_reaction_tasks
 * (tar_time = 0, tar_action = 1, num_reset_reaction += 1, bounce_in = 0, est_* = 0 with return_w_estimate, the history fill with
 * use_history_ball_obs, target_bounce_pos from target_draw: < 0.33 left, > 0.67 right, else middle) and the observation row of the
 * reacting envs (history roll, racket_pos, racket_normal included).  The flags are read, not cleared.  Envs without a flag in their
 * pair keep every bit.  Refused before any HIP call: odd n, null dual / dual_buffers or a null required pointer, F outside 1..100, a
 * table without rows, a grid that is not (lo < hi, step > 0), use_random_ball_target without target_draw. */
int v2p_tennis_dual_handover(const v2p_tennis_cfg* cfg, const v2p_tennis_dual_cfg* dual, int64_t n, const v2p_tennis_buffers* buffers,
                             const v2p_tennis_dual_buffers* dual_buffers, void* stream);

/* ---- the action part of the controller's pre_physics_step (physics_mvae_controller.py:247-266) with `random_walk_in_recovery`
 * (:252-257) in one launch, without a host synchronisation or an allocation.  A policy action row is 32 latent columns, then
 * num_res_dof residual-DoF columns, then num_res_root residual-root columns; columns behind them are not read.
 * The random numbers are Philox4x32-10 under key (seed) and counter (env, block | stream << 28, call) with the laws of csrc/philox.hpp
 * (numpy: vid2player3d_amd/device_rng.py): env i draws its 32 normals from blocks 0..7 of the WALK stream, normal 4b+2p+q is element q of
 * the Box-Muller pair of words 2p, 2p+1 of block b.  A draw depends on (seed, call, env) alone - the reference deals draw k of a call to
 * the k-th env in recovery instead; both are iid.  The caller counts `call` on the host. */
typedef struct {
    int32_t num_res_dof;            /* columns 32 .. 32+num_res_dof-1 (add_residual_dof: 3), >= 0 */
    int32_t num_res_root;           /* the columns behind them (add_residual_root: 3), >= 0 */
    int32_t random_walk;            /* 0 / 1: random_walk_in_recovery */
    float vae_action_scale, residual_dof_scale, residual_root_scale;
    float clamp;                    /* 5.0: the drawn latent is clamped to [-clamp, clamp]; >= 0 */
    uint64_t seed, call;
} v2p_controller_actions_cfg;
typedef struct {                    /* DEVICE buffers */
    const float* actions;           /* [N, actions_stride] read only */
    int64_t actions_stride;         /* floats from one row to the next, >= 32 + num_res_dof + num_res_root */
    const int64_t* tar_action;      /* [N] read only; required with random_walk: 0 = the env is in recovery */
    const uint32_t* words;          /* [N,32] nullable: stands in for the generator's output words (word 4b+j = word j of block b) */
    float* actions_out;             /* [N, 32+num_res_dof+num_res_root] `_actions`: the copy */
    float* mvae_actions;            /* [N,32] `_mvae_actions`: actions[:, :32] * vae_action_scale; in recovery under random_walk the
                                     * clamped draws */
    float* res_dof_actions;         /* [N,num_res_dof] `_res_dof_actions` (nullable when num_res_dof = 0) */
    float* res_root_actions;        /* [N,num_res_root] `_res_root_actions` (nullable when num_res_root = 0) */
} v2p_controller_actions_buffers;
/* Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): null cfg / buffers, n < 0 or above 2^31-1, a negative
 * column count, a stride below the row's width, a clamp that is negative or NaN, a null required pointer.  n = 0 is a no-op. */
int v2p_controller_actions(const v2p_controller_actions_cfg* cfg, int64_t n, const v2p_controller_actions_buffers* buffers, void* stream);

/* ---- the flag-driven half of the single-player `_reset_envs` (physics_mvae_controller.py:167-242 with `_reset_balls`,
 * humanoid_smpl_im_mvae.py:503-524, and TennisBallGeneratorOffline.generate, utils/tennis_ball.py:422-456) for all n envs in ONE launch,
 * without an id list, a host synchronisation or an allocation; one wavefront per env.  rx = reset_reaction[e], rc = reset_recovery[e],
 * both as they stand at entry; the flags are read, not cleared.  In the reference's order:
 *   rx: the pool row - random rule: integer(word 0, 0, rows), and for a ball with y > 0
 *       clamp(long((x + 4) / 8 * rows) + integer(word 1, -1000, 1000), 0, rows - 1), the float part in float32; round-robin rule:
 *       sample_idx[e], post-incremented modulo rows -; ball_state = (pos, (0,0,0,1), vel, vspin 2 pi normalize(vel x (0,0,-1)));
 *       has_bounce, bounce_pos, has_racket_contact cleared; ball_traj row = the pool row's frames, zeros past them; traj_cursor = 0;
 *       prev_ball_vy = the launch vy
 *   rc: tar_action = 0, has_bounce and bounce_pos cleared
 *   rx: the history fill (use_history_ball_obs), tar_time = 0, tar_action = 1, num_reset_reaction += 1, bounce_in and est_* cleared,
 *       swing_type_cycle = -1, tar_time_total = reset_reaction_nframes + integer(word 2, -5, 5); target_bounce_pos: discrete mode from
 *       u = uniform(word 3): u < 0.33 -> (-3, 10, 0), u > 0.67 -> (3, 10, 0), else (0, 10, 0); continuous mode
 *       uniform(words 4..6) * (target_max - target_min) + target_min, ONE draw for all envs of the call
 *   rx | rc: the observation row of v2p_tennis_task_obs (history roll, racket_pos, racket_normal included)
 * Envs without a flag keep every bit.  The words are block 0 of the RESET stream of csrc/philox.hpp under (seed, call, env), words 4..6
 * those of env 0xffffffff (the whole call); `words` [N,8], when given, stands in for them.  A draw depends on (seed, call, env) alone -
 * the reference draws for the flagged envs in order of env id; both are iid.
 * What the launch writes of buffers that v2p_tennis_buffers declares read-only comes again, writable, in v2p_tennis_reset_buffers (the
 * same memory).  Of v2p_tennis_buffers it reads rb_state, root_states, racket_state, wrist_link, reset_reaction, reset_recovery and
 * writes tar_time, prev_ball_vy, traj_cursor, ball_obs, bounce_in, est_*, racket_pos, racket_normal, obs. */
enum { V2P_TENNIS_TARGET_OFF = 0, V2P_TENNIS_TARGET_DISCRETE = 1, V2P_TENNIS_TARGET_CONTINUOUS = 2 };
enum { V2P_TENNIS_POOL_RANDOM = 0, V2P_TENNIS_POOL_ROUND_ROBIN = 1 };
typedef struct {
    int64_t reset_reaction_nframes; /* cfg_v2p reset_reaction_nframes */
    int32_t target_mode;            /* V2P_TENNIS_TARGET_* (cfg_v2p use_random_ball_target: False / True / 'continuous') */
    int32_t pool_rule;              /* V2P_TENNIS_POOL_* (TennisBallGeneratorOffline.sample_random: True / False) */
    float target_min[3], target_max[3]; /* (-3, 9, 0), (3, 11, 0) (:84-85) */
    int64_t pool_rows;              /* >= 1 */
    int32_t pool_frames;            /* frames of a pool row's trajectory, 1..100 */
    int64_t pool_stride;            /* floats from one pool row to the next, >= 7 + 3 pool_frames */
    uint64_t seed, call;
} v2p_tennis_reset_cfg;
typedef struct {                    /* DEVICE buffers */
    const float* pool;              /* [rows, pool_stride]: launch pos3, vel3, vspin1, then pool_frames x 3 positions; read only */
    int64_t* sample_idx;            /* [N] the round-robin rule's next row per env (nullable under the random rule) */
    float* ball_state;              /* [N,13] */
    uint8_t* has_bounce;            /* [N] */
    float* bounce_pos;              /* [N,3] */
    uint8_t* has_racket_contact;    /* [N] */
    float* ball_traj;               /* [N,100,3] */
    int64_t* tar_time_total;        /* [N] */
    int64_t* tar_action;            /* [N] */
    float* target_bounce_pos;       /* [N,3] (nullable with V2P_TENNIS_TARGET_OFF) */
    int64_t* num_reset_reaction;    /* [N] */
    int64_t* swing_type_cycle;      /* [N] */
    const uint32_t* words;          /* [N,8] nullable: stands in for the generator's output words */
} v2p_tennis_reset_buffers;
/* Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): null cfg / reset cfg / buffers / reset buffers, n < 0
 * or above 2^31-1, L outside 1..100, pool_rows < 1, pool_frames outside 1..100, a stride below 7 + 3 pool_frames, an unknown target
 * mode or pool rule, a null required pointer.  n = 0 is a no-op. */
int v2p_tennis_task_reset(const v2p_tennis_cfg* cfg, const v2p_tennis_reset_cfg* reset_cfg, int64_t n, const v2p_tennis_buffers* buffers,
                          const v2p_tennis_reset_buffers* reset_buffers, void* stream);

/* ---- the MotionVAE motion generator of a control step (vid2player/players/mvae_player.py `MVAEPlayer.step` / `reset` around
 * motion_vae/model.py:186-252 `MixedDecoder.forward`): the gate, the three expert-blended layers and the player's state update
 * (`_update_mvae_state`) in ONE launch, without a host synchronisation or an allocation.  The decoder computes every expert and blends
 * the results, out = sum_e c_e (x W_e + b_e) - the same function as the reference's per-env blended weights - on the fp32-input MFMA,
 * fp32 throughout.  Only the shipped architecture is built: frame 288, latent 32, hidden 256, 6 experts, gate 64, 1 condition frame,
 * 1 prediction, predicted phase; the feature layout is root pos 0:3, root vel 3:6, joint pos 6:75, joint vel 75:144, rot6d 144:288.
 * Stateless like v2p_tennis_task_step: every buffer is the caller's. */
enum { V2P_MVAE_PLAYER_DJOKOVIC = 0, V2P_MVAE_PLAYER_FEDERER = 1, V2P_MVAE_PLAYER_NADAL = 2 };
#define V2P_MVAE_FRAME 288
#define V2P_MVAE_LATENT 32
#define V2P_MVAE_HIDDEN 256
#define V2P_MVAE_EXPERTS 6
#define V2P_MVAE_GATE 64
typedef struct {
    int32_t frame_size, latent_size, hidden_size, num_experts, gate_hidden_size; /* 288, 32, 256, 6, 64: anything else is refused */
    int32_t num_condition_frames, num_future_predictions, predict_phase;         /* 1, 1, 1 */
    int32_t player;            /* V2P_MVAE_PLAYER_*: whose residual-DoF windows and base angles (mvae_player.py:306-408) */
    int32_t righthand;         /* the playing hand: elbow / wrist of the residual, the swing-type numbers, the racket's FK chain */
    int32_t is_train;          /* 0: residuals outside swings are zeroed, and joint_rot is written */
    int32_t add_residual_dof;  /* 1 ('euler'): v2p_mvae_step takes a residual */
} v2p_mvae_cfg;
/* DEVICE pointers.  The matrices are REPACKED (vid2player3d_amd/mvae.py `pack_matrix`): a stack W[E][K][N] (y = x W) becomes
 * [E][ceil(N/32)][K/8][64][4], element q of lane l of column tile t, k-group g being W[e][8g + 2q + (l>>5)][32t + (l&31)] (0 past column
 * N) - what lane l feeds to four consecutive 32x32x2 MFMAs as one 16-byte load; biases are padded with zeros to a multiple of 32
 * columns.  The gate's three Linear layers (torch weight [out,in]) are packed as one-expert stacks of their transposes. */
typedef struct {
    const float *w0, *b0;            /* [6][320][256] packed, [6][256] */
    const float *w1, *b1;            /* [6][288][256] packed, [6][256] */
    const float *w2, *b2;            /* [6][288][290] packed (10 tiles), [6][320] */
    const float *gate_w0, *gate_b0;  /* [1][320][64] packed, [64] */
    const float *gate_w1, *gate_b1;  /* [1][64][64] packed, [64] */
    const float *gate_w2, *gate_b2;  /* [1][64][6] packed (1 tile), [32] */
    const float *avg, *std;          /* [288] */
} v2p_mvae_weights;
typedef struct {                     /* DEVICE buffers: the player's state under the reference's names */
    float* conditions;               /* [N,1,288] normalized */
    float* root_pos;                 /* [N,3] */
    float* root_vel;                 /* [N,3] */
    float* joint_rot6d;              /* [N,24,6] */
    float* joint_rotmat;             /* [N,24,3,3] */
    float* joint_rot;                /* [N,24,3] angle-axis; written when not training (nullable with is_train) */
    float* racket_pos;               /* [N,3] written by reset only */
    float* racket_normal;            /* [N,3] written by reset only */
    float* phase_pred;               /* [N] */
    int64_t* swing_type;             /* [N] */
    int64_t* swing_type_cycle;       /* [N] */
} v2p_mvae_buffers;
/* `MVAEPlayer.step(latents, residual)` for envs 0 .. n-1 (:184-190, 221-223, 254-422 with init=False).  residual [n,3] is nullable (no
 * residual rule then), and refused without add_residual_dof; latents and residual are only read.  Refused before any HIP call
 * (V2P_ERR_INVALID, a message that names the call): a null struct or required pointer, n < 0, another architecture, an unknown player.
 * n = 0 is a no-op. */
int v2p_mvae_step(const v2p_mvae_cfg* cfg, int64_t n, const v2p_mvae_weights* weights, const v2p_mvae_buffers* buffers, const float* latents /*[n,32]*/,
                  const float* residual /*[n,3], nullable*/, void* stream);
/* `MVAEPlayer.reset(env_ids)` (:160-165, 212-252, 424-431 with init=True) for env_ids [n_ids] (device; ids outside 0 .. num_envs-1 are
 * skipped): swing types -1, the condition from init_feature (row i belongs to env_ids[i]), the root position with xy = root_xy (the
 * caller's draw), rot6d -> rotmat (-> joint_rot when not training), racket head position and normal by the 9-joint FK chain of
 * utils/racket.py:183-203, 235-269 over joint_pos_bind_rel with the eastern racket vectors (the player builds its Racket without a
 * grip).  Only avg and std of `weights` are read.  Refusals as v2p_mvae_step. */
int v2p_mvae_reset(const v2p_mvae_cfg* cfg, int64_t num_envs, const v2p_mvae_weights* weights, const v2p_mvae_buffers* buffers, const int64_t* env_ids,
                   int64_t n_ids, const float* init_feature /*[n_ids,288]*/, const float* root_xy /*[n_ids,2]*/, const float* joint_pos_bind_rel /*[24,3]*/,
                   void* stream);
/* Where the start of a reset env comes from when v2p_mvae_reset_flagged is given no root_xy (`draw_root_xy`, mvae_player.py:230-236):
 * V2P_MVAE_ROOT_CENTRE is (0, -13), the branch taken when not training with a test_mode other than `random`; V2P_MVAE_ROOT_DRAW is the
 * kernel's own draw near it, in float32 with every operation rounded on its own: x = (u0 - 0.5) * 2 + 0, y = (u1 - 0.5) * 1.5 + (-13),
 * u = (word >> 8) * 2^-24 of words 0 and 1 of Philox4x32-10 block 0 of stream 2 (csrc/philox.hpp PHILOX_STREAM_ROOT) under
 * (seed, call, env): a draw depends on those three alone, never on which other envs are flagged.  `call` is the host's count of launches. */
enum { V2P_MVAE_ROOT_CENTRE = 0, V2P_MVAE_ROOT_DRAW = 1 };
typedef struct {
    int32_t rule;            /* V2P_MVAE_ROOT_* */
    uint64_t seed, call;
} v2p_mvae_root_rule;
/* v2p_mvae_reset for every env e of 0 .. num_envs-1 whose flags[e] is not 0 (device, [num_envs]; any non-zero value counts), in ONE
 * launch over all envs: no id list, no host read.  init_feature is [num_envs,288] and row e belongs to env e (the player's initial
 * frames read in place, without a gather); root_xy [num_envs,2] is nullable: where given, row e is env e's start, where null the start
 * follows `rule` (required then).  Rows of envs whose flag is 0 keep every bit; the flags are only read.  Equal, bit for bit, to
 * v2p_mvae_reset with env_ids = the flagged envs, ascending, and the gathered rows.  Refusals as v2p_mvae_reset, and: null flags /
 * init_feature / joint_pos_bind_rel, num_envs above 2^31-1, no root_xy and no rule, an unknown rule.  num_envs = 0 is a no-op. */
int v2p_mvae_reset_flagged(const v2p_mvae_cfg* cfg, int64_t num_envs, const v2p_mvae_weights* weights, const v2p_mvae_buffers* buffers, const int64_t* flags /*[N]*/,
                           const float* init_feature /*[N,288]*/, const float* root_xy /*[N,2], nullable*/, const v2p_mvae_root_rule* rule /*nullable with root_xy*/,
                           const float* joint_pos_bind_rel /*[24,3]*/, void* stream);

/* ---- the motion generator of a two-player batch (`MVAEPlayer` with cfg `dual_mode: different`, mvae_player.py:23-57, 167-199): env 2k
 * is side 0 and env 2k+1 side 1; each side has its own decoder weights, normalisation statistics, playing hand and player rule, the
 * state is one set of buffers.  A row's side is its parity: nothing is read back to the host. */
typedef struct {             /* the ONE racket object of the batch (:56-57): the server's hand and grip, walked by every reset env */
    int32_t righthand;       /* which arm the FK chain takes (utils/racket.py:152-161) */
    float dir[3];            /* canonical racket direction in the wrist's frame: (-1, 0, 0) for both grips (utils/racket.py:10-32) */
    float normal[3];         /* canonical racket normal: eastern (0, 1, 0), semi_western (0, 1, 1) normalised as F.normalize does */
} v2p_mvae_racket;
enum { V2P_MVAE_DUAL_MAP_PARITY = 0,   /* workgroup b serves side b & 1 */
       V2P_MVAE_DUAL_MAP_HALVES = 1 }; /* the grid's first half serves side 0, its second half side 1: the mapping the player uses -
                                        * 3.0 % faster at 8192 envs, 1.6 % slower at 1024 (profiles/r27a_mvae_dual_bench.log); both
                                        * stay callable so that the choice can be measured again */
/* `MVAEPlayer.step` under `_is_dual` for envs 0 .. n-1, n even, in ONE launch of 2 ceil(n / 64) workgroups, each of 32 envs of one
 * side.  cfg[2], weights[2]: side 0, side 1 (is_train and add_residual_dof must agree).  Per side: the decoder's weights, avg and std of
 * the unnormalised feature, righthand in the swing-type rule, the player's residual table and the elbow / wrist joints it rewrites.
 * One quirk of the reference is reproduced: the root-position columns 0:3 of EVERY env's condition are normalised with side 1's avg and
 * std (:254-262 writes all envs, and side 1's call runs last).  mapping: V2P_MVAE_DUAL_MAP_*; both give the same numbers, bit for bit.  Refusals as
 * v2p_mvae_step, and: an odd n, cfgs that disagree on is_train or add_residual_dof, an unknown mapping. */
int v2p_mvae_dual_step(const v2p_mvae_cfg* cfg /*[2]*/, int64_t n, const v2p_mvae_weights* weights /*[2]*/, const v2p_mvae_buffers* buffers,
                       const float* latents /*[n,32]*/, const float* residual /*[n,3], nullable*/, int32_t mapping, void* stream);
/* `reset_dual` under `_is_dual` (:167-180, 212-252, 424-431) for env_ids [n_ids] (device): whole pairs (2k, 2k+1), ascending - the
 * reference splits the list by position, which is the env's parity only then; the caller sees to it.  A row is normalised with the
 * statistics of its own side (env & 1), feature and root columns alike.  Every reset env walks `racket`'s arm chain.
 * joint_pos_bind_rel [bind_rows,24,3]: `infer_with_fk` reads joint_pos_bind_rel[:batch] of a side's sub-list, so the pair at list
 * positions 2i, 2i+1 reads row i, NOT the env's own row; bind_rows = 1 is one row for all, otherwise 2 bind_rows >= n_ids is required.
 * Rows outside the list are not touched; ids outside 0 .. num_envs-1 are skipped.  Only avg and std of `weights` are read. */
int v2p_mvae_dual_reset(const v2p_mvae_cfg* cfg /*[2]*/, int64_t num_envs, const v2p_mvae_weights* weights /*[2]*/, const v2p_mvae_buffers* buffers,
                        const v2p_mvae_racket* racket, const int64_t* env_ids, int64_t n_ids, const float* init_feature /*[n_ids,288]*/,
                        const float* root_xy /*[n_ids,2]*/, const float* joint_pos_bind_rel /*[bind_rows,24,3]*/, int64_t bind_rows, void* stream);
/* v2p_mvae_dual_reset for every env e of 0 .. num_envs-1 (even) whose flags[e] is not 0, in ONE launch over all envs: no id list, no
 * host read.  The caller raises both flags of a pair (v2p_ctl_pair_reset_begin does).  init_feature is [num_envs,288] and row e belongs
 * to env e: the caller interleaves the serve and ready frames by parity and serve_from once.  root_xy [num_envs,2] and rule: as
 * v2p_mvae_reset_flagged (the same stream and law under (seed, call, env)).  joint_pos_bind_rel is ONE [24,3] row: the id-list form
 * reads the row of a pair's POSITION in the list, which without a list would need a prefix count of the flagged pairs - bind_rows > 1
 * is refused with V2P_ERR_UNSUPPORTED and a message.  Rows of envs whose flag is 0 keep every bit; the flags are only read.  Equal, bit
 * for bit, to v2p_mvae_dual_reset with env_ids = the flagged envs, ascending, and the gathered rows.  Refusals as v2p_mvae_dual_reset,
 * and: an odd num_envs or one above 2^31-1, null flags / init_feature / joint_pos_bind_rel, no root_xy and no rule, an unknown rule,
 * bind_rows < 1.  num_envs = 0 is a no-op. */
int v2p_mvae_dual_reset_flagged(const v2p_mvae_cfg* cfg /*[2]*/, int64_t num_envs, const v2p_mvae_weights* weights /*[2]*/, const v2p_mvae_buffers* buffers,
                                const v2p_mvae_racket* racket, const int64_t* flags /*[N]*/, const float* init_feature /*[N,288]*/,
                                const float* root_xy /*[N,2], nullable*/, const v2p_mvae_root_rule* rule /*nullable with root_xy*/,
                                const float* joint_pos_bind_rel /*[bind_rows,24,3]*/, int64_t bind_rows, void* stream);

/* ---- the imitation target from the motion generator's pose (vid2player/env/tasks/humanoid_smpl_im_mvae.py): what turns the root
 * position and the 24 local joint matrices that v2p_mvae_step writes into the packed target row [331] (layout of v2p_env_buffers.target)
 * that the low-level policy's humanoid tracks.  Stateless like v2p_mvae_step: every buffer is the caller's, no allocation, no host
 * synchronisation, one launch per call.  The SMPL tree and the order of the engine's bodies come in with the cfg (the task knows them
 * from the body names): joint s of SMPL is the engine's body b with smpl_of_body[b] = s (`_smpl_2_mujoco`, :218-237). */
enum { V2P_PD_BASE_TARGET_POS = 0, V2P_PD_BASE_CURRENT_POS = 1, V2P_PD_BASE_NONE = 2 };
typedef struct {
    float dt;                       /* the control step (> 0): velocities are differences against the previous target over dt */
    int32_t fix_head_orientation;   /* cfg_v2p fix_head_orientation: turn Head and Neck towards the ball (:605-634) */
    int32_t head_body;              /* the engine's body index of Head */
    int32_t smpl_head, smpl_neck;   /* SMPL joints Head (15) and Neck (12) */
    int32_t key_bodies[4];          /* engine body indices whose rb_pos make key_pos */
    int32_t smpl_parents[24];       /* the SMPL tree: [0] = -1, 0 <= parents[s] < s */
    int32_t smpl_of_body[24];       /* a permutation of 0..23 with smpl_of_body[0] = 0 */
    int32_t num_shapes;             /* rows of joint_pos_bind (>= 1) */
    int32_t pd_target_base;         /* V2P_PD_BASE_*: v2p_mvae_target_actions only */
    int32_t no_scale_action;        /* 1: the action is added unscaled (v2p_mvae_target_actions only) */
} v2p_mvae_target_cfg;
typedef struct {                    /* DEVICE buffers */
    const float* root_pos;          /* [N,3] the player's `_root_pos` */
    float* joint_rotmat;            /* [N,24,3,3] the player's `_joint_rotmat`; Head and Neck are WRITTEN by the head rule of the step */
    const float* residual_root;     /* [N,3] nullable: `_res_root_actions`, already scaled (add_residual_root, :602-603) */
    const float* ball_state;        /* [N,13] the ball's root state (position read); required by the head rule */
    const float* joint_pos_bind;    /* [num_shapes,24,3] rest joints of the SMPL bodies, SMPL order */
    const int32_t* env_shape_id;    /* [N] nullable (= shape 0): row of joint_pos_bind of an env */
    float* target;                  /* [N,331] the row that is written */
    const float* prev_target;       /* [N,331] the previous target (root_pos and rb_rot are read); step only; must not alias target */
    float* root_states;             /* [N,13]    step: nullable, unused.  reset: nullable, the ids' rows are written (pose, zero velocities) */
    float* dof_state;               /* [N,69,2]  reset: as root_states.  actions with V2P_PD_BASE_CURRENT_POS: the current dof_pos is read */
    float* rb_state;                /* [N,24,13] step: body 0's position is the simulated root of the head rule's miss test (required by it);
                                     * reset: as root_states */
    int64_t* hold_reset;            /* [N] nullable, step only: zeroed - the wrapped imitation task's own episode bookkeeping (its clip */
    int64_t* hold_progress;         /* [N] nullable      clock against the clip's length, progress against its episode length) must not end */
    float* hold_cur_time;           /* [N] nullable      an episode the controller owns, nor mask its actions */
    const float* pd_action_scale;   /* [69] actions only, unless no_scale_action */
    const float* pd_action_offset;  /* [69] actions only, with V2P_PD_BASE_NONE */
} v2p_mvae_target_buffers;
/* `_set_target_motion_state` (:600-661) for envs 0 .. n-1: the target root = root_pos (+ residual_root); with fix_head_orientation the
 * head rule (:605-634) on a first forward-kinematics pass, Head and Neck written back into joint_rotmat; then `_smpl_to_sim` /
 * `_forward_kinematics` (:897-946, utils/hybrik.py:598-652 batch_rigid_transform): dof_pos = angle-axis of the local matrices, rb_pos /
 * rb_rot by the chain of transforms over the env's row of joint_pos_bind, velocities against prev_target (root_ang_vel divided by dt
 * twice, as the reference has it, :919).  Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): a null struct or
 * required pointer, n < 0, dt <= 0, a body / key-body / joint index outside 0..23, a tree or body order that is none, target ==
 * prev_target.  n = 0 is a no-op. */
int v2p_mvae_target_step(const v2p_mvae_target_cfg* cfg, int64_t n, const v2p_mvae_target_buffers* buffers, void* stream);
/* `_reset_actors` + `_set_env_state` (:463-501) for env_ids [n_ids] (device; ids outside 0 .. num_envs-1 are skipped): `_smpl_to_sim`
 * without a previous pose - no head rule, every velocity zero - into rows env_ids of `target` (the caller names the buffer that holds the
 * PREVIOUS target: the reference stores the init pose as `_prev_target_*`, :492-494) and, where given, of root_states, dof_state and
 * rb_state (v2p_env_push_state with_rb_state = 1 then puts the humanoid there).  Rows of other envs are not touched.  Refusals as the step. */
int v2p_mvae_target_reset(const v2p_mvae_target_cfg* cfg, int64_t num_envs, const v2p_mvae_target_buffers* buffers, const int64_t* env_ids, int64_t n_ids,
                          void* stream);
/* v2p_mvae_target_reset for every env e of 0 .. num_envs-1 whose flags[e] is not 0 (device, [num_envs]; only read), in ONE launch over
 * all envs: the flagged envs' rows of `target` (the buffer the caller names: the previous target) and, where given, of root_states,
 * dof_state and rb_state; every other row keeps every bit.  Equal, bit for bit, to v2p_mvae_target_reset with env_ids = the flagged
 * envs.  Refusals as v2p_mvae_target_reset, and null flags.  num_envs = 0 is a no-op. */
int v2p_mvae_target_reset_flagged(const v2p_mvae_target_cfg* cfg, int64_t num_envs, const v2p_mvae_target_buffers* buffers, const int64_t* flags /*[N]*/,
                                  void* stream);
/* `_action_to_pd_targets` (:693-703) before its clamp, for envs 0 .. n-1: actions_out[:, :69] = base + (no_scale_action ? 1 :
 * pd_action_scale[c]) * actions_in[:, :69], base = target's dof_pos / dof_state's dof_pos / pd_action_offset by pd_target_base; columns
 * 69..74 are copied.  The clamp to dof_pos +- pi/2 (:705-707) is the engine's pre-physics clamp with pd_tar_lim = pi/2.  actions_out may
 * be actions_in.  Refused: as the step, and an unknown pd_target_base. */
int v2p_mvae_target_actions(const v2p_mvae_target_cfg* cfg, int64_t n, const float* actions_in /*[n,75]*/, const v2p_mvae_target_buffers* base_buffers,
                            float* actions_out /*[n,75]*/, void* stream);

/* ---- what stands around the policy networks' dense layers in a control step (vid2player/players/im_player.py:187-199,
 * players/v2p_player.py:113-131, models/im_network_builder.py:53-81, models/im_network_builder_dual.py:37-45): the clamp of the
 * observation, the input normaliser, the split of a two-player batch into one contiguous GEMM operand per network, and on the way back
 * the clamp of the low-level policy's mu and `_action_to_pd_targets`.  The dense layers themselves are the caller's (hipBLASLt).
 * Stateless: every buffer is the caller's, no allocation, no host synchronisation, one launch per call.
 *
 * Side-major order of the network's rows: with sides = 1 env i is row i; with sides = 2 (n even; env i is player i & 1, rows 0::2 go
 * through network1 and rows 1::2 through network2) env i is row (i & 1) * (n / 2) + (i >> 1), so that each network reads and writes one
 * contiguous [n/2, .] block and nothing is gathered or interleaved.
 * Every clamp is torch.clamp's: a NaN stays a NaN, a clip of +inf changes nothing. */
enum { V2P_NORM_NONE = 0, V2P_NORM_RUNNING = 1, V2P_NORM_MEAN_VAR = 2 };
typedef struct {
    int32_t kind;        /* V2P_NORM_NONE:     y = x (models/running_norm.py:35 with n == 0)
                          * V2P_NORM_RUNNING:  y = clamp((x - mean) / (spread + 1e-8), -clip, clip), spread = the std (running_norm.py:31-42, eval)
                          * V2P_NORM_MEAN_VAR: y = clamp((x - mean) / sqrt(spread + eps), -clip, clip), spread = the variance (rl_games'
                          *                    RunningMeanStd in eval mode: eps 1e-5, clip 5, statistics cast to float32) */
    float eps;           /* MEAN_VAR only */
    float clip;          /* > 0 (not read by NONE) */
    const float* mean;   /* [dim] DEVICE (not read by NONE) */
    const float* spread; /* [dim] DEVICE: std or variance by kind (not read by NONE) */
} v2p_policy_norm;
typedef struct {
    int32_t sides;           /* 1 or 2 */
    float clip_obs;          /* the observation is clamped to +-clip_obs first (> 0; +inf: no clamp) */
    v2p_policy_norm norm[2]; /* the normaliser of each side's network; [1] is not read with sides = 1 */
} v2p_policy_input_cfg;
/* x = normaliser(clamp(obs, +-clip_obs)) for envs 0 .. n-1, obs [n,dim] in env order, x [n,dim] in side-major order; dim >= 1.  x must
 * not alias obs with sides = 2.  Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): a null cfg, obs or x, a
 * null mean / spread of a normaliser that reads them, sides outside {1, 2}, an odd n with two sides, n < 0, dim < 1, an unknown
 * normaliser kind, a clip that is not > 0.  n = 0 is a no-op. */
int v2p_policy_input(const v2p_policy_input_cfg* cfg, int64_t n, int64_t dim, const float* obs /*[n,dim]*/, float* x /*[n,dim]*/, void* stream);
typedef struct {                  /* DEVICE buffers the imitation observation is computed from, in place */
    const float* rb_state;        /* [n,24,13] the engine's `_rigid_body_state` */
    const float* dof_state;       /* [n,69,2]  the engine's `_dof_state` */
    const float* target;          /* the packed current-target rows (layout of v2p_env_buffers.target): rb_pos, rb_rot, dof_pos are read */
    int64_t target_stride;        /* floats between the rows of `target` (>= 331) */
    const float* motion_bodies;   /* [n,11] `_reset_ref_motion_bodies` */
} v2p_ll_policy_src;
/* The same tail over the low-level policy's own observation: the 734 columns of v2p_obs_imitation (the same device code, the same bits)
 * are computed from the engine's state in place, written to raw_obs [n,734] in env order when it is given (nullable), and
 * x [n,734] = normaliser(clamp(row, +-clip_obs)) in side-major order.  Refused: as v2p_policy_input, and dim != 734, a null src or
 * pointer of it, target_stride < 331. */
int v2p_ll_policy_input(const v2p_policy_input_cfg* cfg, int64_t n, int64_t dim, const v2p_ll_policy_src* src, float* raw_obs /*[n,734] nullable*/,
                        float* x /*[n,734]*/, void* stream);
/* v2p_mvae_target_actions of clamp(mu, +-clip_actions), mu [n,75] in side-major order, actions_out [n,75] in env order (the same device
 * code as v2p_mvae_target_actions, the same bits).  actions_out must not alias mu with sides = 2.  Refused: as v2p_mvae_target_actions,
 * and sides outside {1, 2}, an odd n with two sides, a clip_actions that is not > 0. */
int v2p_ll_policy_actions(const v2p_mvae_target_cfg* cfg, int64_t n, int32_t sides, float clip_actions, const float* mu /*[n,75]*/,
                          const v2p_mvae_target_buffers* base_buffers, float* actions_out /*[n,75]*/, void* stream);

/* ---- The tennis controller's PPO agent (V2PAgent, vid2player/agents/v2p_agent.py, over PhysicsMVAEController): three row kernels.
 * All of them are built without FMA contraction, with the correctly rounded division and square root, and clamp by compare-and-select
 * (a NaN stays a NaN).  DEVICE pointers throughout. */
#define V2P_CTL_MAX_ACTIONS 128
#define V2P_CTL_MAX_SUB_REWARDS 8
/* What V2PModel.Network.forward(is_train = False) and the env wrapper do behind the `mu` layer (models/v2p_models.py:41-52,
 * env/tasks/vec_task.py:103), rows 0 .. n-1, columns 0 .. num_actions-1 (1 <= num_actions <= 128):
 *   actions = mu + sigma * noise;  mus = mu;  sigmas = sigma (every row);
 *   neglogp = 0.5 sum(((actions - mu) / sigma)^2) + float(0.5 log(2 pi) num_actions) + sum(logstd);
 *   actions_clamped = clamp(actions, +-clip_actions).
 * sigma [A] is exp(logstd), made by the caller; noise [n,A] are the caller's standard-normal draws.  The elementwise outputs are
 * torch's float32 results bit for bit; the two sums of neglogp are taken over the wave (columns k and k + 64 on lane k, then a
 * butterfly), so neglogp agrees with torch's to rounding.  actions_row / mus_row / sigmas_row (the experience buffer's rows) are
 * nullable.  Refused before any HIP call: n < 0, num_actions outside [1, 128], a clip_actions that is not > 0, a null mu, logstd,
 * sigma, noise, neglogp_row or actions_clamped.  n = 0 is a no-op. */
int v2p_ctl_policy_head(int64_t n, int32_t num_actions, const float* mu /*[n,A]*/, const float* logstd /*[A]*/, const float* sigma /*[A]*/,
                        const float* noise /*[n,A]*/, float clip_actions, float* actions_row /*[n,A] nullable*/, float* mus_row /*[n,A] nullable*/,
                        float* sigmas_row /*[n,A] nullable*/, float* neglogp_row /*[n]*/, float* actions_clamped /*[n,A]*/, void* stream);
/* The bookkeeping of V2PAgent.play_steps behind env_step (v2p_agent.py:245-276) in one launch.  obs [n,obs_dim], rew [n], reset /
 * terminate [n] int64 (the controller's buffers), sub_rewards [n,num_sub] with 0 <= num_sub <= 8 (nullable at 0):
 *   next_obs_row = clamp(obs, +-clip_obs) (the env wrapper's clamp; +inf: none);  rewards_row = rew;  dones_row = float(reset);
 *   terminated = float(terminate);  cur_rewards += rew;  cur_lengths += 1;
 *   acc[0] += the number of envs with reset != 0, acc[1] += the sum of their cur_rewards, acc[2] += the sum of their cur_lengths
 *   (what game_rewards / game_lengths receive), acc[3] += sum(rew) over ALL envs, sub_acc[k] += sum(sub_rewards[:, k]) over all envs
 *   (what the two AverageMeters receive, times n);  then cur_rewards *= 1 - dones, cur_lengths *= 1 - dones.
 * The sums are float64 and deterministic, with no atomics: workgroup 0 alone takes the per-env work; its thread t adds the envs
 * t, t + 256, ... in rising order, the 64 lanes of a wave combine by a butterfly (offsets 32, 16, .., 1; lane 0's value), the four
 * waves add as ((w0 + w1) + w2) + w3, and one thread adds the result to the accumulator.  The other workgroups stream the
 * observation rows.  Refused before any HIP call: n < 0, obs_dim < 1, num_sub outside [0, 8], a clip_obs that is not > 0, any null
 * pointer with n > 0 (sub_rewards / sub_acc only with num_sub > 0).  n = 0 is a no-op. */
int v2p_ctl_rollout_record(int64_t n, int64_t obs_dim, int32_t num_sub, float clip_obs, const float* obs, const float* rew, const int64_t* reset,
                           const int64_t* terminate, const float* sub_rewards, float* next_obs_row /*[n,obs_dim]*/, float* rewards_row /*[n]*/,
                           float* dones_row /*[n]*/, float* terminated /*[n]*/, float* cur_rewards /*[n] in/out*/, float* cur_lengths /*[n] in/out*/,
                           double* acc /*[4] in/out*/, double* sub_acc /*[num_sub] in/out*/, void* stream);
/* The controller's own bookkeeping around a reset by flags (`PhysicsMVAEController._reset_envs`, physics_mvae_controller.py:167-199):
 * flags [n] int64 is the controller's `reset_buf`, any non-zero value means "reset this env"; rows of envs whose flag is 0 keep every
 * bit.  v2p_ctl_reset_begin, for the flagged envs: progress = 0, terminate = 0, num_reset_reaction = 0, distance = 0, num_reset += 1.
 * v2p_ctl_reset_end, for the flagged envs: reset_reaction = 0 and reset_recovery = 0, then flags[e] = 0 - the mask is the buffer that
 * is cleared, so it goes last.  Between the two stand v2p_mvae_reset_flagged, v2p_mvae_target_reset_flagged,
 * v2p_env_push_state_flagged and v2p_tennis_task_reset (by its own two flags): one fixed sequence of launches, whatever the number of
 * flagged envs, with no host read of a device result.  Refused before any HIP call (V2P_ERR_INVALID, a message that names the call):
 * n < 0, null flags or buffers, a null pointer among the buffers the call writes.  n = 0 is a no-op. */
typedef struct {                    /* DEVICE buffers of the controller */
    int64_t* progress;              /* [n] begin */
    int64_t* terminate;             /* [n] begin */
    int64_t* num_reset_reaction;    /* [n] begin */
    int64_t* num_reset;             /* [n] begin */
    float* distance;                /* [n] begin */
    uint8_t* reset_reaction;        /* [n] end */
    uint8_t* reset_recovery;        /* [n] end */
} v2p_ctl_reset_buffers;
int v2p_ctl_reset_begin(int64_t n, const int64_t* flags /*[n]*/, const v2p_ctl_reset_buffers* buffers, void* stream);
int v2p_ctl_reset_end(int64_t n, int64_t* flags /*[n], cleared*/, const v2p_ctl_reset_buffers* buffers, void* stream);
/* ---- the two-player controller's reset of finished PAIRS by flags (`PhysicsMVAEControllerDual._reset_envs`,
 * physics_mvae_controller_dual.py:22-66, `HumanoidSMPLIMMVAEDual._reset_balls`, humanoid_smpl_im_mvae_dual.py:52-63).  Envs 2k and 2k+1
 * are a pair; a pair is flagged when EITHER of its two words of flags [n] int64 (the controller's `reset_buf`) is non-zero - the dual
 * step's law raises both, accepting either makes the entry total without a check on the host.  A pair that is not flagged keeps every
 * bit.  serve_from says who receives: V2P_SERVE_FROM_NEAR the even env of a pair (the odd env serves, :31-36), V2P_SERVE_FROM_FAR the
 * odd env.  The sequence, the same launches whether 0 or n / 2 pairs are done and with no host read of a device result:
 *   v2p_ctl_pair_reset_begin       one thread per pair: a word that is 0 in a flagged pair becomes 1 (the per-env flagged entries that
 *                                  follow then see a whole mask; a non-zero word keeps its value); for both envs progress = 0,
 *                                  terminate = 0, num_reset_reaction = 0, distance = 0, num_reset += 1; the receiver gets
 *                                  reset_reaction = 1, reset_recovery = 0 and the server reset_reaction = 0, reset_recovery = 1 (:31-38)
 *   v2p_mvae_dual_reset_flagged    (`dual_mode: different`; with one generator for both sides: v2p_mvae_reset_flagged on a per-env table
 *                                  of serve / ready frames)
 *   v2p_mvae_target_reset_flagged, v2p_env_push_state_flagged
 *   v2p_tennis_dual_serve_flagged  one thread per pair, after the generator's entry (which writes racket_pos): for the server s of a
 *                                  flagged pair ball_state[s,0:3] = racket_pos[s], ball_state[s,10:13] = (-40, 0, 0),
 *                                  ball_state[s,7:10] = u * (4, 4, 3) + (-2, 28, 5), product and sum each rounded in float32; columns
 *                                  3:7 are not touched.  u = row s >> 1 of draws [n/2,3] or, where draws is null, (word >> 8) * 2^-24 of
 *                                  words 0..2 of Philox4x32-10 block 0 of stream 3 (csrc/philox.hpp PHILOX_STREAM_SERVE) under
 *                                  (rule->seed, rule->call, s): a draw never depends on which other pairs are flagged
 *   v2p_tennis_dual_handover       as it is: the two flags that begin wrote make the serve the receiver's incoming ball
 *   v2p_ctl_pair_reset_end         flags[e] = 0 where it is not 0, and nothing else: reset_reaction and reset_recovery stay up as they
 *                                  do after the id-list reset (the next step overwrites them; v2p_ctl_reset_end clears them)
 * Equal, bit for bit, to the id-list reset of the flagged pairs.  Refused before any HIP call (V2P_ERR_INVALID, a message that names
 * the call): n < 0, an odd n, an unknown serve_from, a null flags / buffers / required pointer, the serve with neither draws nor a
 * rule, n above 2^31-1 where the env is a counter word.  n = 0 is a no-op. */
enum { V2P_SERVE_FROM_NEAR = 0, V2P_SERVE_FROM_FAR = 1 };
typedef struct {
    uint64_t seed, call;     /* `call` is the host's count of serve launches that draw */
} v2p_serve_rule;
int v2p_ctl_pair_reset_begin(int64_t n, int64_t* flags /*[n], made whole*/, const v2p_ctl_reset_buffers* buffers /*all seven*/, int32_t serve_from, void* stream);
int v2p_tennis_dual_serve_flagged(int64_t n, const int64_t* flags /*[n]*/, int32_t serve_from, const float* racket_pos /*[n,3]*/, float* ball_state /*[n,13]*/,
                                  const float* draws /*[n/2,3], nullable*/, const v2p_serve_rule* rule /*nullable with draws*/, void* stream);
int v2p_ctl_pair_reset_end(int64_t n, int64_t* flags /*[n], cleared*/, void* stream);

/* ---- the record of a match run (vid2player/env/tasks/mvae_controller_vis_dual.py:156-195: MVAEControllerVisDual.render_vis with cfg
 * env.record, called once after the first reset and after every control step, players/v2p_player.py:142,150) without a host read (the
 * reference: six .cpu() copies per step, a nonzero() and Python lists).
 *   frame   env e's frame goes to slot p = progress[e] of its own L = record_length slots of the six env-major arrays: `_joint_rot`
 *           (the row of v2p_tennis_eval_buffers.joint_rot, the same device lines), root and ball position, phase, swing type,
 *           tar_action.  p outside [0, L) (the reference would raise, or wrap below zero): nothing is stored and overflow[e] = 1.
 *           `target_pos_all` is allocated by the reference and never written in the dual class: it is left out.
 *   select  a pair (2k, 2k+1) is finished when either word of `reset` is not 0; d = distance[2k] + distance[2k+1] (one float32 add;
 *           a NaN sum is no candidate).  The candidate is the lowest finished pair that reaches the maximum of d - only this one pair
 *           is considered in a step.  It is inserted iff the list is empty or d > the last entry's, strict - so a candidate no better
 *           than the current worst is dropped even while the list holds fewer than num_best - in front of the first entry with
 *           d > entry (equal entries stay ahead); the list is cut to num_best.  best_distance / best_pair / best_nframes are by rank,
 *           best first; best_slot[rank] is the storage slot holding the rank's frames (a free one, or the evicted entry's), so frames
 *           are never shifted.  nframes = min(progress[2k], L); slots [0, nframes) of both envs are copied to
 *           best_*[slot, 0..1, 0..nframes-1] - the slot written this very step lies outside, as in the reference; what a storage slot
 *           held behind nframes stays.  decision = {pair, storage slot, nframes}, or {-1, -1, 0} without an insertion.
 * No atomics: two runs give the same bits. */
#define V2P_MATCH_RECORD_MAX_BEST 16
#define V2P_MATCH_RECORD_MAX_LENGTH (1 << 20)
typedef struct {
    int64_t record_length;          /* L, 1..V2P_MATCH_RECORD_MAX_LENGTH (the reference's hard-coded 1800) */
    int32_t num_best;               /* cfg env.num_eg, 1..V2P_MATCH_RECORD_MAX_BEST */
    int32_t body_of_smpl[24];       /* `_mujoco_2_smpl`: the engine's body of SMPL joint s; [0] = 0, a permutation */
} v2p_match_record_cfg;
typedef struct {                    /* DEVICE buffers, all required */
    /* read only */
    const float* rb_state;          /* [N,24,13] */
    const float* dof_state;         /* [N,69,2] the engine's DoF (position, velocity) pairs, body order */
    const float* ball_state;        /* [N,13] */
    const float* phase_pred;        /* [N] */
    const int64_t* swing_type_cycle; /* [N] */
    const int64_t* tar_action;      /* [N] */
    const int64_t* progress;        /* [N] after the step's increment */
    const int64_t* reset;           /* [N] */
    const float* distance;          /* [N] */
    /* the record, written by frame and read by select */
    float* joint_rot_all;           /* [N,L,24,3] */
    float* root_pos_all;            /* [N,L,3] */
    float* ball_pos_all;            /* [N,L,3] */
    float* phase_all;               /* [N,L] */
    int64_t* swing_type_all;        /* [N,L] */
    int64_t* tar_action_all;        /* [N,L] */
    int32_t* overflow;              /* [N] */
    /* the best list, read and written by select; best_count 0 before the first insertion */
    float* best_distance;           /* [num_best] by rank */
    int32_t* best_pair;             /* [num_best] */
    int32_t* best_nframes;          /* [num_best] */
    int32_t* best_slot;             /* [num_best] rank -> storage slot */
    int32_t* best_count;            /* [1] */
    int32_t* decision;              /* [3] */
    float* best_joint_rot;          /* [num_best,2,L,24,3] by storage slot */
    float* best_root_pos;           /* [num_best,2,L,3] */
    float* best_ball_pos;           /* [num_best,2,L,3] */
    float* best_phase;              /* [num_best,2,L] */
    int64_t* best_swing_type;       /* [num_best,2,L] */
    int64_t* best_tar_action;       /* [num_best,2,L] */
} v2p_match_record_buffers;
/* Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): a null cfg / buffers, n <= 0, an odd n, n above 2^31-1,
 * a null array, record_length or num_best outside their ranges, body_of_smpl that is no permutation with [0] = 0.  select launches the
 * selection (one workgroup) and the copy (a grid for 2 L frames, which returns at once without an insertion). */
int v2p_match_record_frame(const v2p_match_record_cfg* cfg, int64_t n, const v2p_match_record_buffers* buffers, void* stream);
int v2p_match_record_select(const v2p_match_record_cfg* cfg, int64_t n, const v2p_match_record_buffers* buffers, void* stream);

/* ---- the two-hand backhand fix of a record (vid2player/env/tasks/humanoid_smpl_im_mvae.py:948-1031, optimize_two_hand_backhand with
 * single=True, called as render_one_result calls it under cfg v2p fix_two_hand_backhand_post: mvae_controller_vis.py:181-190,
 * mvae_controller_vis_dual.py:213-231).  T tracks of L slots each, one workgroup per track, one launch:
 *   flags    frame f < nframes[t] of track t is flagged when swing_type == 2 and 2 < phase < 5; the F flagged frames are compacted in
 *            frame order.  Frames that are not flagged are copied to `out`; slots behind nframes[t] are neither read nor written.
 *   pose     all 24 joints of a flagged frame go angle_axis_to_rotation_matrix and rotation_matrix_to_angle_axis; the free arm's four
 *            joints (wrist, elbow, shoulder, collar: SMPL 20, 18, 16, 13 for righthand != 0, else 21, 19, 17, 14) get delta added
 *            in between.  Compacted frame i reads bind row i % num_bind (the reference's joint_pos_bind[:batch_size]).
 *   law      target = 2 rb_pos[hand] - rb_pos[wrist] - rb_pos[0] (bodies 23, 22 / 18, 17) from the input pose with root position 0;
 *            loss = mean|p_free - target| + 0.2 mean|delta| + 0.5 mean|delta[1:] - delta[:-1].detach()| (free hand: body 18 / 23);
 *            num_iters steps of Adam (lr 0.005, betas 0.9 / 0.999, eps 1e-8) as torch's single-tensor form runs it, from delta = 0.
 * Every float operation is the one of the numpy statement (two_hand_fix.two_hand_fix_reference) in its order, sine / cosine / the
 * closing arctangent evaluated in double and rounded once: the same bits.  No atomics, no host read, no allocation.
 * A track holds at most V2P_TWO_HAND_FIX_MAX_FRAMES flagged frames - V2P_TWO_HAND_FIX_FRAMES_PER_THREAD per thread of its workgroup,
 * whose delta and Adam moments stay in registers (at the cap the exchange of delta between neighbours takes 96 KB of the 160 KB of
 * LDS).  A track above the cap is copied whole and overflow[t] = F; else overflow[t] = 0. */
#define V2P_TWO_HAND_FIX_THREADS 256
#define V2P_TWO_HAND_FIX_FRAMES_PER_THREAD 8
#define V2P_TWO_HAND_FIX_MAX_FRAMES (V2P_TWO_HAND_FIX_THREADS * V2P_TWO_HAND_FIX_FRAMES_PER_THREAD)
typedef struct {
    int32_t num_iters;              /* >= 0 (the reference: 500) */
    int32_t num_bind;               /* R >= 1, rows of `bind` */
    int32_t smpl_parents[24];       /* the SMPL tree in SMPL joint order, root -1, a parent before its children */
    int32_t smpl_of_body[24];       /* `_smpl_2_mujoco`: the SMPL joint of the engine's body b; [0] = 0, a permutation */
} v2p_two_hand_fix_cfg;
typedef struct {                    /* DEVICE buffers, all required */
    const float* joint_rot;         /* [T,L,24,3] */
    const float* phase;             /* [T,L] */
    const int64_t* swing_type;      /* [T,L] */
    const int32_t* nframes;         /* [T], clamped to 0..L */
    const int32_t* righthand;       /* [T] */
    const float* bind;              /* [num_bind,24,3] */
    float* out;                     /* [T,L,24,3], no overlap with joint_rot */
    int32_t* overflow;              /* [T] */
} v2p_two_hand_fix_buffers;
/* Refused before any HIP call (V2P_ERR_INVALID, a message that names the call): a null cfg / buffers / array, T < 0, L < 1 or above
 * 2^31-1, num_iters < 0, num_bind < 1, a tree or a body table that is none, an arm that is not the chain collar - shoulder - elbow -
 * wrist - hand of the law's joints, a chain from the root longer than 12 joints, an `out` that is or overlaps joint_rot (the other
 * arrays are the caller's to keep apart from `out`).  T = 0 is a no-op. */
int v2p_two_hand_fix(const v2p_two_hand_fix_cfg* cfg, int64_t num_tracks, int64_t track_length, const v2p_two_hand_fix_buffers* buffers, void* stream);
/* The loss head of V2PAgent.calc_gradients (v2p_agent.py:329-362, 395-397; learning/common_agent.py:442-450, 491-520 with clip_value
 * False; PhysicsMVAEController.get_aux_losses) under a fixed sigma, forward and backward.  With row r of the minibatch and
 * j = idx ? idx[r] : r its row of the epoch's dataset:
 *   t = (actions[j] - mu[r]) / sigma;  neglogp = 0.5 sum(t^2) + float(0.5 log(2 pi) A) + sum(logstd);
 *   ratio = exp(old_neglogp[j] - neglogp);  a = max(-adv[j] ratio, -adv[j] clamp(ratio, 1 - e_clip, 1 + e_clip));
 *   c = (returns[j] - value[r])^2;  b = sum(clamp_max(mu + 1, 0)^2 + clamp_min(mu - 1, 0)^2) (0 without has_bounds_loss);
 *   d = sum(mu[r, c0:c1]^2);  loss = mean a + critic_coef mean c - entropy_coef ent + bounds_loss_coef mean b + dof_res_weight mean d.
 * grad_mu [B,A] and grad_value [B] are d loss / d mu and d loss / d value, computed directly (ties of the max split evenly and the
 * inclusive bounds of the clamp pass, as autograd has them).  stats[8] (float64): the means of a, c, b, d, of |ratio - 1| > e_clip,
 * of policy_kl(mu, sigma, old_mu[j], old_sigma) with its 1e-5 guards, the entropy sum(0.5 + 0.5 log(2 pi) + log(sigma)), and loss.
 * One wave per row (columns k and k + 64 on lane k); the statistics reduce in two stages - per-workgroup partials in float64 into
 * `partials`, then a second launch of one workgroup that adds them in workgroup order - so they are the same bits on every run.
 * A row whose j is outside [0, dataset_rows) gets NaN gradients and makes the statistics NaN; nothing is read for it. */
#define V2P_PPO_LOSS_MAX_BLOCKS 1024
#define V2P_PPO_LOSS_PARTIALS (6 * V2P_PPO_LOSS_MAX_BLOCKS) /* doubles of the `partials` workspace */
typedef struct {
    int32_t num_actions;       /* A, 1 .. 128 */
    int32_t has_bounds_loss;   /* 0: bounds_loss_coef None */
    int32_t c0, c1;            /* columns [c0, c1) of the residual-DoF means, 0 <= c0 <= c1 <= A (empty allowed) */
    int64_t dataset_rows;      /* rows of the dataset arrays (N * T); B with idx null */
    double e_clip;             /* > 0 */
    float critic_coef, entropy_coef, bounds_loss_coef, dof_res_weight;
} v2p_ppo_loss_cfg;
typedef struct {
    const float* mu;           /* [B,A] the network's means */
    const float* value;        /* [B] the network's values */
    const int64_t* idx;        /* [B] rows of the dataset, nullable = identity */
    const float* old_neglogp;  /* [rows] */
    const float* advantages;   /* [rows] */
    const float* returns;      /* [rows] */
    const float* actions;      /* [rows,A] */
    const float* old_mu;       /* [rows,A] */
    const float* old_sigma;    /* [A] */
    const float* logstd;       /* [A] */
    const float* sigma;        /* [A] exp(logstd) */
    float* grad_mu;            /* [B,A] out */
    float* grad_value;         /* [B] out */
    double* stats;             /* [8] out */
    double* partials;          /* [V2P_PPO_LOSS_PARTIALS] workspace */
} v2p_ppo_loss_buffers;
/* Refused before any HIP call: a null cfg / buffers, B < 0, A outside [1, 128], c0 / c1 outside 0 <= c0 <= c1 <= A, an e_clip that
 * is not > 0, dataset_rows < B without idx, any null pointer but idx with B > 0.  B = 0 is a no-op. */
int v2p_ppo_loss(const v2p_ppo_loss_cfg* cfg, int64_t B, const v2p_ppo_loss_buffers* buffers, void* stream);

/* measurement: HIP events around every launch of the physics kernel (the dominant kernel of the step), recorded on the launch stream
 * by v2p_env_step / v2p_env_physics between _begin and _end (at most max_launches of them).  _end synchronises the events and returns
 * the summed kernel time in milliseconds and the number of launches measured.  bench.py's roofline.kernel_ms comes from here, from
 * the very steps it times. */
int v2p_env_profile_begin(v2p_env* e, int64_t max_launches);
/* the same around a SAMPLE of the launches (ABI 10): launch L since _begin is bracketed when L % stride == (L / period) % stride, so
 * that with period = the steps of an epoch every position of the epoch is measured once in `stride` epochs.  Two event records per
 * launch cost ~8 us of dispatch on this stack (2 % of a 0.41 ms step): bench.py measures one launch in eight. */
int v2p_env_profile_begin_sampled(v2p_env* e, int64_t max_launches, int32_t stride, int32_t period);
int v2p_env_profile_end(v2p_env* e, double* physics_ms_total, int64_t* launches);

/* Substep jobs: a job whose predecessor (the previous substep of its env pair, another workgroup of the launch) does not show up within
 * ~20 ms stops waiting and recomputes the pair's earlier substeps itself - results and progress do not depend on the order in which the
 * hardware dispatches workgroups, only time is lost.  Every such recovery is counted on the device (it should never happen: jobs are
 * numbered the way workgroups are dispatched).  v2p_env_check synchronises `stream` and fetches the counter; v2p_env_check_async (ABI 9)
 * enqueues the fetch behind the work already on `stream` and picks up what the previous call's fetch brought back, without waiting (one
 * call per epoch: HumanoidSMPLIM.reset of all envs makes it); v2p_env_job_recoveries returns the count as last fetched (total since
 * the batch was created).
 * A recovery loses time only.  One consequence of it can lose DATA: when the late predecessor finally starts after the whole step of its pair
 * is complete, it must not run (its inputs are the next step's) and is skipped - and what only that job publishes (the exposed PD targets,
 * the in-place masking of dead envs' actions, the ball's per-simulate() records) is then missing for that step.  Such skips are counted
 * too (v2p_env_jobs_skipped, ABI 13); v2p_env_check returns V2P_ERR_INTERNAL the first time it sees new ones. */
int v2p_env_check(v2p_env* e, void* stream);
int v2p_env_check_async(v2p_env* e, void* stream);
int v2p_env_job_recoveries(v2p_env* e, int64_t* count);
int v2p_env_jobs_skipped(v2p_env* e, int64_t* count);

/* Guard zones and poison for the engine's own device arrays (ABI 15; a debugging aid of the test suite, off by default).
 * v2p_debug_guards sets the process-wide zone size and returns the previous one: 0 = off, otherwise a multiple of 256 bytes up to 1 MiB
 * (anything else: V2P_ERR_INVALID, nothing changed).  It is read when a batch allocates; a batch keeps what it was created with.  While
 * it is on, every array of a batch lies between two zones of 0xff bytes - the back zone begins at the array's end to the byte - and an
 * array the engine leaves unfilled is poisoned: 0xff bytes (a NaN) for float / double arrays, 0x00 for every other type (integer arrays
 * hold indices; zero is what a fresh page holds, so the poison cannot form a wild index).  v2p_env_check then also copies the zones back
 * and returns V2P_ERR_INTERNAL with a message that names the array, the side and the first byte when one was written.  Not seen: a store
 * past one slot of a structure-of-arrays buffer that stays inside the allocation, and a read-before-write of an integer array.
 * v2p_env_guard_counts: the arrays of the batch that lie between zones, and the float arrays among them that were poisoned (0, 0 for a
 * batch created with guards off).  v2p_debug_guards_selftest: writes one byte in front of one small array of its own and four bytes
 * behind another with hipMemset - inside its own allocations - and returns V2P_OK only when exactly that is reported. */
int v2p_debug_guards(int64_t zone_bytes);
int v2p_debug_guards_selftest(int device);
int v2p_env_guard_counts(const v2p_env* e, int64_t* guarded, int64_t* poisoned);

const char* v2p_last_error(void);
int v2p_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* V2P_ROLLOUT_H */
