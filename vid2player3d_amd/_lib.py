"""ctypes binding of libv2p_rollout.so (the C ABI in include/v2p_rollout.h).

There is NO fallback: if the HIP library is missing or a call fails, a RuntimeError is raised
(the reference's error convention is Python exceptions).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libv2p_rollout.so")

NUM_BODIES, NUM_DOF, NUM_ACTIONS, NUM_OBS = 24, 69, 75, 461
MOTION_STATE_DIM, CONTEXT_DIM = 331, 378
CONTEXT_DIM_CONF = CONTEXT_DIM + NUM_BODIES  # frames of a batch with a context transform: + joint_conf (humanoid_smpl_im.py:202-205)
CTX_MASK_JOINTS, CTX_NOISY_JOINTS, CTX_MASK_RANDOM_JOINTS = 1, 2, 3  # v2p_context_transform.ops
ABI_VERSION = 15

c_f = C.POINTER(C.c_float)
c_i32 = C.POINTER(C.c_int32)
c_i64 = C.POINTER(C.c_int64)
c_u8 = C.POINTER(C.c_uint8)
vp = C.c_void_p


class ModelDesc(C.Structure):
    _fields_ = [("num_bodies", C.c_int32), ("parents", c_i32), ("local_pos", c_f), ("mass", c_f), ("com", c_f), ("inertia", c_f),
                ("kp", c_f), ("kd", c_f), ("armature", c_f), ("hull_offsets", c_i32), ("hull_verts", c_f),
                ("limit_lower", c_f), ("limit_upper", c_f)]


class MotionTables(C.Structure):
    _fields_ = [("num_motions", C.c_int64), ("num_frames_total", C.c_int64), ("gts", vp), ("grs", vp), ("lrs", vp), ("grvs", vp),
                ("gravs", vp), ("dvs", vp), ("motion_lengths", vp), ("motion_num_frames", vp), ("motion_dt", vp),
                ("motion_min_verts_h", vp), ("length_starts", vp), ("motion_bodies", vp), ("key_body_ids", C.c_int32 * 4)]


class SimCfg(C.Structure):
    _fields_ = [("sim_dt", C.c_float), ("substeps", C.c_int32), ("control_freq_inv", C.c_int32), ("num_solver_iterations", C.c_int32),
                ("enable_contact", C.c_int32), ("residual_hold_sims", C.c_int32), ("gravity_z", C.c_float), ("friction", C.c_float),
                ("contact_offset", C.c_float), ("max_depenetration_velocity", C.c_float), ("erp", C.c_float),
                ("angular_damping", C.c_float), ("max_angular_velocity", C.c_float), ("pd_tar_lim", C.c_float),
                ("residual_force_scale", C.c_float), ("residual_torque_scale", C.c_float), ("ground_tolerance", C.c_float),
                ("max_episode_length", C.c_float), ("enable_early_termination", C.c_int32), ("context_length", C.c_int32),
                ("context_padding", C.c_int32), ("term_heights", C.c_float * 24), ("body_pos_weights", C.c_float * 24),
                ("reward_specs", C.c_float * 8), ("freeze_terminated_envs", C.c_int32), ("schedule", C.c_int32), ("pair_envs_by_load", C.c_int32),
                ("solver_type", C.c_int32), ("substep_jobs", C.c_int32), ("job_mono_permille", C.c_int32), ("pair_mix_permille", C.c_int32), ("debug_contacts", C.c_int32),
                ("joint_limits", C.c_int32), ("limit_margin", C.c_float),
                ("rest_offset", C.c_float), ("bounce_threshold_velocity", C.c_float), ("num_velocity_iterations", C.c_int32), ("kernel_build", C.c_int32),
                ("job_timeout_spins", C.c_int32), ("job_len", C.c_int32), ("job_lead", C.c_int32), ("job_no_interleave", C.c_int32),
                ("friction_frame", C.c_int32)]


class EnvBuffers(C.Structure):
    _fields_ = [("root_states", vp), ("dof_state", vp), ("rb_state", vp), ("contact_force", vp), ("dof_force", vp), ("pd_target", vp),
                ("obs", vp), ("rew", vp), ("sub_rewards", vp), ("reset", vp), ("terminate", vp), ("progress", vp), ("cur_time", vp),
                ("reset_time", vp), ("target", vp * 2), ("context_feat", vp), ("context_mask", vp)]


class BallCfg(C.Structure):
    _fields_ = [("radius", C.c_float), ("mass", C.c_float), ("inertia", C.c_float), ("restitution_ground", C.c_float), ("friction_ground", C.c_float),
                ("restitution_racket", C.c_float), ("friction_racket", C.c_float), ("bounce_threshold_velocity", C.c_float),
                ("angular_damping", C.c_float), ("max_angular_velocity", C.c_float), ("spin_scale", C.c_float), ("racket_link", C.c_int32),
                ("num_cylinders", C.c_int32), ("cylinders", (C.c_float * 8) * 2), ("racket_offset", C.c_float * 3),
                ("restitution_body", C.c_float), ("friction_body", C.c_float), ("body_contacts", C.c_int32), ("bounce_height", C.c_float),
                ("poll_racket_hits", C.c_int32)]


class BallBuffers(C.Structure):
    _fields_ = [("ball_state", vp), ("racket_state", vp), ("ball_per_sim", vp), ("racket_hit_per_sim", vp), ("ball_contact", vp),
                ("ball_body_contact", vp), ("has_bounce", vp), ("has_bounce_now", vp), ("bounce_pos", vp), ("has_racket_contact", vp),
                ("has_racket_contact_now", vp), ("contact_force_sum", vp)]


class RacketGeom(C.Structure):
    _fields_ = [("racket_link", C.c_int32), ("num_cylinders", C.c_int32), ("cylinders", (C.c_float * 8) * 2), ("racket_offset", C.c_float * 3)]


class BallSim(C.Structure):
    """v2p_ball_sim: a free ball on its own (v2p_ball_rollout)."""
    _fields_ = [("radius", C.c_float), ("mass", C.c_float), ("inertia", C.c_float), ("restitution_ground", C.c_float), ("friction_ground", C.c_float),
                ("bounce_threshold_velocity", C.c_float), ("angular_damping", C.c_float), ("max_angular_velocity", C.c_float), ("spin_scale", C.c_float),
                ("sim_dt", C.c_float), ("substeps", C.c_int32), ("control_freq_inv", C.c_int32), ("num_iterations", C.c_int32), ("solver_type", C.c_int32),
                ("gravity_z", C.c_float), ("contact_offset", C.c_float), ("erp", C.c_float), ("max_depenetration_velocity", C.c_float),
                ("enable_ground", C.c_int32), ("num_frames", C.c_int32), ("net_height", C.c_float), ("bounce_height", C.c_float), ("resample", C.c_int32),
                ("grid_x", C.c_double * 3), ("grid_y", C.c_double * 3)]


class BallRolloutOut(C.Structure):
    _fields_ = [("traj", vp), ("bounce_pos", vp), ("bounce_idx", vp), ("pass_net", vp), ("peak_after_bounce", vp), ("final_state", vp),
                ("traj_x", vp), ("traj_y", vp)]


class TennisCfg(C.Structure):
    """v2p_tennis_cfg: settings of the tennis controller's task step (v2p_tennis_task_step / _obs)."""
    _fields_ = [("reward_type", C.c_int32), ("obs_ball_traj_length", C.c_int32), ("use_history_ball_obs", C.c_int32), ("use_random_ball_target", C.c_int32),
                ("contact_by_velocity", C.c_int32), ("enable_early_termination", C.c_int32), ("max_episode_length", C.c_int64), ("grip_normal", C.c_float * 3),
                ("court_min", C.c_float * 2), ("court_max", C.c_float * 2), ("scale_pos", C.c_float), ("scale_phase", C.c_float), ("scale_bounce_pos", C.c_float),
                ("scale_bounce_time", C.c_float), ("weight_pos", C.c_float), ("weight_ball_pos", C.c_float), ("grid", (C.c_double * 3) * 5),
                ("table_rows", C.c_int64), ("table_nx", C.c_int32), ("table_ny", C.c_int32)]


TENNIS_BUFFER_NAMES = ("rb_state", "root_states", "racket_state", "ball_state", "wrist_link", "has_bounce", "has_bounce_now", "bounce_pos", "phase_pred", "swing_type",
                       "swing_type_cycle", "traj_out_x", "traj_out_y", "tar_time_total", "tar_action", "target_bounce_pos", "ball_traj", "has_racket_contact",
                       "has_racket_contact_now", "tar_time", "progress", "prev_ball_vy", "traj_cursor", "ball_obs", "bounce_in", "est_bounce_pos", "est_bounce_time",
                       "est_max_height", "est_bounce_in", "distance", "vel_x_overflow", "racket_pos", "racket_normal", "obs", "rew", "sub_rewards", "reset", "terminate",
                       "reset_reaction", "reset_recovery")


class TennisBuffers(C.Structure):
    _fields_ = [(k, vp) for k in TENNIS_BUFFER_NAMES]


TENNIS_METER_NAMES = ("hit_rate", "fh_ratio", "bounce_in_rate", "bounce_in_pos_error")  # V2P_TENNIS_METER_*


class TennisEvalCfg(C.Structure):
    """v2p_tennis_eval_cfg: what the evaluation step (v2p_tennis_eval_step) needs on top of v2p_tennis_cfg."""
    _fields_ = [("episode_length", C.c_int64), ("num_frames", C.c_int64), ("body_of_smpl", C.c_int32 * 24)]


class TennisEvalBuffers(C.Structure):
    """v2p_tennis_eval_buffers: the four meters (sum, count, avg, max of each, in the order of TENNIS_METER_NAMES) and the record."""
    _fields_ = [("meter_sum", vp * 4), ("meter_count", vp * 4), ("meter_avg", vp * 4), ("meter_max", vp * 4), ("dof_state", vp), ("joint_rot", vp), ("root_pos", vp),
                ("ball_pos", vp), ("target_pos", vp), ("phase", vp), ("swing_type_cycle", vp)]


MATCH_RECORD_MAX_BEST, MATCH_RECORD_MAX_LENGTH = 16, 1 << 20  # V2P_MATCH_RECORD_MAX_*


class MatchRecordCfg(C.Structure):
    """v2p_match_record_cfg: the settings of the match record (v2p_match_record_frame / _select)."""
    _fields_ = [("record_length", C.c_int64), ("num_best", C.c_int32), ("body_of_smpl", C.c_int32 * 24)]


MATCH_RECORD_INPUT_NAMES = ("rb_state", "dof_state", "ball_state", "phase_pred", "swing_type_cycle", "tar_action", "progress", "reset", "distance")
MATCH_RECORD_FRAME_NAMES = ("joint_rot", "root_pos", "ball_pos", "phase", "swing_type", "tar_action")  # the six `*_all` arrays and their `best_*` storage
MATCH_RECORD_TABLE_NAMES = ("best_distance", "best_pair", "best_nframes", "best_slot", "best_count", "decision")
MATCH_RECORD_BUFFER_NAMES = (MATCH_RECORD_INPUT_NAMES + tuple(k + "_all" for k in MATCH_RECORD_FRAME_NAMES) + ("overflow",) + MATCH_RECORD_TABLE_NAMES +
                             tuple("best_" + k for k in MATCH_RECORD_FRAME_NAMES))


class MatchRecordBuffers(C.Structure):
    _fields_ = [(k, vp) for k in MATCH_RECORD_BUFFER_NAMES]


TWO_HAND_FIX_THREADS, TWO_HAND_FIX_FRAMES_PER_THREAD = 256, 8  # V2P_TWO_HAND_FIX_*
TWO_HAND_FIX_MAX_FRAMES = TWO_HAND_FIX_THREADS * TWO_HAND_FIX_FRAMES_PER_THREAD


class TwoHandFixCfg(C.Structure):
    """v2p_two_hand_fix_cfg: the settings of the two-hand backhand fix (v2p_two_hand_fix)."""
    _fields_ = [("num_iters", C.c_int32), ("num_bind", C.c_int32), ("smpl_parents", C.c_int32 * 24), ("smpl_of_body", C.c_int32 * 24)]


TWO_HAND_FIX_BUFFER_NAMES = ("joint_rot", "phase", "swing_type", "nframes", "righthand", "bind", "out", "overflow")


class TwoHandFixBuffers(C.Structure):
    _fields_ = [(k, vp) for k in TWO_HAND_FIX_BUFFER_NAMES]


class TennisDualCfg(C.Structure):
    """v2p_tennis_dual_cfg: what the two-player step and hand-over need on top of v2p_tennis_cfg."""
    _fields_ = [("grip_normal", (C.c_float * 3) * 2), ("in_grid", (C.c_double * 3) * 4), ("in_rows", C.c_int64), ("in_frames", C.c_int32)]


TENNIS_DUAL_BUFFER_NAMES = ("traj_in", "target_draw", "ball_state", "has_bounce", "bounce_pos", "tar_action", "target_bounce_pos", "ball_traj", "num_reset_reaction")


class TennisDualBuffers(C.Structure):
    _fields_ = [(k, vp) for k in TENNIS_DUAL_BUFFER_NAMES]


class TennisResetCfg(C.Structure):
    """v2p_tennis_reset_cfg: what the flag-driven task reset (v2p_tennis_task_reset) needs on top of v2p_tennis_cfg."""
    _fields_ = [("reset_reaction_nframes", C.c_int64), ("target_mode", C.c_int32), ("pool_rule", C.c_int32), ("target_min", C.c_float * 3), ("target_max", C.c_float * 3),
                ("pool_rows", C.c_int64), ("pool_frames", C.c_int32), ("pool_stride", C.c_int64), ("seed", C.c_uint64), ("call", C.c_uint64)]


TENNIS_RESET_BUFFER_NAMES = ("pool", "sample_idx", "ball_state", "has_bounce", "bounce_pos", "has_racket_contact", "ball_traj", "tar_time_total", "tar_action",
                             "target_bounce_pos", "num_reset_reaction", "swing_type_cycle", "words")
TENNIS_TARGET_MODES = {False: 0, True: 1, "continuous": 2}  # V2P_TENNIS_TARGET_*
TENNIS_POOL_RULES = {"random": 0, "round_robin": 1}  # V2P_TENNIS_POOL_*


class TennisResetBuffers(C.Structure):
    _fields_ = [(k, vp) for k in TENNIS_RESET_BUFFER_NAMES]


class ControllerActionsCfg(C.Structure):
    """v2p_controller_actions_cfg: the action part of the controller's pre_physics_step (v2p_controller_actions)."""
    _fields_ = [("num_res_dof", C.c_int32), ("num_res_root", C.c_int32), ("random_walk", C.c_int32), ("vae_action_scale", C.c_float),
                ("residual_dof_scale", C.c_float), ("residual_root_scale", C.c_float), ("clamp", C.c_float), ("seed", C.c_uint64), ("call", C.c_uint64)]


class ControllerActionsBuffers(C.Structure):
    _fields_ = [("actions", vp), ("actions_stride", C.c_int64), ("tar_action", vp), ("words", vp), ("actions_out", vp), ("mvae_actions", vp),
                ("res_dof_actions", vp), ("res_root_actions", vp)]


class MvaeCfg(C.Structure):
    """v2p_mvae_cfg: sizes and switches of the MotionVAE motion generator (v2p_mvae_step / _reset)."""
    _fields_ = [(k, C.c_int32) for k in ("frame_size", "latent_size", "hidden_size", "num_experts", "gate_hidden_size", "num_condition_frames", "num_future_predictions",
                                         "predict_phase", "player", "righthand", "is_train", "add_residual_dof")]


MVAE_WEIGHT_NAMES = ("w0", "b0", "w1", "b1", "w2", "b2", "gate_w0", "gate_b0", "gate_w1", "gate_b1", "gate_w2", "gate_b2", "avg", "std")
MVAE_BUFFER_NAMES = ("conditions", "root_pos", "root_vel", "joint_rot6d", "joint_rotmat", "joint_rot", "racket_pos", "racket_normal", "phase_pred", "swing_type",
                     "swing_type_cycle")


class MvaeWeights(C.Structure):
    _fields_ = [(k, vp) for k in MVAE_WEIGHT_NAMES]


class MvaeBuffers(C.Structure):
    _fields_ = [(k, vp) for k in MVAE_BUFFER_NAMES]


MVAE_ROOT_RULES = {"centre": 0, "draw": 1}  # V2P_MVAE_ROOT_*


class MvaeRootRule(C.Structure):
    """v2p_mvae_root_rule: where v2p_mvae_reset_flagged takes the start of a reset env from when no table is given."""
    _fields_ = [("rule", C.c_int32), ("seed", C.c_uint64), ("call", C.c_uint64)]


CTL_RESET_BUFFER_NAMES = ("progress", "terminate", "num_reset_reaction", "num_reset", "distance", "reset_reaction", "reset_recovery")


class CtlResetBuffers(C.Structure):
    """v2p_ctl_reset_buffers: the controller's bookkeeping around a reset by flags (v2p_ctl_reset_begin / _end)."""
    _fields_ = [(k, vp) for k in CTL_RESET_BUFFER_NAMES]


SERVE_FROM = {"near": 0, "far": 1}  # V2P_SERVE_FROM_*: the even / the odd env of a pair receives


class ServeRule(C.Structure):
    """v2p_serve_rule: the key of the serve velocity that v2p_tennis_dual_serve_flagged draws when no table is given."""
    _fields_ = [("seed", C.c_uint64), ("call", C.c_uint64)]


class MvaeRacket(C.Structure):
    """v2p_mvae_racket: the one racket object of a two-player batch (v2p_mvae_dual_reset)."""
    _fields_ = [("righthand", C.c_int32), ("dir", C.c_float * 3), ("normal", C.c_float * 3)]


class MvaeTargetCfg(C.Structure):
    """v2p_mvae_target_cfg: settings of the imitation target from the motion generator's pose (v2p_mvae_target_step / _reset / _actions)."""
    _fields_ = [("dt", C.c_float), ("fix_head_orientation", C.c_int32), ("head_body", C.c_int32), ("smpl_head", C.c_int32), ("smpl_neck", C.c_int32),
                ("key_bodies", C.c_int32 * 4), ("smpl_parents", C.c_int32 * 24), ("smpl_of_body", C.c_int32 * 24), ("num_shapes", C.c_int32),
                ("pd_target_base", C.c_int32), ("no_scale_action", C.c_int32)]


MVAE_TARGET_BUFFER_NAMES = ("root_pos", "joint_rotmat", "residual_root", "ball_state", "joint_pos_bind", "env_shape_id", "target", "prev_target", "root_states",
                            "dof_state", "rb_state", "hold_reset", "hold_progress", "hold_cur_time", "pd_action_scale", "pd_action_offset")
PD_TARGET_BASES = {"target_pos": 0, "current_pos": 1, "none": 2}  # V2P_PD_BASE_*


class MvaeTargetBuffers(C.Structure):
    _fields_ = [(k, vp) for k in MVAE_TARGET_BUFFER_NAMES]


NORM_KINDS = {"none": 0, "running": 1, "mean_var": 2}  # V2P_NORM_*


class PolicyNorm(C.Structure):
    """v2p_policy_norm: the input normaliser of one side's network."""
    _fields_ = [("kind", C.c_int32), ("eps", C.c_float), ("clip", C.c_float), ("mean", vp), ("spread", vp)]


class PolicyInputCfg(C.Structure):
    """v2p_policy_input_cfg: the clamp and the normalisers in front of the policy networks (v2p_policy_input / v2p_ll_policy_input)."""
    _fields_ = [("sides", C.c_int32), ("clip_obs", C.c_float), ("norm", PolicyNorm * 2)]


class LLPolicySrc(C.Structure):
    """v2p_ll_policy_src: the engine's state the low-level policy's observation is computed from."""
    _fields_ = [("rb_state", vp), ("dof_state", vp), ("target", vp), ("target_stride", C.c_int64), ("motion_bodies", vp)]


CTL_MAX_ACTIONS, CTL_MAX_SUB_REWARDS = 128, 8
PPO_LOSS_MAX_BLOCKS = 1024
PPO_LOSS_PARTIALS = 6 * PPO_LOSS_MAX_BLOCKS  # doubles of v2p_ppo_loss_buffers.partials
PPO_LOSS_STATS = ("actor_loss", "critic_loss", "b_loss", "aux_dof_res_loss", "actor_clip_frac", "kl", "entropy", "loss")


class PpoLossCfg(C.Structure):
    """v2p_ppo_loss_cfg: the constants of the controller agent's loss head (v2p_ppo_loss)."""
    _fields_ = [("num_actions", C.c_int32), ("has_bounds_loss", C.c_int32), ("c0", C.c_int32), ("c1", C.c_int32), ("dataset_rows", C.c_int64),
                ("e_clip", C.c_double), ("critic_coef", C.c_float), ("entropy_coef", C.c_float), ("bounds_loss_coef", C.c_float), ("dof_res_weight", C.c_float)]


PPO_LOSS_BUFFER_NAMES = ("mu", "value", "idx", "old_neglogp", "advantages", "returns", "actions", "old_mu", "old_sigma", "logstd", "sigma", "grad_mu", "grad_value",
                         "stats", "partials")


class PpoLossBuffers(C.Structure):
    _fields_ = [(k, vp) for k in PPO_LOSS_BUFFER_NAMES]


class ContextTransform(C.Structure):
    _fields_ = [("num_ops", C.c_int32), ("ops", C.c_int32 * 3), ("mask_joints", C.c_uint32), ("noise_prob", C.c_float), ("noise_std", C.c_float),
                ("conf_std", C.c_float), ("min_conf", C.c_float), ("drop_prob", C.c_float)]


_lib = None


def load():
    """Load the HIP library; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libv2p_rollout.so is missing (%s): build it with `python -m vid2player3d_amd.build`; "
                           "there is no CPU fallback for the rollout engine" % LIB_PATH)
    # PyTorch-ROCm owns the device memory and the streams we launch on, and it ships its own HIP
    # runtime: import it first so that this library binds to the SAME libamdhip64 instance (two HIP
    # runtimes in one process do not see each other's devices or streams).
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    lib.v2p_last_error.restype = C.c_char_p
    lib.v2p_abi_version.restype = C.c_int
    if lib.v2p_abi_version() != ABI_VERSION:
        raise RuntimeError("libv2p_rollout.so ABI %d != binding ABI %d: rebuild" % (lib.v2p_abi_version(), ABI_VERSION))
    sig = {
        "v2p_model_create": [C.POINTER(ModelDesc), C.c_int, C.POINTER(vp)],
        "v2p_mlib_create": [C.POINTER(MotionTables), C.c_int, C.POINTER(vp)],
        "v2p_motion_state": [vp, vp, vp, C.c_int64, C.c_int, C.c_float, C.POINTER(vp * 9), vp],
        "v2p_reward": [C.c_int64] + [vp] * 8 + [c_f, c_f, vp, vp, vp],
        "v2p_reset_flags": [C.c_int64, vp, vp, c_f, vp, vp, C.c_float, C.c_int, vp, vp, vp],
        "v2p_obs_imitation": [C.c_int64] + [vp] * 10 + [vp, vp, C.c_float, vp, vp],
        "v2p_obs_imitation_packed": [C.c_int64, C.c_int64, vp, vp, C.c_int64, C.c_int64, vp, vp, C.c_float, vp, vp],
        "v2p_policy_head": [C.c_int64, vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp],
        "v2p_policy_head_record": [C.c_int64, vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp],
        "v2p_obs_imitation_packed_w": [C.c_int64, C.c_int64, vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp, C.c_float, vp, vp],
        "v2p_policy_head_w": [C.c_int64, vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp],
        "v2p_policy_head_record_w": [C.c_int64, vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp],
        "v2p_gae": [C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp],
        "v2p_value_record": [C.c_int64, vp, vp, vp, C.c_float, vp, vp, vp, vp],
        "v2p_rollout_record": [C.c_int64, vp, C.c_int64] + [vp] * 15,
        "v2p_motion_tables_build": [C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, c_i32, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp],
        "v2p_shapes_compile": [C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_double, C.c_int32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp],
        "v2p_env_create": [vp, vp, C.POINTER(SimCfg), vp, C.c_int64, C.POINTER(EnvBuffers), C.c_int, C.POINTER(vp)],
        "v2p_env_create_shapes": [C.POINTER(vp), C.c_int32, c_i32, vp, C.POINTER(SimCfg), vp, C.c_int64, C.POINTER(EnvBuffers), C.c_int, C.POINTER(vp)],
        "v2p_env_reset": [vp, vp, C.c_int64, vp, vp],
        "v2p_env_context": [vp, vp, C.c_int64, vp, vp],
        "v2p_env_set_context_transform": [vp, C.POINTER(ContextTransform), vp],
        "v2p_env_step": [vp, vp, vp],
        "v2p_env_pre_physics": [vp, vp, vp],
        "v2p_env_physics": [vp, vp],
        "v2p_env_export": [vp, vp],
        "v2p_env_post_physics": [vp, vp],
        "v2p_env_push_state": [vp, vp, C.c_int64, C.c_int, vp],
        "v2p_env_push_state_flagged": [vp, vp, C.c_int, vp],
        "v2p_env_target_index": [vp],
        "v2p_env_kernel_build": [vp],
        "v2p_env_set_schedule": [vp, C.c_int],
        "v2p_env_debug_contacts": [vp, vp, vp],
        "v2p_env_debug_contacts_substeps": [vp, vp, vp],
        "v2p_env_debug_pairing": [vp, vp, vp, vp],
        "v2p_env_check": [vp, vp],
        "v2p_env_check_async": [vp, vp],
        "v2p_env_job_recoveries": [vp, C.POINTER(C.c_int64)],
        "v2p_env_jobs_skipped": [vp, C.POINTER(C.c_int64)],
        "v2p_env_attach_ball": [vp, C.POINTER(BallCfg), C.POINTER(BallBuffers)],
        "v2p_env_set_racket_shapes": [vp, C.POINTER(RacketGeom), C.c_int32],
        "v2p_ball_rollout": [C.POINTER(BallSim), C.c_int64, vp, vp, vp, C.POINTER(BallRolloutOut), vp],
        "v2p_tennis_task_step": [C.POINTER(TennisCfg), C.c_int64, C.POINTER(TennisBuffers), C.POINTER(C.c_char_p), vp],
        "v2p_tennis_task_obs": [C.POINTER(TennisCfg), C.c_int64, C.POINTER(TennisBuffers), vp, C.c_int64, vp],
        "v2p_tennis_eval_step": [C.POINTER(TennisCfg), C.POINTER(TennisEvalCfg), C.c_int64, C.POINTER(TennisBuffers), C.POINTER(TennisEvalBuffers), C.c_int64,
                                 C.POINTER(C.c_char_p), vp],
        "v2p_tennis_dual_step": [C.POINTER(TennisCfg), C.POINTER(TennisDualCfg), C.c_int64, C.POINTER(TennisBuffers), C.POINTER(C.c_char_p), vp],
        "v2p_tennis_dual_handover": [C.POINTER(TennisCfg), C.POINTER(TennisDualCfg), C.c_int64, C.POINTER(TennisBuffers), C.POINTER(TennisDualBuffers), vp],
        "v2p_tennis_task_reset": [C.POINTER(TennisCfg), C.POINTER(TennisResetCfg), C.c_int64, C.POINTER(TennisBuffers), C.POINTER(TennisResetBuffers), vp],
        "v2p_controller_actions": [C.POINTER(ControllerActionsCfg), C.c_int64, C.POINTER(ControllerActionsBuffers), vp],
        "v2p_mvae_step": [C.POINTER(MvaeCfg), C.c_int64, C.POINTER(MvaeWeights), C.POINTER(MvaeBuffers), vp, vp, vp],
        "v2p_mvae_reset": [C.POINTER(MvaeCfg), C.c_int64, C.POINTER(MvaeWeights), C.POINTER(MvaeBuffers), vp, C.c_int64, vp, vp, vp, vp],
        "v2p_mvae_reset_flagged": [C.POINTER(MvaeCfg), C.c_int64, C.POINTER(MvaeWeights), C.POINTER(MvaeBuffers), vp, vp, vp, C.POINTER(MvaeRootRule), vp, vp],
        "v2p_mvae_dual_step": [C.POINTER(MvaeCfg), C.c_int64, C.POINTER(MvaeWeights), C.POINTER(MvaeBuffers), vp, vp, C.c_int32, vp],
        "v2p_mvae_dual_reset": [C.POINTER(MvaeCfg), C.c_int64, C.POINTER(MvaeWeights), C.POINTER(MvaeBuffers), C.POINTER(MvaeRacket), vp, C.c_int64, vp, vp, vp, C.c_int64, vp],
        "v2p_mvae_target_step": [C.POINTER(MvaeTargetCfg), C.c_int64, C.POINTER(MvaeTargetBuffers), vp],
        "v2p_mvae_target_reset": [C.POINTER(MvaeTargetCfg), C.c_int64, C.POINTER(MvaeTargetBuffers), vp, C.c_int64, vp],
        "v2p_mvae_target_reset_flagged": [C.POINTER(MvaeTargetCfg), C.c_int64, C.POINTER(MvaeTargetBuffers), vp, vp],
        "v2p_ctl_reset_begin": [C.c_int64, vp, C.POINTER(CtlResetBuffers), vp],
        "v2p_ctl_reset_end": [C.c_int64, vp, C.POINTER(CtlResetBuffers), vp],
        "v2p_ctl_pair_reset_begin": [C.c_int64, vp, C.POINTER(CtlResetBuffers), C.c_int32, vp],
        "v2p_ctl_pair_reset_end": [C.c_int64, vp, vp],
        "v2p_match_record_frame": [C.POINTER(MatchRecordCfg), C.c_int64, C.POINTER(MatchRecordBuffers), vp],
        "v2p_match_record_select": [C.POINTER(MatchRecordCfg), C.c_int64, C.POINTER(MatchRecordBuffers), vp],
        "v2p_two_hand_fix": [C.POINTER(TwoHandFixCfg), C.c_int64, C.c_int64, C.POINTER(TwoHandFixBuffers), vp],
        "v2p_tennis_dual_serve_flagged": [C.c_int64, vp, C.c_int32, vp, vp, vp, C.POINTER(ServeRule), vp],
        "v2p_mvae_dual_reset_flagged": [C.POINTER(MvaeCfg), C.c_int64, C.POINTER(MvaeWeights), C.POINTER(MvaeBuffers), C.POINTER(MvaeRacket), vp, vp, vp, C.POINTER(MvaeRootRule), vp,
                                        C.c_int64, vp],
        "v2p_mvae_target_actions": [C.POINTER(MvaeTargetCfg), C.c_int64, vp, C.POINTER(MvaeTargetBuffers), vp, vp],
        "v2p_policy_input": [C.POINTER(PolicyInputCfg), C.c_int64, C.c_int64, vp, vp, vp],
        "v2p_ll_policy_input": [C.POINTER(PolicyInputCfg), C.c_int64, C.c_int64, C.POINTER(LLPolicySrc), vp, vp, vp],
        "v2p_ll_policy_actions": [C.POINTER(MvaeTargetCfg), C.c_int64, C.c_int32, C.c_float, vp, C.POINTER(MvaeTargetBuffers), vp, vp],
        "v2p_ctl_policy_head": [C.c_int64, C.c_int32, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp],
        "v2p_ctl_rollout_record": [C.c_int64, C.c_int64, C.c_int32, C.c_float] + [vp] * 14,
        "v2p_ppo_loss": [C.POINTER(PpoLossCfg), C.c_int64, C.POINTER(PpoLossBuffers), vp],
        "v2p_debug_guards": [C.c_int64],
        "v2p_debug_guards_selftest": [C.c_int],
        "v2p_env_guard_counts": [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
        "v2p_env_profile_begin": [vp, C.c_int64],
        "v2p_env_profile_begin_sampled": [vp, C.c_int64, C.c_int32, C.c_int32],
        "v2p_env_profile_end": [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    for name in ("v2p_model_destroy", "v2p_mlib_destroy", "v2p_env_destroy"):
        fn = getattr(lib, name)
        fn.argtypes = [vp]
        fn.restype = None
    _lib = lib
    return lib


EXPORTED_SYMBOLS = (
    "v2p_model_create", "v2p_model_destroy", "v2p_mlib_create", "v2p_mlib_destroy", "v2p_motion_state", "v2p_reward", "v2p_reset_flags",
    "v2p_obs_imitation", "v2p_obs_imitation_packed", "v2p_policy_head", "v2p_policy_head_record", "v2p_obs_imitation_packed_w", "v2p_policy_head_w", "v2p_policy_head_record_w", "v2p_gae", "v2p_value_record", "v2p_rollout_record", "v2p_motion_tables_build", "v2p_shapes_compile", "v2p_env_create", "v2p_env_create_shapes", "v2p_env_destroy", "v2p_env_reset", "v2p_env_context", "v2p_env_set_context_transform", "v2p_env_step", "v2p_env_pre_physics", "v2p_env_physics", "v2p_env_export",
    "v2p_env_post_physics", "v2p_env_push_state", "v2p_env_target_index", "v2p_env_kernel_build", "v2p_env_set_schedule", "v2p_env_debug_contacts", "v2p_env_debug_contacts_substeps", "v2p_env_debug_pairing", "v2p_env_attach_ball", "v2p_env_set_racket_shapes", "v2p_env_check", "v2p_env_check_async", "v2p_env_job_recoveries", "v2p_env_jobs_skipped", "v2p_env_profile_begin", "v2p_env_profile_begin_sampled", "v2p_env_profile_end", "v2p_ball_rollout", "v2p_tennis_task_step", "v2p_tennis_task_obs", "v2p_tennis_dual_step", "v2p_tennis_dual_handover", "v2p_controller_actions", "v2p_tennis_task_reset", "v2p_mvae_step", "v2p_mvae_reset", "v2p_mvae_dual_step", "v2p_mvae_dual_reset", "v2p_mvae_target_step", "v2p_mvae_target_reset", "v2p_mvae_target_actions", "v2p_policy_input", "v2p_ll_policy_input", "v2p_ll_policy_actions", "v2p_ctl_policy_head", "v2p_ctl_rollout_record", "v2p_ppo_loss", "v2p_last_error", "v2p_abi_version",
    "v2p_debug_guards", "v2p_debug_guards_selftest", "v2p_env_guard_counts",
    "v2p_mvae_reset_flagged", "v2p_mvae_target_reset_flagged", "v2p_env_push_state_flagged", "v2p_ctl_reset_begin", "v2p_ctl_reset_end",
    "v2p_ctl_pair_reset_begin", "v2p_ctl_pair_reset_end", "v2p_tennis_dual_serve_flagged", "v2p_mvae_dual_reset_flagged",
    "v2p_tennis_eval_step",
    "v2p_match_record_frame", "v2p_match_record_select",
    "v2p_two_hand_fix",
)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, load().v2p_last_error().decode()))


def ptr(t):
    """Device (or host) address of a torch tensor / None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream(device):
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
