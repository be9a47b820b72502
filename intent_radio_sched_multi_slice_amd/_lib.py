"""ctypes binding of the C ABI in include/ranenv.h (libranenv_hip.so).

There is no fallback: if the HIP library is missing the import of the product path fails
loudly, and every non-zero status from the library raises RanEnvError.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RANENV_LIB") or os.path.join(_HERE, "csrc", "libranenv_hip.so")

ABI_VERSION = 10
POLICY_EXTERNAL, POLICY_MARR, POLICY_MAPF, POLICY_NETWORK, POLICY_HEAD_NETWORK = 0, 1, 2, 3, 4
HEAD_DIST_GAUSS_CLIP, HEAD_DIST_GAUSS_TANH = 0, 1
HEAD_SRC_HEAD, HEAD_SRC_INTER = 0, 1
ACT_TANH, ACT_RELU = 0, 1
NET_IN_OBS, NET_IN_MASK_OBS = 0, 1
NET_F32, NET_BF16 = 0, 1
NET_PRECISIONS = {"f32": NET_F32, "bf16": NET_BF16}
NET_MAX_HIDDEN, NET_MAX_WIDTH = 4, 512
INTRA_RR, INTRA_PF, INTRA_MT, INTRA_PER_SLICE = 0, 1, 2, 255
F_CLEAR_HISTORY_ON_RESET, F_NO_RAW_OUTPUT, F_SYNC_CHECK, F_SCALE_PER_ELEMENT = 0x1, 0x2, 0x4, 0x8
SE_STREAM, SE_GATHER = 0, 1
SLICE_METRIC_COLS = 10
LOAD_SLICE_COLS = 6

class RanEnvError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("n_slices", C.c_int32),
        ("n_ues", C.c_int32), ("n_rbs", C.c_int32), ("rbs_per_rbg", C.c_int32), ("max_ues_slice", C.c_int32),
        ("hist_depth", C.c_int32), ("max_age_cap", C.c_int32), ("max_steps", C.c_int32),
        ("n_scenarios", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
        ("bandwidth_hz", C.c_double), ("overfulfill", C.c_double), ("norm_traffic", C.c_double),
        ("norm_ues", C.c_double), ("norm_se", C.c_double),
    ]


SCENARIO_FIELDS = (
    "slice_active", "slice_has_req", "slice_nues", "slice_ues", "slice_priority", "slice_traffic",
    "slice_buffer_size", "slice_buffer_latency", "slice_message_size", "slice_nparams", "param_metric",
    "param_op", "param_value", "sorted_slices", "ue_slice", "ue_pos", "ue_pkt_size", "ue_max_pkts", "ue_max_age",
)
SCENARIO_F64 = {"slice_priority", "slice_traffic", "param_value"}


class ScenarioTablesC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SCENARIO_FIELDS]


class Episode(C.Structure):
    _fields_ = [
        ("scenario", C.c_int32), ("se_len", C.c_int32), ("se_base", C.c_int64), ("se_offset", C.c_int32),
        ("trf_len", C.c_int32), ("trf_base", C.c_int64), ("trf_offset", C.c_int32), ("reserved", C.c_int32),
    ]


VIEW_FIELDS = (
    ("pkt_incoming", "i4", "BU"), ("pkt_throughputs", "i4", "BU"), ("pkt_effective_thr", "i4", "BU"),
    ("dropped_pkts", "i4", "BU"), ("queue_pkts", "i4", "BU"), ("queue_age_sum", "i8", "BU"),
    ("rb_start", "i4", "BU"), ("rb_count", "i4", "BU"), ("se_mean", "f8", "BU"), ("win_sent", "i8", "BU"),
    ("win_dropped", "i8", "BU"), ("step_number", "i4", "B"), ("hist_len", "i4", "B"),
    ("mask_inter", "i1", "BS"), ("mask_intra", "i1", "BSK"), ("policy_scores", "f8", "BS"),
    ("episode_number", "i4", "B"), ("episodes", "i4", "BE"),
)


class Mlp(C.Structure):
    """ranenv_mlp: n_hidden Linear + activation layers and an output Linear, torch layout, device pointers."""
    _fields_ = [("n_hidden", C.c_int32), ("activation", C.c_int32), ("input_layout", C.c_int32), ("precision", C.c_int32),
                ("dims", C.c_int32 * 6), ("weight", C.c_void_p * 5), ("bias", C.c_void_p * 5)]


TRAJECTORY_FIELDS = ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "action_inter", "action_intra", "logp", "vf", "reward", "done",
                     "adv", "vtarg")


class Trajectory(C.Structure):
    """ranenv_trajectory: caller-owned device pointers of a ranenv_collect record, [t]-major (NULL = not recorded)."""
    _fields_ = [(n, C.c_void_p) for n in TRAJECTORY_FIELDS]


HEAD_TRAJECTORY_FIELDS = ("obs_head", "action", "logp", "vf", "reward_head", "done", "adv", "vtarg")


class PpoHparams(C.Structure):
    """ranenv_ppo_hparams: one member's hyper-parameters of ranenv_ppo_update."""
    _fields_ = [(n, C.c_double) for n in ("lr", "clip", "vf_coeff", "ent_coeff", "grad_clip", "beta1", "beta2", "eps")] + [
        (n, C.c_int32) for n in ("minibatch", "epochs", "adv_norm", "reserved")]


PPO_ROWS_MEMBERS, PPO_ROWS_SLICES = 0, 1      # ranenv_ppo_row_count / _row_order: the grouping
PPO_STATS = ("policy_loss", "value_loss", "entropy", "kl", "clip_frac", "grad_norm", "rows", "minibatches")
SAC_STATS = ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef", "logp_mean", "q1_mean", "q2_mean", "target_mean")
SAC_NETS = {"actor": 0, "q1": 1, "q2": 2, "q1_target": 3, "q2_target": 4}
SAC_ACTOR_TAG = 0x53415000       # counter word c3 of the SAC update's actor-pass draws: tag + position (include/ranenv.h "SAC update")


class HeadTrajectory(C.Structure):
    """ranenv_head_trajectory: caller-owned device pointers of a ranenv_collect_head record, [t]-major (NULL = not recorded)."""
    _fields_ = [(n, C.c_void_p) for n in HEAD_TRAJECTORY_FIELDS]


class Replay(C.Structure):
    """ranenv_replay: the caller-owned replay ring of ranenv_collect_replay, [slot]-major device pointers (all required)."""
    _fields_ = [("capacity", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_void_p) for n in ("obs", "next_obs", "action", "reward_head", "done")]


# ranenv_trace's device buffers in declaration order: name -> (typestr, trailing shape in the letters of BatchedRanEnv.bind_trace)
TRACE_FIELDS = (
    ("pkt_incoming", "i4", "U"), ("pkt_throughputs", "i4", "U"), ("pkt_effective_thr", "i4", "U"), ("dropped_pkts", "i4", "U"),
    ("queue_pkts", "i4", "U"), ("rb_start", "i4", "U"), ("rb_count", "i4", "U"), ("queue_age_sum", "i8", "U"), ("se", "f4", "RU"),
    ("reward", "f8", "P"), ("scores", "f8", "S"), ("intra", "u1", "S"), ("obs_inter", "f4", "I"), ("obs_intra", "f4", "SW"),
    ("step_number", "i4", ""), ("episode_number", "i4", ""), ("scenario", "i4", ""), ("done", "u1", ""),
)


class Trace(C.Structure):
    """ranenv_trace: the caller-owned ring of ranenv_bind_trace, [capacity][n_envs][...] device pointers (NULL = not recorded) and
    the HOST list of recorded envs."""
    _fields_ = [("n_envs", C.c_int32), ("capacity", C.c_int32), ("envs", C.c_void_p)] + [(n, C.c_void_p) for n, _, _ in TRACE_FIELDS]


class Views(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in VIEW_FIELDS]


# Every function of the C ABI: name -> (restype, argtypes).  Pointers (handle, device buffers, streams) pass as void *.
_P, _I32, _I64, _F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
FUNCTIONS = {
    "ranenv_last_error": (C.c_char_p, [_P]),
    "ranenv_abi_version": (C.c_int, []),
    "ranenv_create": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "ranenv_destroy": (C.c_int, [_P]),
    "ranenv_load_scenarios": (C.c_int, [_P, _I32, _I32, C.POINTER(ScenarioTablesC), _P]),
    "ranenv_bind_se_pool": (C.c_int, [_P, _P, _I64, _I64]),
    "ranenv_bind_traffic_pool": (C.c_int, [_P, _P, _I64]),
    "ranenv_set_episodes": (C.c_int, [_P, _P, _P]),
    "ranenv_set_policy": (C.c_int, [_P, _I32, _I32]),
    "ranenv_reset": (C.c_int, [_P] + [_P] * 6),
    "ranenv_step": (C.c_int, [_P] + [_P] * 9),
    "ranenv_step_dense": (C.c_int, [_P] + [_P] * 8),
    "ranenv_profile_begin": (C.c_int, [_P]),
    "ranenv_profile_end": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "ranenv_profile_ttis": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "ranenv_get_views": (C.c_int, [_P, C.POINTER(Views)]),
    "ranenv_launch_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ranenv_se_from_power": (C.c_int, [_P, _P, _I64, _F64, _F64, _P]),
    "ranenv_bind_head_outputs": (C.c_int, [_P, _P, _P]),
    "ranenv_set_slice_usecase": (C.c_int, [_P, _I32, _I32, _P, _P]),
    "ranenv_set_traffic_generator": (C.c_int, [_P, _I32, C.c_uint64, _I32, _P]),
    "ranenv_set_max_steps": (C.c_int, [_P, _P, _P]),
    "ranenv_set_episode_table": (C.c_int, [_P, _P, _I32, _I32, _P]),
    "ranenv_set_autoreset": (C.c_int, [_P, _I32, _I32, _I32, _I32, C.c_uint64, _P, _P]),
    "ranenv_autoreset": (C.c_int, [_P] + [_P] * 7),
    "ranenv_get_poisson_tables": (C.c_int, [_P, _P, _P]),
    "ranenv_set_partitions": (C.c_int, [_P, _I32]),
    "ranenv_rollout": (C.c_int, [_P, _I32] + [_P] * 5),
    "ranenv_enable_metrics": (C.c_int, [_P, _I32, _P]),
    "ranenv_get_metrics": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "ranenv_step_range": (C.c_int, [_P, _I32, _I32] + [_P] * 9),
    "ranenv_set_se_mode": (C.c_int, [_P, _I32, _P]),
    "ranenv_get_se_sidecars": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "ranenv_step_part": (C.c_int, [_P, _I32] + [_P] * 9),
    "ranenv_wait_part": (C.c_int, [_P, _I32, _P]),
    "ranenv_get_partition": (C.c_int, [_P, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ranenv_get_part_stream": (C.c_int, [_P, _I32, C.POINTER(C.c_void_p)]),
    "ranenv_autoreset_part": (C.c_int, [_P, _I32] + [_P] * 7),
    "ranenv_set_option": (C.c_int, [_P, C.c_char_p, _I64]),
    "ranenv_get_option": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "ranenv_profile_work": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_bind_se_gather_from_power": (C.c_int, [_P, _P, _I64, _F64, _F64, _P]),
    "ranenv_bind_se_pool_quad": (C.c_int, [_P, _P, _I64, _I64]),
    "ranenv_se_retile_quad": (C.c_int, [_P, _P, _I64, _I32, _I32, _P]),
    "ranenv_packed_step_fits": (C.c_int, [C.POINTER(Config), _I64, _I64]),
    "ranenv_se_retile_member_lines": (C.c_int, [_P, _I32, _I64, _P, _I64, _I32, _I32, _P]),
    "ranenv_member_line_plan": (C.c_int, [_I32, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ranenv_member_lines_row_sums_host": (C.c_int, [_P, _I32, _I32, _I32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ranenv_member_lines_owner_tail_sums_host": (C.c_int, [_P, _I32, _I32, _I32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "ranenv_se_retile_member_lines_packed": (C.c_int, [_P, _I32, _I64, _P, _I64, _I32, _I32, _P]),
    "ranenv_member_lines_packed_layout": (C.c_int, [_I32, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_member_lines_packed_sums_host": (C.c_int, [_P, _P, _I32, _I32, _I32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ranenv_member_serving_order": (C.c_int, [C.c_uint64, C.c_uint64, _I32, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ranenv_selftest_ddiv": (C.c_int, [_P, _P, _P, _P, _I64, _P]),
    "ranenv_set_policy_network": (C.c_int, [_P, C.POINTER(Mlp), C.POINTER(Mlp), _I32, C.c_uint64, _P]),
    "ranenv_get_policy_actions": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "ranenv_set_value_network": (C.c_int, [_P, C.POINTER(Mlp), C.POINTER(Mlp), _P]),
    "ranenv_collect": (C.c_int, [_P, _I32, C.POINTER(Trajectory), _F64, _F64] + [_P] * 5),
    "ranenv_gae": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _F64, _F64, _P, _P, _P]),
    "ranenv_set_head_policy_network": (C.c_int, [_P, C.POINTER(Mlp), _I32, _P, _I32, C.c_uint64, _P]),
    "ranenv_set_head_value_network": (C.c_int, [_P, C.POINTER(Mlp), _P]),
    "ranenv_get_head_metrics": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "ranenv_collect_head": (C.c_int, [_P, _I32, C.POINTER(HeadTrajectory), _I32, _F64, _F64] + [_P] * 5),
    "ranenv_enable_slice_metrics": (C.c_int, [_P, _I32, _P]),
    "ranenv_get_slice_metrics": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "ranenv_bind_replay": (C.c_int, [_P, C.POINTER(Replay)]),
    "ranenv_collect_replay": (C.c_int, [_P, _I32] + [_P] * 5),
    "ranenv_get_replay_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "ranenv_replay_sample": (C.c_int, [_P, _I64, C.c_uint64, C.c_uint64, _I32] + [_P] * 7),
    "ranenv_set_sac_critics": (C.c_int, [_P, C.POINTER(Mlp), C.POINTER(Mlp), _P]),
    "ranenv_sac_targets": (C.c_int, [_P, _I64, _P, _P, _P, _F64, _F64, _I32, C.c_uint64, C.c_uint64] + [_P] * 5),
    "ranenv_set_intra_policy_networks": (C.c_int, [_P, _I32, C.POINTER(C.POINTER(Mlp)), _P]),
    "ranenv_set_intra_value_networks": (C.c_int, [_P, _I32, C.POINTER(C.POINTER(Mlp)), _P]),
    "ranenv_set_head_policy_source": (C.c_int, [_P, _I32]),
    "ranenv_build_se_stats": (C.c_int, [_P, _P]),
    "ranenv_get_se_stats": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "ranenv_rbs_needed": (C.c_int, [_P, _P, _I32, _I32, _P, _P, _P, _P]),
    "ranenv_bind_trace": (C.c_int, [_P, C.POINTER(Trace), _P]),
    "ranenv_get_trace_counts": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "ranenv_reset_trace": (C.c_int, [_P, _P]),
    "ranenv_set_population": (C.c_int, [_P, _I32, C.POINTER(C.c_int32)]),
    "ranenv_get_population": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ranenv_set_population_policy": (C.c_int, [_P, _I32, C.POINTER(C.POINTER(Mlp)), C.POINTER(C.POINTER(Mlp)), _I32, C.c_uint64, _P]),
    "ranenv_set_population_value": (C.c_int, [_P, _I32, C.POINTER(C.POINTER(Mlp)), C.POINTER(C.POINTER(Mlp)), _P]),
    "ranenv_set_population_member": (C.c_int, [_P, _I32] + [C.POINTER(Mlp)] * 4 + [_P]),
    "ranenv_population_tiles": (C.c_int, [_I32, C.POINTER(C.c_int32), _I32, _I32, _I32] + [C.POINTER(C.c_int32)] * 4),
    "ranenv_set_population_policy_mixed": (C.c_int, [_P, _I32, C.POINTER(C.POINTER(Mlp)), C.POINTER(C.POINTER(Mlp)), _I32, C.c_uint64, _P]),
    "ranenv_set_population_value_mixed": (C.c_int, [_P, _I32, C.POINTER(C.POINTER(Mlp)), C.POINTER(C.POINTER(Mlp)), _P]),
    "ranenv_get_population_net": (C.c_int, [_P, _I32, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64)]),
    "ranenv_packed_net_floats": (C.c_int, [_I32, C.POINTER(C.c_int32), _I32, C.POINTER(C.c_int64)]),
    "ranenv_set_population_gae": (C.c_int, [_P, _I32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ranenv_gae_population": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _I32, C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P, _P]),
    "ranenv_ppo_bind": (C.c_int, [_P, _P]),
    "ranenv_ppo_update": (C.c_int, [_P, _I32, C.POINTER(Trajectory), _I32, C.POINTER(PpoHparams), _P, C.POINTER(C.c_int32), _P, C.POINTER(C.c_int32), _P, _P, _P]),
    "ranenv_ppo_layout": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_ppo_state": (C.c_int, [_P, _I32, _I32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "ranenv_ppo_probe_logp": (C.c_int, [_P, _P]),
    "ranenv_ppo_row_count": (C.c_int, [_P, _I32, _P, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "ranenv_ppo_row_order": (C.c_int, [_P, _I32, _P, _I32, _I32, C.c_uint64, _P, _P, _P]),
    "ranenv_get_net_weights": (C.c_int, [_P, _I32, _I32, C.POINTER(Mlp), _P]),
    "ranenv_ppo_bind_mixed": (C.c_int, [_P, _P]),
    "ranenv_ppo_member_layout": (C.c_int, [_P, _I32, _I32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_ppo_lds_bytes": (C.c_int, [C.POINTER(Mlp), C.POINTER(Mlp), C.POINTER(C.c_int64)]),
    "ranenv_ppo_bind_wide": (C.c_int, [_P, _I32, _P]),
    "ranenv_ppo_wide_bytes": (C.c_int, [C.POINTER(Mlp), C.POINTER(Mlp), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_ppo_bind_slices": (C.c_int, [_P, _I32, _P]),
    "ranenv_ppo_bind_spread": (C.c_int, [_P, _I32, _I32, _P]),
    "ranenv_ppo_spread_bytes": (C.c_int, [C.POINTER(Mlp), C.POINTER(Mlp), _I32, _I32, C.POINTER(C.c_int64)]),
    "ranenv_ppo_spread_plan": (C.c_int, [C.c_int64, _I32, _I32, _I32, C.POINTER(C.c_int64), C.POINTER(_I32), C.POINTER(_I32)]),
    "ranenv_ppo_bind_slices_spread": (C.c_int, [_P, _I32, _I32, _P]),
    "ranenv_ppo_slices_spread_bytes": (C.c_int, [C.POINTER(Mlp), C.POINTER(Mlp), C.POINTER(Mlp), C.POINTER(Mlp), _I32, _I32, _I32, C.POINTER(C.c_int64)]),
    "ranenv_ppo_slices_spread_plan": (C.c_int, [_I32, _I32, C.POINTER(_I32), _I32, _I32, _I32, C.POINTER(C.c_int64), C.POINTER(_I32), C.POINTER(C.c_int64)]),
    "ranenv_ppo_bind_spread_bfloat": (C.c_int, [_P, _I32, _P]),
    "ranenv_ppo_spread_bfloat_bytes": (C.c_int, [C.POINTER(Mlp), C.POINTER(Mlp), _I32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_ppo_update_slices": (C.c_int, [_P, _I32, C.POINTER(Trajectory), C.POINTER(PpoHparams), _P, _I32, _P, C.POINTER(C.c_int32), _P, _P, _P]),
    "ranenv_get_slice_net_weights": (C.c_int, [_P, _I32, _I32, C.POINTER(Mlp), _P]),
    "ranenv_ppo_slice_state": (C.c_int, [_P, _I32, _I32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "ranenv_ppo_bind_head": (C.c_int, [_P, _P]),
    "ranenv_ppo_update_head": (C.c_int, [_P, _I32, C.POINTER(HeadTrajectory), C.POINTER(PpoHparams), _P, _I32, _I32, _P, _P, _P]),
    "ranenv_ppo_head_layout": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_ppo_head_state": (C.c_int, [_P, _I32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "ranenv_get_head_net_weights": (C.c_int, [_P, _I32, C.POINTER(Mlp), _P]),
    "ranenv_get_head_log_std": (C.c_int, [_P, _P, _P]),
    "ranenv_ppo_bind_head_spread": (C.c_int, [_P, _I32, _P]),
    "ranenv_ppo_head_spread_bytes": (C.c_int, [C.POINTER(Mlp), C.POINTER(Mlp), _I32, _I32, C.POINTER(C.c_int64)]),
    "ranenv_sac_bind": (C.c_int, [_P, _F64, _I32, _F64, _I32, _P]),
    "ranenv_sac_update": (C.c_int, [_P, _I32, _I32, _I64, _P, _P, _P, _P, _P, _F64, _F64, _F64, C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    "ranenv_sac_layout": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ranenv_sac_lds_bytes": (C.c_int, [C.POINTER(Mlp), C.POINTER(Mlp), C.POINTER(C.c_int64)]),
    "ranenv_sac_state": (C.c_int, [_P, _I32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "ranenv_get_sac_net_weights": (C.c_int, [_P, _I32, C.POINTER(Mlp), _P]),
    "ranenv_get_sac_log_ent_coef": (C.c_int, [_P, _P, _P]),
}
POPULATION_MAX = 64
POPULATION_ROLES = {"inter": 0, "intra": 1, "v_inter": 2, "v_intra": 3}
EXPORTS = tuple(FUNCTIONS)


_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raises if it was not built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime; it has to be in the process before this library's
    # DT_NEEDED libamdhip64 is resolved, or two runtimes end up loaded and the second sees no GPU.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RanEnvError(
            f"{LIB_PATH} is missing: build it with `python -m intent_radio_sched_multi_slice_amd.csrc.build` "
            "(or __graft_entry__.build()). The env step has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in FUNCTIONS.items():
        if not hasattr(lib, name):
            raise RanEnvError(f"{LIB_PATH} does not export {name}")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.ranenv_abi_version() != ABI_VERSION:
        raise RanEnvError(f"ABI mismatch: library {lib.ranenv_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(lib, handle, status: int, what: str) -> None:
    if status != 0:
        msg = lib.ranenv_last_error(handle)
        raise RanEnvError(f"{what} failed ({status}): {msg.decode() if msg else 'unknown error'}")
