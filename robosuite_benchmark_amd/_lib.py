"""ctypes binding of libsac_hip.so (the C ABI of include/sac_hip.h).

There is NO CPU fallback: if the shared library is missing this module raises, and every
handle constructor raises when no MI355X is visible."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsac_hip.so")

SAC_DIAG_N = 32
ACT_MAX_ROWS = 1024              # rows per member of one sac_policy_act_device / sac_policy_act_many call
DIAG_NAMES = [
    "QF1 Loss", "QF2 Loss", "Policy Loss", "Actor Loss",
    "Q1 Predictions Mean", "Q1 Predictions Std", "Q1 Predictions Max", "Q1 Predictions Min",
    "Q2 Predictions Mean", "Q2 Predictions Std", "Q2 Predictions Max", "Q2 Predictions Min",
    "Q Targets Mean", "Q Targets Std", "Q Targets Max", "Q Targets Min",
    "Log Pis Mean", "Log Pis Std", "Log Pis Max", "Log Pis Min",
    "Policy mu Mean", "Policy mu Std", "Policy mu Max", "Policy mu Min",
    "Policy log std Mean", "Policy log std Std", "Policy log std Max", "Policy log std Min",
    "Alpha", "Alpha Loss",
]
NET_IDS = {"policy": 0, "qf1": 1, "qf2": 2, "target_qf1": 3, "target_qf2": 4}
TD3_NET_IDS = dict(NET_IDS, target_policy=5)
# the Q networks sac_q_values evaluates: name -> SAC_Q_* bit (1 << (SAC_NET_* - 1))
Q_NET_BITS = {"qf1": 1, "qf2": 2, "target_qf1": 4, "target_qf2": 8}


def q_net_mask(nets):
    """(mask, rows) of a selection of Q networks given by name, e.g. ("qf2", "qf1"): the SAC_Q_* mask sac_q_values takes,
    and for each name as given its row in the library's output (the selected nets in ascending SAC_NET_* order)."""
    names = [nets] if isinstance(nets, str) else list(nets)
    if not names:
        raise ValueError("q_values needs at least one Q network")
    for name in names:
        if name not in Q_NET_BITS:
            raise ValueError(f"unknown Q network {name!r}: one of {tuple(Q_NET_BITS)}")
    if len(set(names)) != len(names):
        raise ValueError(f"a Q network is named twice in {tuple(names)}")
    mask = sum(Q_NET_BITS[name] for name in names)
    order = sorted(names, key=Q_NET_BITS.get)
    return mask, [order.index(name) for name in names]


class SacConfig(C.Structure):
    _fields_ = [
        ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("hidden", C.c_int32), ("batch", C.c_int32),
        ("discount", C.c_float), ("reward_scale", C.c_float), ("policy_lr", C.c_float), ("qf_lr", C.c_float),
        ("soft_target_tau", C.c_float), ("target_update_period", C.c_int32),
        ("use_automatic_entropy_tuning", C.c_int32), ("target_entropy", C.c_float),
        ("noise_seed", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_int32),
        ("policy_hidden", C.c_int32 * 2), ("qf_hidden", C.c_int32 * 2),
    ]


class Td3Config(C.Structure):
    _fields_ = [
        ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("hidden", C.c_int32), ("batch", C.c_int32),
        ("discount", C.c_float), ("reward_scale", C.c_float), ("policy_learning_rate", C.c_float),
        ("qf_learning_rate", C.c_float), ("tau", C.c_float), ("target_policy_noise", C.c_float),
        ("target_policy_noise_clip", C.c_float), ("policy_and_target_update_period", C.c_int32),
        ("noise_seed", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_int32),
        ("policy_hidden", C.c_int32 * 2), ("qf_hidden", C.c_int32 * 2),
    ]


# the per-row columns of sac_evaluate (SAC_EVAL_*: the rows of sac_eval_io_t.rows, in this order)
EVAL_ROWS = ["q1", "q2", "q1_new", "q2_new", "tq1", "tq2", "log_pi", "log_pi_next", "y"]
EVAL_ARRAYS = ["mu", "log_std", "a_new", "a_next"]      # its (n, A) outputs


class SacEvalIO(C.Structure):
    """sac_eval_io_t"""
    _fields_ = [(k, C.c_void_p) for k in ("obs", "act", "rew", "term", "next_obs", "eps", "eps_next", "rows",
                                          "mu", "log_std", "a_new", "a_next")] + [("alpha", C.c_float)]


# the per-row columns of td3_evaluate (TD3_EVAL_*: the rows of td3_eval_io_t.rows, in this order) and its (n, A) outputs
TD3_EVAL_ROWS = ["q1", "q2", "q_pi", "tq1", "tq2", "y"]
TD3_EVAL_ARRAYS = ["a_pi", "a_target", "a_smooth"]


class Td3EvalIO(C.Structure):
    """td3_eval_io_t"""
    _fields_ = [(k, C.c_void_p) for k in ("obs", "act", "rew", "term", "next_obs", "eps", "rows",
                                          "a_pi", "a_target", "a_smooth")]


# the moment records of sac_evaluate_stats_many (SAC_EVAL_M_*: sac_eval_stats_t.m, in this order)
EVAL_MOMENTS = ["q1", "q2", "y", "log_pi", "mu", "log_std", "td1", "td2", "policy"]
EVAL_MOMENT_FIELDS = ["count", "sum", "m2", "sumsq", "max", "min"]


class SacEvalMoment(C.Structure):
    """sac_eval_moment_t"""
    _fields_ = [(k, C.c_double) for k in EVAL_MOMENT_FIELDS]


class SacEvalSrc(C.Structure):
    """sac_eval_src_t"""
    _fields_ = [("buf", C.c_void_p), ("idx", C.c_void_p)]


class SacEvalStats(C.Structure):
    """sac_eval_stats_t"""
    _fields_ = [("m", SacEvalMoment * len(EVAL_MOMENTS)), ("alpha", C.c_double), ("log_alpha", C.c_double)]


# the moment records of td3_evaluate_stats_many (TD3_EVAL_M_*: td3_eval_stats_t.m, in this order)
TD3_EVAL_MOMENTS = ["q1", "q2", "y", "q_pi", "a_pi", "td1", "td2", "bellman1", "bellman2"]


class Td3EvalStats(C.Structure):
    """td3_eval_stats_t"""
    _fields_ = [("m", SacEvalMoment * len(TD3_EVAL_MOMENTS))]


# the per-unit records of sac_unit_moments_* (SAC_UNIT_*: the arrays of one hidden layer's record, in this order)
UNIT_FIELDS = ("sum", "sumsq", "active", "max")
UNIT_NET_BITS = {name: 1 << k for name, k in TD3_NET_IDS.items()}      # name -> bit SAC_NET_* of sac_units_io_t.nets
UNIT_Q_NETS = ("qf1", "qf2", "target_qf1", "target_qf2")               # the nets that read cat(obs, act)


class SacUnitsIO(C.Structure):
    """sac_units_io_t"""
    _fields_ = [("obs", C.c_void_p), ("act", C.c_void_p), ("nets", C.c_uint32), ("reserved", C.c_uint32),
                ("moments", C.c_void_p), ("activations", C.c_void_p)]


# the per-tensor records of sac_param_moments* (SAC_PARAM_*: the float64 values of one tensor's record, in this order)
PARAM_FIELDS = ("sum", "sumsq", "absmax", "nonfinite", "m_sumsq", "m_absmax", "v_sum", "v_max", "gap_sumsq")
PARAMS_OPT, PARAMS_GAP = 1, 2                                          # sac_params_io_t.flags
PARAM_MAX_TENSORS = 18


class SacParamsIO(C.Structure):
    """sac_params_io_t"""
    _fields_ = [("nets", C.c_uint32), ("flags", C.c_uint32), ("moments", C.c_void_p)]


RECYCLE_OPT = 1                                                        # sac_recycle_io_t.flags
RECYCLE_NETS = ("policy", "qf1", "qf2")                                # the nets sac_recycle_units writes: the trained ones


class SacRecycleIO(C.Structure):
    """sac_recycle_io_t"""
    _fields_ = [("nets", C.c_uint32), ("flags", C.c_uint32), ("counts", C.c_void_p), ("units", C.c_void_p),
                ("fresh", C.c_void_p)]


PERTURB_OPT, PERTURB_TARGETS = 1, 2                                    # sac_perturb_io_t.flags


class SacPerturbIO(C.Structure):
    """sac_perturb_io_t"""
    _fields_ = [("nets", C.c_uint32), ("flags", C.c_uint32), ("shrink", C.c_float), ("perturb", C.c_float),
                ("seed", C.c_uint64), ("draw", C.c_uint64), ("init_w", C.c_float * 3), ("b_init", C.c_float * 3)]


TD3_DIAG_NAMES = DIAG_NAMES[:16] + [f"Bellman Errors {i} {s}" for i in (1, 2) for s in ("Mean", "Std", "Max", "Min")] + [
    f"Policy Action {s}" for s in ("Mean", "Std", "Max", "Min")]

# every symbol include/sac_hip.h declares: (restype, argtypes)
_P = C.c_void_p
_F = C.POINTER(C.c_float)
SYMBOLS = {
    "sac_last_error": (C.c_char_p, []),
    "sac_device_count": (C.c_int, []),
    "sac_version": (C.c_char_p, []),
    "sac_buffer_create": (C.c_int, [C.POINTER(_P), C.c_int64, C.c_int, C.c_int, C.c_int]),
    "sac_buffer_destroy": (C.c_int, [_P]),
    "sac_buffer_add": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P]),
    "sac_buffer_add_f64": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P]),
    "sac_buffer_ingest_pending": (C.c_int, [_P]),
    "sac_buffer_ingest_wait": (C.c_int, [_P]),
    "sac_buffer_size": (C.c_int64, [_P]),
    "sac_buffer_top": (C.c_int64, [_P]),
    "sac_buffer_capacity": (C.c_int64, [_P]),
    "sac_buffer_rows_written": (C.c_int64, [_P]),
    "sac_buffer_read": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    "sac_buffer_set_cursor": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "sac_rng_seed": (C.c_int, [_P, C.c_uint32]),
    "sac_rng_get_state": (C.c_int, [_P, _P, C.POINTER(C.c_int32)]),
    "sac_rng_set_state": (C.c_int, [_P, _P, C.c_int32]),
    "sac_rng_bind_host": (C.c_int, [_P, _P, _P]),
    "sac_sample_indices": (C.c_int, [_P, C.c_int, C.c_int64, _P]),
    "sac_random_batch": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "sac_random_batch_device": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "sac_read_batch_device": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "sac_gather": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "sac_sample_gather_device": (C.c_int, [_P, C.c_int, C.c_int64, _P]),
    "sac_read_slot": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "sac_read_slot_images": (C.c_int, [_P, C.c_int, C.c_int64, _P, _P]),
    "sac_trainer_create": (C.c_int, [C.POINTER(_P), C.POINTER(SacConfig)]),
    "sac_trainer_create_mlp": (C.c_int, [C.POINTER(_P), C.POINTER(SacConfig), _P, C.c_int32, _P, C.c_int32]),
    "td3_trainer_create": (C.c_int, [C.POINTER(_P), C.POINTER(Td3Config)]),
    "td3_trainer_create_mlp": (C.c_int, [C.POINTER(_P), C.POINTER(Td3Config), _P, C.c_int32, _P, C.c_int32]),
    "sac_trainer_destroy": (C.c_int, [_P]),
    "sac_param_count": (C.c_int64, [_P, C.c_int]),
    "sac_set_params": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "sac_get_params": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "sac_set_opt_state": (C.c_int, [_P, C.c_int, _P, _P, C.c_int64]),
    "sac_get_opt_state": (C.c_int, [_P, C.c_int, _P, _P, C.c_int64]),
    "sac_set_scalars": (C.c_int, [_P, _P]),
    "sac_get_scalars": (C.c_int, [_P, _P]),
    "sac_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sac_step_device": (C.c_int, [_P, _P, C.c_int64, _P]),
    "sac_train_loop": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "sac_sync": (C.c_int, [_P]),
    "sac_trainer_is_fused": (C.c_int, [_P]),
    "sac_trainer_step_kind": (C.c_int, [_P]),
    "sac_last_loop_ms": (C.c_int, [_P, _F, _F, _F, _F]),
    "sac_profile_loop": (C.c_int, [_P, _P, C.c_int64, _P]),
    "sac_measure_peaks": (C.c_int, [C.c_int, _F]),
    "sac_buffer_set_xcd": (C.c_int, [_P, C.c_int]),
    "sac_trainer_set_xcd": (C.c_int, [_P, C.c_int]),
    "sac_buffer_set_xcd_mask": (C.c_int, [_P, C.c_uint]),
    "sac_trainer_set_xcd_mask": (C.c_int, [_P, C.c_uint]),
    "sac_debug_fetch": (C.c_int64, [_P, C.c_char_p, _P, C.c_int64]),
    "sac_debug_set_launch_number": (C.c_int, [_P, C.c_uint32]),
    "sac_policy_mirror": (C.c_int, [_P]),
    "sac_policy_act": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "sac_policy_act_device": (C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P]),
    "sac_policy_act_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "sac_policy_act_general": (C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P]),
    "sac_policy_act_general_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "sac_q_values": (C.c_int, [_P, C.c_int64, _P, _P, C.c_uint32, _P]),
    "sac_q_values_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "sac_q_values_general": (C.c_int, [_P, C.c_int64, _P, _P, C.c_uint32, _P]),
    "sac_q_values_general_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "sac_evaluate": (C.c_int, [_P, C.c_int64, _P]),
    "sac_evaluate_many": (C.c_int, [_P, C.c_int, _P, _P]),
    "sac_evaluate_general": (C.c_int, [_P, C.c_int64, _P]),
    "sac_evaluate_general_many": (C.c_int, [_P, C.c_int, _P, _P]),
    "sac_evaluate_stats_many": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "sac_evaluate_general_stats_many": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "sac_evaluate_replay_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "sac_evaluate_replay_general_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "td3_evaluate": (C.c_int, [_P, C.c_int64, _P]),
    "td3_evaluate_many": (C.c_int, [_P, C.c_int, _P, _P]),
    "td3_evaluate_general": (C.c_int, [_P, C.c_int64, _P]),
    "td3_evaluate_general_many": (C.c_int, [_P, C.c_int, _P, _P]),
    "td3_evaluate_stats_many": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "td3_evaluate_general_stats_many": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "td3_evaluate_replay_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "td3_evaluate_replay_general_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "sac_unit_moments": (C.c_int, [_P, C.c_int64, _P]),
    "sac_unit_moments_many": (C.c_int, [_P, C.c_int, _P, _P]),
    "sac_unit_moments_general": (C.c_int, [_P, C.c_int64, _P]),
    "sac_unit_moments_general_many": (C.c_int, [_P, C.c_int, _P, _P]),
    "sac_param_tensors": (C.c_int, [_P, C.c_int, _P]),
    "sac_param_moments": (C.c_int, [_P, _P]),
    "sac_param_moments_many": (C.c_int, [_P, C.c_int, _P]),
    "sac_recycle_units": (C.c_int, [_P, _P]),
    "sac_recycle_units_many": (C.c_int, [_P, C.c_int, _P]),
    "sac_shrink_perturb": (C.c_int, [_P, _P]),
    "sac_shrink_perturb_many": (C.c_int, [_P, C.c_int, _P]),
    "sac_group_create": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "td3_group_create": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "sac_group_create_mixed": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "td3_group_create_mixed": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "sac_group_create_mlp": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "td3_group_create_mlp": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "sac_group_create_arch": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "td3_group_create_arch": (C.c_int, [C.POINTER(_P), _P, C.c_int]),
    "sac_group_stage_count": (C.c_int, [_P]),
    "sac_group_destroy": (C.c_int, [_P]),
    "sac_group_train_loop": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "sac_actor_create": (C.c_int, [C.POINTER(_P), _P, C.c_int, _P]),
    "sac_actor_destroy": (C.c_int, [_P]),
    "sac_actor_arrays": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "sac_actor_act": (C.c_int, [_P, _P, _P]),
    "sac_gactor_create": (C.c_int, [C.POINTER(_P), _P, C.c_int, _P]),
    "sac_gactor_destroy": (C.c_int, [_P]),
    "sac_gactor_arrays": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "sac_gactor_act": (C.c_int, [_P, _P, _P]),
}

_lib = None


def load():
    """Load libsac_hip.so, binding every declared symbol.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m robosuite_benchmark_amd.build` "
            "(hipcc --offload-arch=gfx950).  robosuite_benchmark_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().sac_last_error().decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc < 0:
        raise RuntimeError(f"{what} failed: {last_error()}")
    return rc


def device_count() -> int:
    return int(load().sac_device_count())


def ptr(a):
    """void* of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)
