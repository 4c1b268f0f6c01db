"""ctypes binding of libv21.so (C ABI: include/v21.h).

The product path has NO CPU fallback: if the HIP library is missing or no GPU is
visible, the first call that needs the engine raises ``EngineUnavailable``.  Loading
the library and listing its symbols works without a GPU (used by the CPU test suite).
"""
import ctypes as C
import os
import threading
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("V21_LIB") or os.path.join(HERE, "libv21.so")

PREC_F32, PREC_F16, PREC_BF16 = 0, 1, 2
PRECISIONS = {"f32": PREC_F32, "fp32": PREC_F32, "float32": PREC_F32,
              "f16": PREC_F16, "fp16": PREC_F16, "float16": PREC_F16,
              "bf16": PREC_BF16, "bfloat16": PREC_BF16}
ACT_LINEAR, ACT_RELU, ACT_GAUSS = 0, 1, 2
ACT_TANH, ACT_SIGMOID, ACT_ELU, ACT_SOFTPLUS = 3, 4, 5, 6  # include/v21.h: Keras' definitions, hidden layers
FWD_IN_TRANSFORM, FWD_OUT_TRANSFORM, FWD_FORCE_GENERIC, FWD_NO_SMALL, FWD_FORCE_CHAIN, FWD_FORCE_JIT = 1, 2, 4, 8, 16, 32
COMM_ID_BYTES = 128


class EngineUnavailable(RuntimeError):
    """libv21.so cannot be loaded or no MI355X is visible."""


class EngineError(RuntimeError):
    """A v21_* call returned a negative status."""


class AffineIn(C.Structure):
    _fields_ = [("n", C.c_int32), ("log_mask", C.c_int32 * 8), ("zero_floor", C.c_double * 8),
                ("lo", C.c_double * 8), ("span", C.c_double * 8)]


class AffineOut(C.Structure):
    _fields_ = [("std", C.c_float), ("mean", C.POINTER(C.c_float)), ("n", C.c_int32)]


_HOST_AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_size_t)


class CommHostOps(C.Structure):
    _fields_ = [("user", C.c_void_p), ("allreduce_sum_f32", _HOST_AR), ("reduce_scatter_sum_f32", _HOST_AR),
                ("allgather_f32", _HOST_AR)]


class Adam(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class FitOpts(C.Structure):
    """v21_fit_opts (include/v21_types.h)"""
    _fields_ = [("max_iter", C.c_int), ("lambda0", C.c_double), ("xtol", C.c_double), ("check_every", C.c_int)]


class MapOpts(C.Structure):
    """v21_map_opts (include/v21_types.h)"""
    _fields_ = [("use_prior", C.c_int), ("hold", C.c_int * 8)]


MAP_OUTPUTS = ("lnp", "laplace", "prec_u")


class MapOut(C.Structure):
    """v21_map_out (include/v21_types.h): host or device addresses, NULL = not asked for"""
    _fields_ = [(k, C.c_void_p) for k in MAP_OUTPUTS]


FIT_DEFAULTS = {"max_iter": 50, "lambda0": 1e-3, "xtol": 1e-7, "check_every": 8}
FIT_STATUS = {0: "iteration limit", 1: "converged", 2: "no improving step", 3: "no information"}


class SampleOpts(C.Structure):
    """v21_sample_opts (include/v21_types.h)"""
    _fields_ = [("n_steps", C.c_int), ("n_warmup", C.c_int), ("thin", C.c_int), ("eps0", C.c_double), ("ridge", C.c_double),
                ("target_accept", C.c_double), ("seed", C.c_ulonglong), ("chain0", C.c_longlong), ("step0", C.c_longlong)]


SAMPLE_DEFAULTS = {"n_steps": 1000, "n_warmup": 200, "thin": 1, "eps0": 1.0, "ridge": 1.0, "target_accept": 0.574, "seed": 0,
                   "chain0": 0, "step0": 0}
SAMPLE_OUTPUTS = ("samples", "samples_lnl", "x_last", "lnl_last", "eps_last", "accept_rate", "mean_u", "cov_u", "last_prop_u",
                  "last_log_alpha")


class SampleOut(C.Structure):
    """v21_sample_out (include/v21_types.h): host or device addresses, NULL = not asked for"""
    _fields_ = [(k, C.c_void_p) for k in SAMPLE_OUTPUTS]


class TemperOpts(C.Structure):
    """v21_temper_opts (include/v21_types.h)"""
    _fields_ = [("n_temps", C.c_int), ("betas", C.c_double * 32), ("swap_every", C.c_int)]


TEMPER_OUTPUTS = ("mean_lnl", "var_lnl", "swap_accept")


class TemperOut(C.Structure):
    """v21_temper_out (include/v21_types.h): host or device addresses, NULL = not asked for"""
    _fields_ = [(k, C.c_void_p) for k in TEMPER_OUTPUTS]


class EnsembleOpts(C.Structure):
    """v21_ensemble_opts (include/v21_types.h)"""
    _fields_ = [("n_walkers", C.c_int), ("a", C.c_double), ("n_steps", C.c_int), ("n_warmup", C.c_int), ("thin", C.c_int),
                ("seed", C.c_ulonglong), ("chain0", C.c_longlong), ("step0", C.c_longlong)]


ENSEMBLE_DEFAULTS = {"n_walkers": 64, "a": 2.0, "n_steps": 1000, "n_warmup": 500, "thin": 1, "seed": 0, "chain0": 0, "step0": 0}
ENSEMBLE_OUTPUTS = ("samples", "samples_lnl", "x_last", "lnl_last", "accept_rate", "mean_u", "cov_u", "last_prop_u", "last_log_alpha",
                    "last_partner")
ENSEMBLE_MAX_WALKERS = 512


class EnsembleOut(C.Structure):
    """v21_ensemble_out (include/v21_types.h): host or device addresses, NULL = not asked for"""
    _fields_ = [(k, C.c_void_p) for k in ENSEMBLE_OUTPUTS]


class NestedOpts(C.Structure):
    """v21_nested_opts (include/v21_types.h)"""
    _fields_ = [("n_live", C.c_int), ("n_repeats", C.c_int), ("n_iter", C.c_int), ("gamma", C.c_double), ("seed", C.c_ulonglong),
                ("iter0", C.c_longlong), ("chain0", C.c_longlong)]


NESTED_DEFAULTS = {"n_live": 256, "n_repeats": 0, "n_iter": 100, "gamma": 0.0, "seed": 0, "iter0": 0, "chain0": 0}
NESTED_OUTPUTS = ("dead_u", "dead_lnl", "lstar", "live_u", "live_lnl", "accept_rate", "last_partner", "last_prop_u")
NESTED_MIN_LIVE, NESTED_MAX_LIVE = 16, 512


class NestedOut(C.Structure):
    """v21_nested_out (include/v21_types.h): host or device addresses, NULL = not asked for"""
    _fields_ = [(k, C.c_void_p) for k in NESTED_OUTPUTS]


_P = C.c_void_p
_F = C.POINTER(C.c_float)
# name -> (restype, argtypes); every symbol include/v21.h declares
SIGNATURES = {
    "v21_last_error": (C.c_char_p, []),
    "v21_version": (C.c_int, []),
    "v21_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "v21_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "v21_ctx_destroy": (C.c_int, [_P]),
    "v21_ctx_sync": (C.c_int, [_P]),
    "v21_ctx_set_stream": (C.c_int, [_P, _P]),
    "v21_ctx_get_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "v21_malloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "v21_free": (C.c_int, [_P, _P]),
    "v21_memcpy_h2d": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "v21_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "v21_memset": (C.c_int, [_P, _P, C.c_int, C.c_size_t]),
    "v21_event_create": (C.c_int, [_P, C.POINTER(_P)]),
    "v21_event_destroy": (C.c_int, [_P, _P]),
    "v21_event_record": (C.c_int, [_P, _P]),
    "v21_event_elapsed_ms": (C.c_int, [_P, _P, _P, C.POINTER(C.c_float)]),
    "v21_mlp_create": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_P)]),
    "v21_mlp_destroy": (C.c_int, [_P]),
    "v21_mlp_num_params": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "v21_mlp_set_weights": (C.c_int, [_P, _F, C.c_size_t]),
    "v21_mlp_get_weights": (C.c_int, [_P, _F, C.c_size_t]),
    "v21_mlp_set_input_transform": (C.c_int, [_P, C.POINTER(AffineIn)]),
    "v21_mlp_set_output_transform": (C.c_int, [_P, C.POINTER(AffineOut)]),
    "v21_mlp_has_fused": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "v21_mlp_jit": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "v21_jit_prebuild": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_char_p]),
    "v21_mlp_forward": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int, C.c_int]),
    "v21_mlp_forward_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int, C.c_int]),
    "v21_trainer_create": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "v21_trainer_destroy": (C.c_int, [_P]),
    "v21_trainer_set_adam": (C.c_int, [_P, C.POINTER(Adam)]),
    "v21_trainer_set_lr": (C.c_int, [_P, C.c_float]),
    "v21_trainer_get_lr": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "v21_trainer_set_data": (C.c_int, [_P, C.c_int, _F, _F, _F, C.c_int64]),
    "v21_trainer_run_epoch": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double)]),
    "v21_trainer_eval": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "v21_trainer_step_dev": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int]),
    "v21_trainer_last_step_loss": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "v21_trainer_get_state": (C.c_int, [_P, C.POINTER(C.c_int64), _F, _F, C.c_size_t]),
    "v21_trainer_set_state": (C.c_int, [_P, C.c_int64, _F, _F, C.c_size_t]),
    "v21_trainer_get_grad": (C.c_int, [_P, _F, C.c_size_t]),
    "v21_trainer_use_graph": (C.c_int, [_P, C.c_int]),
    "v21_debug_poison_lds": (C.c_int, [_P, C.c_uint32]),
    "v21_debug_check_chain_jobs": (C.c_int, [_P, C.c_longlong, C.c_longlong]),
    "v21_debug_trainer_counters": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "v21_route_forward": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "v21_route_train": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "v21_trainer_jit": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "v21_mlp_last_route": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "v21_mlp_jacobian": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, _F, C.c_int, C.c_int]),
    "v21_mlp_jacobian_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, C.c_int, C.c_int]),
    "v21_mlp_set_likelihood": (C.c_int, [_P, _F, _F, C.c_int32]),
    "v21_mlp_loglike": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, _F, C.c_int, C.c_int]),
    "v21_mlp_loglike_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int]),
    "v21_route_jacobian": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int)]),
    "v21_route_jacobian_rt": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "v21_mlp_jit_jacobian": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "v21_mlp_last_jac_route": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "v21_mlp_loglike_fwd": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int64, _F, C.c_int, C.c_int]),
    "v21_mlp_loglike_fwd_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, C.c_int, C.c_int]),
    "v21_route_loglike_fwd": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                        C.POINTER(C.c_int)]),
    "v21_route_loglike_fwd_rt": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                           C.POINTER(C.c_int)]),
    "v21_mlp_jit_loglike": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "v21_mlp_last_lnl_route": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "v21_mlp_fisher": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, _F, _F, C.c_int, C.c_int]),
    "v21_mlp_fisher_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int, C.c_int]),
    "v21_mlp_fit": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int64, C.POINTER(FitOpts), _P, _F, _F, _F, C.POINTER(C.c_int32),
                              C.c_int, C.c_int]),
    "v21_mlp_fit_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(FitOpts), _P, _P, _P, _P, _P, C.c_int, C.c_int]),
    "v21_mlp_fit_map": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int64, C.POINTER(FitOpts), C.POINTER(MapOpts), _P, _F, _F, _F,
                                  C.POINTER(C.c_int32), C.POINTER(MapOut), C.c_int, C.c_int]),
    "v21_mlp_fit_map_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(FitOpts), C.POINTER(MapOpts), _P, _P, _P, _P,
                                      _P, C.POINTER(MapOut), C.c_int, C.c_int]),
    "v21_mlp_sample": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int64, C.POINTER(SampleOpts), _P, C.POINTER(SampleOut),
                                 C.c_int, C.c_int]),
    "v21_mlp_sample_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(SampleOpts), _P, C.POINTER(SampleOut),
                                     C.c_int, C.c_int]),
    "v21_mlp_sample_tempered": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int64, C.POINTER(SampleOpts), C.POINTER(TemperOpts), _P,
                                          C.POINTER(SampleOut), C.POINTER(TemperOut), C.c_int, C.c_int]),
    "v21_mlp_sample_tempered_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(SampleOpts), C.POINTER(TemperOpts), _P,
                                              C.POINTER(SampleOut), C.POINTER(TemperOut), C.c_int, C.c_int]),
    "v21_mlp_sample_ensemble": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int64, C.POINTER(EnsembleOpts), C.POINTER(EnsembleOut),
                                          C.c_int, C.c_int]),
    "v21_mlp_sample_ensemble_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(EnsembleOpts), C.POINTER(EnsembleOut),
                                              C.c_int, C.c_int]),
    "v21_route_ensemble": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "v21_route_ensemble_rt": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "v21_mlp_sample_nested": (C.c_int, [_P, _P, C.c_int, C.c_int64, _F, C.c_int64, C.POINTER(NestedOpts), C.POINTER(NestedOut), C.c_int,
                                        C.c_int]),
    "v21_mlp_sample_nested_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(NestedOpts), C.POINTER(NestedOut),
                                            C.c_int, C.c_int]),
    "v21_route_nested": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "v21_nuisance_whiten": (C.c_int, [C.POINTER(C.c_double), _F, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "v21_mlp_set_nuisance": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int32, C.c_int32]),
    "v21_mlp_set_prior": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32]),
    "v21_mlp_set_hold": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32]),
    "v21_mlp_nuisance_info": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "v21_mlp_nuisance_coef": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.POINTER(C.c_double), C.c_int, C.c_int]),
    "v21_trainer_last_route": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "v21_route_name": (C.c_char_p, [C.c_int, C.c_int]),
    "v21_trainer_get_data_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    "v21_debug_clock_probe_start": (C.c_int, [_P, C.c_double, C.c_double]),
    "v21_debug_forward_clocked": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "v21_debug_clock_probe_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "v21_trainer_set_vae": (C.c_int, [_P, C.c_float, C.c_int, C.c_uint64]),
    "v21_trainer_enable_stamps": (C.c_int, [_P, C.c_int]),
    "v21_trainer_chain_stamps": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "v21_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "v21_host_free": (C.c_int, [_P, _P]),
    "v21_sweep_create": (C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    "v21_sweep_destroy": (C.c_int, [_P]),
    "v21_sweep_run_epoch": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double)]),
    "v21_joint_create": (C.c_int, [_P, _P, C.c_int, C.POINTER(_P)]),
    "v21_joint_destroy": (C.c_int, [_P]),
    "v21_joint_run_epoch": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double)]),
    "v21_joint_eval": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "v21_comm_get_unique_id": (C.c_int, [_P, _P]),
    "v21_comm_init": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "v21_comm_init_host": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(CommHostOps)]),
    "v21_comm_destroy": (C.c_int, [_P]),
    "v21_comm_init_null": (C.c_int, [_P, C.c_int, C.c_int]),
    "v21_comm_set_buckets": (C.c_int, [_P, C.c_int]),
    "v21_trainer_phase_timing": (C.c_int, [_P, C.c_int, C.c_int]),
    "v21_trainer_phase_times": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "v21_comm_set_sharded": (C.c_int, [_P, C.c_int]),
    "v21_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "v21_comm_allreduce_f32": (C.c_int, [_P, _P, C.c_size_t]),
    "v21_comm_reduce_scatter_f32": (C.c_int, [_P, _P, C.c_size_t]),
    "v21_comm_allgather_f32": (C.c_int, [_P, _P, C.c_size_t]),
}

# ---- routes (include/v21.h: v21_route_*; csrc/routes.h): the names the tests and INTEGRATION.md section 6 use
FWD_ROUTES = {1: "small", 2: "fused", 3: "fused_rt", 4: "table", 5: "generic"}
TRAIN_FWD_ROUTES = {1: "per_layer", 2: "chain16", 3: "fused128", 4: "fused64", 5: "chain32", 6: "chain32s_8", 7: "chain32s_4"}
TRAIN_UPD_ROUTES = {1: "per_layer", 2: "dw16_adam", 3: "dw16_splitk", 4: "dwadam32", 5: "nt_dwadam", 6: "nt_sliced"}


def route_forward(dims, act, precision, n, flags=0, rt_ready=False):
    """The route v21_mlp_forward_dev takes for n rows of this stack (pure host logic: no GPU).  -> name of FWD_ROUTES."""
    r = C.c_int(0)
    check(load_library().v21_route_forward(*_layers(dims, act), precision_id(precision), int(n), int(flags), 1 if rt_ready else 0,
                                           C.byref(r)))
    return FWD_ROUTES[r.value]


JAC_ROUTES = {1: "fused", 2: "generic", 3: "fused_rt"}


def route_jacobian(dims, act, precision, n, flags=0):
    """The route v21_mlp_jacobian / v21_mlp_loglike take for this stack (pure host logic: no GPU).  -> name of JAC_ROUTES."""
    r = C.c_int(0)
    check(load_library().v21_route_jacobian(*_layers(dims, act), precision_id(precision), int(n), int(flags), C.byref(r)))
    return JAC_ROUTES[r.value]


def route_jacobian_rt(dims, act, precision, flags=0):
    """The route of a handle that asked for its run-time Jacobian kernel (Stack.jit_jacobian) and has it: "fused_rt" where
    the stack can have one, else route_jacobian's answer (pure host logic: no GPU).  -> name of JAC_ROUTES."""
    r = C.c_int(0)
    check(load_library().v21_route_jacobian_rt(*_layers(dims, act), precision_id(precision), int(flags), C.byref(r)))
    return JAC_ROUTES[r.value]


LNL_ROUTES = {1: "fused", 2: "two_launch"}   # what a route query without a handle can answer
# ... and what a handle can record (last_lnl_route) and the _rt queries answer: route 3 is the fused kernel instantiated for
# the handle's own stack at run time, only for a handle that asked (Stack.jit_loglike)
LNL_ROUTES_RT = {1: "fused", 2: "two_launch", 3: "fused_rt"}


def route_loglike_fwd(dims, act, precision, n, n_data=0, n_modes=0, flags=0):
    """The route v21_mlp_loglike_fwd[_dev] takes for n rows of this stack against n_data data rows (0: the likelihood
    record) with n_modes nuisance modes (pure host logic: no GPU).  -> name of LNL_ROUTES."""
    r = C.c_int(0)
    check(load_library().v21_route_loglike_fwd(*_layers(dims, act), precision_id(precision), int(n), int(n_data), int(n_modes),
                                               int(flags), C.byref(r)))
    return LNL_ROUTES[r.value]


def route_loglike_fwd_rt(dims, act, precision, n, n_data=0, n_modes=0, flags=0):
    """route_loglike_fwd for a handle that asked for its run-time ln L kernel (Stack.jit_loglike) and has it: "fused_rt"
    where a compiled stack would say "fused" and this stack can have the kernel, else route_loglike_fwd's answer (pure
    host logic: no GPU).  -> name of LNL_ROUTES."""
    r = C.c_int(0)
    check(load_library().v21_route_loglike_fwd_rt(*_layers(dims, act), precision_id(precision), int(n), int(n_data), int(n_modes),
                                                  int(flags), C.byref(r)))
    return LNL_ROUTES_RT[r.value]


def route_ensemble_rt(dims, act, precision, n, n_walkers, n_data=0, n_modes=0, flags=0, host_form=False):
    """route_ensemble -- and, with n_live for n_walkers, route_nested -- for a handle that asked for its run-time ln L kernel
    and has it (pure host logic: no GPU).  -> (name of LNL_ROUTES, chunk rows)."""
    r, c = C.c_int(0), C.c_int64(0)
    check(load_library().v21_route_ensemble_rt(*_layers(dims, act), precision_id(precision), int(n), int(n_data), int(n_walkers),
                                               int(n_modes), int(flags), 1 if host_form else 0, C.byref(r), C.byref(c)))
    return LNL_ROUTES_RT[r.value], int(c.value)


def route_ensemble(dims, act, precision, n, n_walkers, n_data=0, n_modes=0, flags=0, host_form=False):
    """The route v21_mlp_sample_ensemble[_dev] takes for n rows in ensembles of n_walkers against n_data data rows (0: the
    likelihood record) with n_modes nuisance modes, and the rows of a host chunk (the _dev form: n) (pure host logic: no
    GPU; EngineError for the shapes the library refuses).  -> (name of LNL_ROUTES, chunk rows)."""
    r, c = C.c_int(0), C.c_int64(0)
    check(load_library().v21_route_ensemble(*_layers(dims, act), precision_id(precision), int(n), int(n_data), int(n_walkers),
                                            int(n_modes), int(flags), 1 if host_form else 0, C.byref(r), C.byref(c)))
    return LNL_ROUTES[r.value], int(c.value)


def route_nested(dims, act, precision, n, n_live, n_data=0, n_modes=0, flags=0, host_form=False):
    """The route v21_mlp_sample_nested[_dev] takes for n rows in runs of n_live live points against n_data data rows (0: the
    likelihood record) with n_modes nuisance modes, and the rows of a host chunk (the _dev form: n) (pure host logic: no
    GPU; EngineError for the shapes the library refuses).  -> (name of LNL_ROUTES, chunk rows)."""
    r, c = C.c_int(0), C.c_int64(0)
    check(load_library().v21_route_nested(*_layers(dims, act), precision_id(precision), int(n), int(n_data), int(n_live),
                                          int(n_modes), int(flags), 1 if host_form else 0, C.byref(r), C.byref(c)))
    return LNL_ROUTES[r.value], int(c.value)


def nuisance_whiten(basis, inv_var):
    """The W-orthonormalised nuisance basis (include/v21.h: v21_nuisance_whiten; pure host arithmetic: no GPU).  basis
    (K, out) float64, inv_var (out,) float32 -> (Q (K, out), R (K, K)) float64 with Q diag(inv_var) Q^T = I and
    sqrt(W) basis^T = sqrt(W) Q^T R; EngineError for a rank-deficient basis, K outside 1 .. 8, or too few weighted bins."""
    A = np.ascontiguousarray(basis, dtype=np.float64)
    w = np.ascontiguousarray(inv_var, dtype=np.float32).ravel()
    if A.ndim != 2 or A.shape[1] != w.size:
        raise ValueError("nuisance: basis must be (K, %d), got %r" % (w.size, np.shape(basis)))
    K, D = A.shape
    q, r = np.zeros((max(K, 1), D), np.float64), np.zeros((max(K, 1), max(K, 1)), np.float64)
    dp = C.POINTER(C.c_double)
    check(load_library().v21_nuisance_whiten(A.ctypes.data_as(dp), _fptr(w), K, D, q.ctypes.data_as(dp), r.ctypes.data_as(dp)))
    return q, r


def route_train(dims, act, precision, max_batch, rows, nranks=1, rt_ready=False):
    """The kernels one optimizer step of `rows` rows takes for a trainer created with max_batch on nranks ranks (pure host
    logic: no GPU; rt_ready: the run-time instantiated fused training kernel of a stack outside archs.h has arrived).
    -> (name of TRAIN_FWD_ROUTES, name of TRAIN_UPD_ROUTES)."""
    f, u = C.c_int(0), C.c_int(0)
    check(load_library().v21_route_train(*_layers(dims, act), precision_id(precision), int(max_batch), int(rows), int(nranks),
                                         1 if rt_ready else 0, C.byref(f), C.byref(u)))
    return TRAIN_FWD_ROUTES[f.value], TRAIN_UPD_ROUTES[u.value]


_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen libv21.so and attach prototypes.  Needs no GPU."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise EngineUnavailable(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C 21cmvae_amd/csrc)" % LIB_PATH)
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # missing libamdhip64 etc.
            raise EngineUnavailable("cannot load %s: %s" % (LIB_PATH, e)) from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
        return lib


def check(status):
    if status != 0:
        msg = load_library().v21_last_error()
        raise EngineError("v21 error %d: %s" % (status, msg.decode() if msg else "?"))


def precision_id(p):
    if isinstance(p, int):
        return p
    try:
        return PRECISIONS[str(p).lower()]
    except KeyError:
        raise ValueError("unknown precision %r (use f32, f16 or bf16)" % (p,)) from None


def _layers(dims, act):
    """A stack's layout as the C ABI takes it: (L, int[L + 1] widths, int[L] activations)."""
    L = len(act)
    return L, (C.c_int * (L + 1))(*[int(d) for d in dims]), (C.c_int * L)(*[int(a) for a in act])


def _row_table(perm, n_rows, who):
    """An epoch's row table as the C ABI takes it: a pointer to int32, contiguous, one entry per row of the training set (the
    library reads exactly that many entries from the pointer: a shorter array would be read past its end); None (the rows
    in order) stays None.  (The pointer keeps its array alive.)"""
    if perm is None:
        return None
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    if n_rows is not None and perm.shape != (n_rows,):
        raise ValueError("%s: the row table has shape %s, the training set has %d rows" % (who, perm.shape, n_rows))
    return perm.ctypes.data_as(C.POINTER(C.c_int32))


def _fptr(a):
    return a.ctypes.data_as(_F)


def _opt(a):
    """An optional pointer argument: a float32 numpy array -> float*, a device address -> void*, None / 0 -> NULL."""
    if isinstance(a, np.ndarray):
        return _fptr(a)
    return _P(a) if a else None


def _data_rows(what, data, n, dout):
    """The data matrix of a `what` call of n rows -> (float32 (n_data, dout) array, n_data), or (None, 0) for None (the
    record's data); one spectrum may come as (dout,).  ValueError unless n_data >= 1 divides n."""
    if data is None:
        return None, 0
    dp = np.ascontiguousarray(data, dtype=np.float32)
    if dp.ndim == 1:
        dp = dp[None, :]
    if dp.ndim != 2 or dp.shape[1] != dout or dp.shape[0] < 1:
        raise ValueError("%s: data must be (n_data, %d), got %r" % (what, dout, np.shape(data)))
    if n % dp.shape[0]:
        raise ValueError("%s: %d rows are not a multiple of %d data rows" % (what, n, dp.shape[0]))
    return dp, dp.shape[0]


def _count_opts(what, o, keys, below):
    """The counts `keys` of a sampler's options o, `below` {key: its limit}: ValueError for what the library would refuse"""
    for k in keys:
        if int(o[k]) != o[k] or int(o[k]) < 0:
            raise ValueError("%s: %s = %r (a non-negative integer)" % (what, k, o[k]))
    if any(int(o[k]) >= lim for k, lim in below.items()):
        raise ValueError("%s: count out of range" % what)


def _step_opts(what, o, more=()):
    """The counts of the options o of a sampler that runs n_warmup + n_steps steps (and the keys `more`)"""
    _count_opts(what, o, tuple(more) + ("n_steps", "n_warmup", "thin", "chain0", "step0", "seed"),
                {"n_steps": 2 ** 31, "n_warmup": 2 ** 31, "thin": 2 ** 31, "seed": 2 ** 64})
    if int(o["step0"]) + int(o["n_warmup"]) + int(o["n_steps"]) >= 2 ** 32:
        raise ValueError("%s: step0 + n_warmup + n_steps must stay below 2^32" % what)


def _whole_groups(what, noun, n, n_data, G):
    """ValueError unless the n rows of a `what` call (None: not known yet), and with n_data the rows of a data row, are
    whole `noun` of G rows"""
    if n is not None and (n % G or (n_data and (n // n_data) % G)):
        raise ValueError("%s: %d rows%s are no whole %s of %d" % (what, n, " over %d data rows" % n_data if n_data else "", noun, G))


def _sample_results(x, o, samples, diagnostics, rows=(), diag_rows=()):
    """The result arrays every sampler's host form returns for the start rows x under the options o, by the names of its
    out struct; rows / diag_rows: (name, dtype) of the sampler's own (n,) results, always / with diagnostics"""
    n, din = x.shape
    keep = o.n_steps // o.thin if o.thin > 0 else 0
    res = {"x_last": np.empty_like(x), "lnl_last": np.empty(n, np.float32)}
    res.update({k: np.empty(n, t) for k, t in rows})
    res.update({"accept_rate": np.empty(n, np.float64), "mean_u": np.empty((n, din), np.float64),
                "cov_u": np.empty((n, din, din), np.float64)})
    if samples and keep > 0:
        res["samples"] = np.empty((n, keep, din), x.dtype)
        res["samples_lnl"] = np.empty((n, keep), np.float32)
    if diagnostics:
        res["last_prop_u"] = np.empty((n, din), np.float32)
        res["last_log_alpha"] = np.empty(n, np.float64)
        res.update({k: np.empty(n, t) for k, t in diag_rows})
    return res


def _last_route(fn, h, tables, slots=8):
    """fn(h, int* route per table, long long counts[slots] per table) -> ([name of the last route per table],
    [{route name: calls since creation, zero counts left out} per table])."""
    routes = [C.c_int(0) for _ in tables]
    counts = [(C.c_longlong * slots)() for _ in tables]
    check(fn(h, *[C.byref(r) for r in routes], *counts))
    return ([t.get(r.value, "none") for t, r in zip(tables, routes)],
            [{t[i]: int(c[i]) for i in t if c[i]} for t, c in zip(tables, counts)])


class _Owned:
    """A C handle that must outlive the handles built on it (a Stack its Trainers, a Trainer the Joint / Sweep it is
    part of).  Python gives no such order: when a script ends, everything reachable from its module namespace is one
    unreachable cycle (every function defined there refers to it) and the collector calls the finalizers of such a set
    in ANY order -- a Trainer destroyed before its Joint was a use-after-free in v21_joint_destroy (r4: found by
    scripts/diag/joint_fuzz.py as a segmentation fault at interpreter exit).  So the wrappers count: finalizing a
    wrapper only marks it; its handle is destroyed once nothing built on it is left, children first."""

    def _own(self, destroy, parents=()):
        self._destroy, self._parents, self._children, self._finalized = destroy, list(parents), 0, False
        for p in self._parents:
            p._children += 1

    def _release(self):
        self._finalized = True
        self._try_destroy()

    def _try_destroy(self):
        if not self._finalized or self._children > 0 or not getattr(self, "h", None):
            return
        h, self.h = self.h, None
        try:
            self._destroy(h)
        except Exception:
            pass
        parents, self._parents = self._parents, []
        for p in parents:
            p._children -= 1
            p._try_destroy()

    def __del__(self):
        try:
            if hasattr(self, "_finalized"):
                self._release()
        except Exception:
            pass


class Context:
    """One per device.  Owns a HIP stream; calls on one context are serialised."""
    _default = {}

    def __init__(self, device=0):
        self.lib = load_library()
        n = C.c_int(0)
        st = self.lib.v21_device_count(C.byref(n))
        if st != 0 or n.value < 1:
            raise EngineUnavailable("no HIP device visible (v21_device_count -> %d, n=%d): the MI355X "
                                    "engine has no CPU fallback" % (st, n.value))
        h = _P()
        check(self.lib.v21_ctx_create(device, C.byref(h)))
        self.h, self.device = h, device
        self.lock = threading.Lock()
        self.nranks, self.rank = 1, 0  # the data-parallel communicator's (comm_init*)
        self._host_ops = None          # comm_init_host: the callbacks the library holds pointers to
        self._pin_pool = {"free": [], "live": 0, "lock": threading.Lock()}  # pinned_empty: (pointer, bytes) of idle buffers

    @classmethod
    def default(cls, device=None):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("V21_DEVICE_FROM_RANK") else 0
        if device not in cls._default:
            cls._default[device] = cls(device)
        return cls._default[device]

    def sync(self):
        check(self.lib.v21_ctx_sync(self.h))

    def set_stream(self, hip_stream):
        check(self.lib.v21_ctx_set_stream(self.h, _P(hip_stream)))

    def poison_lds(self, pattern=0xFFFFFFFF):
        """Diagnostics: fill every CU's LDS with ``pattern`` (NaN by default) before the next launch."""
        check(self.lib.v21_debug_poison_lds(self.h, pattern))

    def clock_probe_start(self, duration_ms, period_us=50.0):
        """Diagnostics: sample the shader clock for `duration_ms` beside the kernels launched meanwhile (include/v21.h)."""
        check(self.lib.v21_debug_clock_probe_start(self.h, float(duration_ms), float(period_us)))

    def clock_probe_read(self):
        """-> {"ghz_mean", "ghz_min", "ghz_max", "samples"} of the probe started last (waits for it)."""
        a, b, c_, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int(0)
        check(self.lib.v21_debug_clock_probe_read(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(n)))
        return {"ghz_mean": a.value, "ghz_min": b.value, "ghz_max": c_.value, "samples": n.value}

    def memset(self, dptr, byte, nbytes):
        check(self.lib.v21_memset(self.h, _P(dptr), int(byte), int(nbytes)))

    def malloc(self, nbytes):
        p = _P()
        check(self.lib.v21_malloc(self.h, nbytes, C.byref(p)))
        return p.value

    # ---- page-locked result buffers -----------------------------------------------------------
    # A large predict() result lands in host memory over PCIe; into an ordinary numpy array the
    # runtime goes through an internal staging buffer (~10 GB/s), into page-locked memory it goes
    # directly.  Pinning is expensive, so buffers are pooled: an array handed out owns its buffer
    # until it is garbage-collected, then the buffer returns to the pool (at most PIN_POOL_MAX
    # buffers are alive; beyond that, and for small results, plain numpy arrays are used).
    PIN_MIN_BYTES = 8 << 20
    PIN_POOL_MAX = 4

    def pinned_empty(self, shape, dtype=np.float32):
        """A numpy array in page-locked memory, or None (pool exhausted / small / unavailable)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if nbytes < self.PIN_MIN_BYTES:
            return None
        pool, ptr = self._pin_pool, None
        with pool["lock"]:  # finalizers of released arrays may run on any thread
            for i, (p, cap) in enumerate(pool["free"]):
                if cap >= nbytes:
                    ptr, cap_ = pool["free"].pop(i)
                    break
            if ptr is None:
                if pool["live"] + len(pool["free"]) >= self.PIN_POOL_MAX:
                    if pool["free"]:  # replace the smallest idle buffer by one that fits
                        pool["free"].sort(key=lambda t: t[1])
                        q, _ = pool["free"].pop(0)
                        self.lib.v21_host_free(self.h, _P(q))
                    else:
                        return None
                hp = _P()
                if self.lib.v21_host_alloc(self.h, nbytes, C.byref(hp)) != 0:
                    return None
                ptr, cap_ = hp.value, nbytes
            pool["live"] += 1
        raw = (C.c_char * nbytes).from_address(ptr)
        arr = np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

        def _back(pool=pool, ptr=ptr, cap=cap_):
            with pool["lock"]:
                pool["live"] -= 1
                pool["free"].append((ptr, cap))
        weakref.finalize(raw, _back)  # `raw` lives exactly as long as any view of the array
        return arr

    def free(self, dptr):
        check(self.lib.v21_free(self.h, _P(dptr)))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        check(self.lib.v21_memcpy_h2d(self.h, _P(dptr), arr.ctypes.data_as(_P), arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags.c_contiguous
        check(self.lib.v21_memcpy_d2h(self.h, arr.ctypes.data_as(_P), _P(dptr), arr.nbytes))

    def event(self):
        e = _P()
        check(self.lib.v21_event_create(self.h, C.byref(e)))
        return e

    def record(self, ev):
        check(self.lib.v21_event_record(self.h, ev))

    def elapsed_ms(self, a, b):
        ms = C.c_float(0)
        check(self.lib.v21_event_elapsed_ms(self.h, a, b, C.byref(ms)))
        return ms.value

    # data-parallel communicator (RCCL inside the library)
    def comm_unique_id(self):
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        check(self.lib.v21_comm_get_unique_id(self.h, buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(uid)
        check(self.lib.v21_comm_init(self.h, nranks, rank, buf))
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_init_host(self, nranks, rank, allreduce, reduce_scatter, allgather):
        """Collectives supplied by the host: three callables ``f(array_view, n_or_n_per) -> None`` that work IN
        PLACE on a float32 numpy view of the library's page-locked staging buffer (see include/v21.h)."""
        def wrap(fn, per_rank):
            def cb(_user, ptr, n):
                try:
                    total = n * nranks if per_rank else n
                    fn(np.ctypeslib.as_array(ptr, shape=(total,)), int(n))
                    return 0
                except Exception:  # an exception must not unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            return _HOST_AR(cb)
        self._host_ops = CommHostOps(None, wrap(allreduce, False), wrap(reduce_scatter, True), wrap(allgather, True))
        check(self.lib.v21_comm_init_host(self.h, nranks, rank, C.byref(self._host_ops)))
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_set_sharded(self, on=True):
        check(self.lib.v21_comm_set_sharded(self.h, 1 if on else 0))

    def comm_init_null(self, nranks, rank=0):
        """A communicator without a transport (include/v21.h: v21_comm_init_null): the N > 1 step structure on one GPU,
        nothing exchanged -- for timing the compute side of a data-parallel step, never for training."""
        check(self.lib.v21_comm_init_null(self.h, int(nranks), int(rank)))
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_set_buckets(self, buckets):
        """1: one all-reduce per step (default); 2: two, the output-side half overlapping the second weight-gradient launch."""
        check(self.lib.v21_comm_set_buckets(self.h, int(buckets)))

    def comm_info(self):
        """(nranks, rank, transport) as the attached communicator reports them; transport "none" / "rccl" / "host"."""
        n, r, t = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self.lib.v21_comm_info(self.h, C.byref(n), C.byref(r), C.byref(t)))
        return n.value, r.value, ("none", "rccl", "host", "null")[t.value]

    def ranks_seen(self):
        """Sum of 1.0 over the communicator (one all-reduce through the library's transport): how many ranks really
        take part in an exchange.  A collective call: every rank must make it."""
        d = self.malloc(4)
        try:
            self.h2d(d, np.ones(1, np.float32))
            self.allreduce(d, 1)
            out = np.zeros(1, np.float32)
            self.d2h(out, d)
        finally:
            self.free(d)
        return int(round(float(out[0])))

    def comm_destroy(self):
        check(self.lib.v21_comm_destroy(self.h))
        self.nranks, self.rank = 1, 0

    def reduce_scatter(self, dptr, n_per):
        check(self.lib.v21_comm_reduce_scatter_f32(self.h, _P(dptr), n_per))

    def allgather(self, dptr, n_per):
        check(self.lib.v21_comm_allgather_f32(self.h, _P(dptr), n_per))

    def allreduce(self, dptr, n):
        check(self.lib.v21_comm_allreduce_f32(self.h, _P(dptr), n))


class Stack(_Owned):
    """A dense stack (v21_mlp): dims[0] -> ... -> dims[-1], per-layer activation."""

    def __init__(self, ctx, dims, act):
        self.ctx, self.lib = ctx, ctx.lib
        self.dims, self.act = [int(d) for d in dims], [int(a) for a in act]
        assert len(self.act) == len(self.dims) - 1
        h = _P()
        check(self.lib.v21_mlp_create(ctx.h, *_layers(self.dims, self.act), C.byref(h)))
        self.h = h
        self._own(self.lib.v21_mlp_destroy)
        n = C.c_size_t(0)
        check(self.lib.v21_mlp_num_params(h, C.byref(n)))
        self.num_params = n.value
        # what the device holds, as use_output_stats / use_input_stats / use_likelihood left it (None: nothing, or set directly)
        self.out_stats = self.in_stats = self.lk_record = self.nu_record = self.prior_record = self.hold_record = None

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32).ravel()
        check(self.lib.v21_mlp_set_weights(self.h, _fptr(flat), flat.size))

    def get_weights(self):
        out = np.empty(self.num_params, np.float32)
        check(self.lib.v21_mlp_get_weights(self.h, _fptr(out), out.size))
        return out

    def set_input_transform(self, log_mask, zero_floor, lo, hi):
        self.in_stats = None
        if log_mask is None:
            check(self.lib.v21_mlp_set_input_transform(self.h, None))
            return
        t = AffineIn()
        n = len(lo)
        t.n = n
        for j in range(n):
            t.log_mask[j] = int(bool(log_mask[j]))
            t.zero_floor[j] = float(zero_floor[j])
            t.lo[j] = float(lo[j])
            t.span[j] = float(hi[j] - lo[j])  # float64, formed as the reference forms `maximum - minimum` (preprocess.py:106)
        check(self.lib.v21_mlp_set_input_transform(self.h, C.byref(t)))

    def set_output_transform(self, std, mean):
        self.out_stats = None
        if mean is None:
            check(self.lib.v21_mlp_set_output_transform(self.h, None))
            return
        mean = np.ascontiguousarray(mean, dtype=np.float32)
        t = AffineOut(float(std), _fptr(mean), mean.size)
        check(self.lib.v21_mlp_set_output_transform(self.h, C.byref(t)))

    # The records the class surface evaluates with, uploaded only when they changed: the statistics records are compared
    # by identity (preprocess hands out a new one whenever the training set changed), the likelihood record by value.
    def use_output_stats(self, ss):
        """set_output_transform from a preprocess.SignalStats record"""
        if self.out_stats is not ss:
            self.set_output_transform(ss.std, ss.mean)
            self.out_stats = ss

    def use_input_stats(self, ps):
        """set_input_transform from a preprocess.ParamStats record"""
        if self.in_stats is not ps:
            self.set_input_transform(ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
            self.in_stats = ps

    def use_likelihood(self, d, w):
        """set_likelihood(d, w); the record is kept on the host as `lk_record` = (d, w)"""
        rec = self.lk_record
        if rec is None or not (np.array_equal(rec[0], d) and np.array_equal(rec[1], w)):
            self.set_likelihood(d, w)
            self.lk_record = (d.copy(), w.copy())

    def use_nuisance(self, basis):
        """set_nuisance(basis) (None: no nuisance modes), uploaded only when it changed; kept on the host as `nu_record`.
        After use_likelihood: the library re-whitens the basis it holds whenever the record changes."""
        rec = self.nu_record
        if basis is None:
            if rec is not None or self.nuisance_modes():
                self.set_nuisance(None)
            return
        basis = np.asarray(basis, np.float64)
        if rec is None or not np.array_equal(rec, basis):
            self.set_nuisance(basis)
            self.nu_record = basis.copy()

    def use_prior(self, prior):
        """set_prior(kind, mu, sd) from a (kind, mu, sd) triple (None: no prior), set only when it changed; kept on the
        host by value as `prior_record`"""
        rec = self.prior_record
        if prior is None:
            if rec is not None:
                self.set_prior(None)
                self.prior_record = None
            return
        new = (np.array(prior[0], np.int32), np.array(prior[1], np.float64), np.array(prior[2], np.float64))
        if rec is None or not all(np.array_equal(a, b) for a, b in zip(rec, new)):
            self.set_prior(*new)
            self.prior_record = new

    def use_hold(self, hold):
        """set_hold(hold, u) from a (hold, u) pair (None: nothing held), set only when it changed; kept on the host by
        value as `hold_record`"""
        rec = self.hold_record
        if hold is None:
            if rec is not None:
                self.set_hold(None)
                self.hold_record = None
            return
        new = (np.array(hold[0], np.int32), np.array(hold[1], np.float64))
        if rec is None or not all(np.array_equal(a, b) for a, b in zip(rec, new)):
            self.set_hold(*new)
            self.hold_record = new

    def has_fused(self, precision="f32"):
        y = C.c_int(0)
        check(self.lib.v21_mlp_has_fused(self.h, precision_id(precision), C.byref(y)))
        return bool(y.value)

    def last_route(self):
        """(route name of the last device forward call, {route name: calls since creation}) -- written where the kernels
        are launched (include/v21.h: v21_mlp_last_route)."""
        (last,), (counts,) = _last_route(self.lib.v21_mlp_last_route, self.h, [FWD_ROUTES])
        return last, counts

    def jit(self, precision="f32", wait_ms=-1):
        """Ask for the fused kernel of THIS stack (run-time instantiation, include/v21.h: v21_mlp_jit) and wait up to
        `wait_ms` (< 0: until compiled).  -> "ready" / "compiling"; raises EngineError when the stack cannot have one."""
        s = C.c_int(0)
        check(self.lib.v21_mlp_jit(self.h, precision_id(precision), int(wait_ms), C.byref(s)))
        return "ready" if s.value == 1 else "compiling"

    def jit_jacobian(self, precision="f32", wait_ms=-1):
        """Ask for the fused JACOBIAN kernel of THIS stack (include/v21.h: v21_mlp_jit_jacobian) and wait up to `wait_ms`
        (< 0: until compiled).  -> "ready" / "compiling"; raises EngineError when the stack cannot have one.  Opt-in:
        once it is ready every Jacobian-side call of this stack in `precision` takes the "fused_rt" route."""
        s = C.c_int(0)
        check(self.lib.v21_mlp_jit_jacobian(self.h, precision_id(precision), int(wait_ms), C.byref(s)))
        return "ready" if s.value == 1 else "compiling"

    def jit_loglike(self, precision="f32", wait_ms=-1):
        """Ask for the fused forward-only ln L kernel of THIS stack (include/v21.h: v21_mlp_jit_loglike) and wait up to
        `wait_ms` (< 0: until compiled).  -> "ready" / "compiling"; raises EngineError when the stack cannot have one.
        Opt-in: once it is ready every loglike_fwd, sample_ensemble and sample_nested call of this stack in `precision`
        whose data layout the fused route serves takes the "fused_rt" route."""
        s = C.c_int(0)
        check(self.lib.v21_mlp_jit_loglike(self.h, precision_id(precision), int(wait_ms), C.byref(s)))
        return "ready" if s.value == 1 else "compiling"

    def forward(self, x, precision="f32", flags=0):
        """host (n, in) float32/float64 -> host (n, out) float32"""
        x, dt = self._rows(x)
        y = self.ctx.pinned_empty((x.shape[0], self.dims[-1]))
        if y is None:
            y = np.empty((x.shape[0], self.dims[-1]), np.float32)
        with self.ctx.lock:
            check(self.lib.v21_mlp_forward(self.h, x.ctypes.data_as(_P), dt, x.shape[0], _fptr(y),
                                           precision_id(precision), flags))
        return y

    def _rows(self, x):
        """host rows as the library takes them: (contiguous (n, in) float32 or float64, 1 for float64 / 0)"""
        x = np.asarray(x)
        if x.dtype != np.float64:
            x = x.astype(np.float32, copy=False)
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[1] != self.dims[0]:
            raise ValueError("expected input of shape (n, %d), got %r" % (self.dims[0], x.shape))
        return x, (1 if x.dtype == np.float64 else 0)

    def jacobian(self, x, precision="f32", flags=0, return_outputs=False):
        """host (n, in) float32/float64 -> jac (n, in, out) float32: jac[n, j, k] = d out[n, k] / d x[n, j] (include/v21.h:
        v21_mlp_jacobian; flags as for forward).  return_outputs: (y, jac) with y the forward's (n, out)."""
        x, dt = self._rows(x)
        n, din, dout = x.shape[0], self.dims[0], self.dims[-1]
        jac = np.empty((n, din, dout), np.float32)
        y = np.empty((n, dout), np.float32) if return_outputs else None
        with self.ctx.lock:
            check(self.lib.v21_mlp_jacobian(self.h, x.ctypes.data_as(_P), dt, n, _opt(y), _fptr(jac),
                                            precision_id(precision), flags))
        return (y, jac) if return_outputs else jac

    def set_likelihood(self, data, inv_var):
        """Gaussian likelihood record: data d and inverse variances 1 / sigma^2 per output bin (copied; None clears)."""
        self.lk_record = None
        if data is None:
            self.nu_record = None  # (the library clears both records)
            check(self.lib.v21_mlp_set_likelihood(self.h, None, None, 0))
            return
        d = np.ascontiguousarray(data, dtype=np.float32).ravel()
        w = np.ascontiguousarray(inv_var, dtype=np.float32).ravel()
        if d.size != self.dims[-1] or w.size != self.dims[-1]:
            raise ValueError("likelihood: expected %d bins, got %d / %d" % (self.dims[-1], d.size, w.size))
        check(self.lib.v21_mlp_set_likelihood(self.h, _fptr(d), _fptr(w), d.size))

    def set_nuisance(self, basis):
        """Linear nuisance modes with a flat prior, integrated out of every likelihood quantity of this stack (include/v21.h:
        v21_mlp_set_nuisance): basis (K, out) float64, 1 <= K <= 8 (copied; None clears).  Needs a likelihood record."""
        self.nu_record = None
        if basis is None:
            check(self.lib.v21_mlp_set_nuisance(self.h, None, 0, 0))
            return
        A = np.ascontiguousarray(basis, dtype=np.float64)
        if A.ndim != 2 or A.shape[1] != self.dims[-1]:
            raise ValueError("nuisance: basis must be (K, %d), got %r" % (self.dims[-1], np.shape(basis)))
        check(self.lib.v21_mlp_set_nuisance(self.h, A.ctypes.data_as(C.POINTER(C.c_double)), A.shape[0], A.shape[1]))

    def set_prior(self, kind, mu=None, sd=None):
        """The samplers' prior in the transformed coordinates u (include/v21.h: v21_mlp_set_prior): per input column
        kind 0 (uniform on [-1, 1]) or 1 (normal(mu, sd) truncated to it); copied.  None clears: uniform everywhere."""
        self.prior_record = None
        if kind is None:
            check(self.lib.v21_mlp_set_prior(self.h, None, None, None, 0))
            return
        kind = np.ascontiguousarray(kind, dtype=np.int32).ravel()
        mu = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64).ravel()
        sd = None if sd is None else np.ascontiguousarray(sd, dtype=np.float64).ravel()
        for a in (mu, sd):
            if a is not None and a.size != kind.size:
                raise ValueError("set_prior: kind, mu and sd must have one entry per input column")
        dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
        check(self.lib.v21_mlp_set_prior(self.h, kind.ctypes.data_as(C.POINTER(C.c_int32)), dp(mu), dp(sd), kind.size))

    def set_hold(self, hold, u=None):
        """The samplers' held columns in the transformed coordinates u (include/v21.h: v21_mlp_set_hold): per input column
        hold 0 (sampled) or 1 (held at u, rounded to float32 once in the library); copied.  None, or nothing held, clears.
        The four samplers read the record; the fits, fisher and loglike do not."""
        self.hold_record = None
        if hold is None:
            check(self.lib.v21_mlp_set_hold(self.h, None, None, 0))
            return
        hold = np.ascontiguousarray(hold, dtype=np.int32).ravel()
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float64).ravel()
        if u is not None and u.size != hold.size:
            raise ValueError("set_hold: hold and u must have one entry per input column")
        if u is None and hold.any():
            raise ValueError("set_hold: a held column needs its u")
        check(self.lib.v21_mlp_set_hold(self.h, hold.ctypes.data_as(C.POINTER(C.c_int32)),
                                        None if u is None else u.ctypes.data_as(C.POINTER(C.c_double)), hold.size))

    def nuisance_modes(self):
        """the number of nuisance modes the library holds for this stack (0: none)"""
        k = C.c_int32(0)
        check(self.lib.v21_mlp_nuisance_info(self.h, C.byref(k)))
        return k.value

    def nuisance_coef(self, x, precision="f32", flags=0):
        """host (n, in) -> (n, K) float64: the best-fit amplitudes of the nuisance modes for the record's raw data at every
        row (include/v21.h: v21_mlp_nuisance_coef)."""
        x, dt = self._rows(x)
        K = self.nuisance_modes()
        coef = np.empty((x.shape[0], max(K, 1)), np.float64)
        with self.ctx.lock:
            check(self.lib.v21_mlp_nuisance_coef(self.h, x.ctypes.data_as(_P), dt, x.shape[0], coef.ctypes.data_as(C.POINTER(C.c_double)),
                                                 precision_id(precision), flags))
        return coef

    def loglike(self, x, precision="f32", flags=0, grad=True):
        """host (n, in) -> lnl (n,) [, grad (n, in)]: ln L = -1/2 sum w (d - out)^2 of the record set_likelihood left (with
        nuisance modes set: marginalised over them, as are fisher, fit and sample)."""
        x, dt = self._rows(x)
        n = x.shape[0]
        lnl = np.empty(n, np.float32)
        g = np.empty((n, self.dims[0]), np.float32) if grad else None
        with self.ctx.lock:
            check(self.lib.v21_mlp_loglike(self.h, x.ctypes.data_as(_P), dt, n, _fptr(lnl), _opt(g), precision_id(precision), flags))
        return (lnl, g) if grad else lnl

    def loglike_fwd(self, x, precision="f32", flags=0, data=None):
        """host (n, in) -> lnl (n,) float32 without a gradient and without a Jacobian (include/v21.h: v21_mlp_loglike_fwd):
        against the record set_likelihood left, or against data (n_data, out) with n % n_data == 0, row i scored against
        data row i // (n // n_data); the inverse variances are the record's either way."""
        x, dt = self._rows(x)
        n = x.shape[0]
        dp, nd = _data_rows("loglike_fwd", data, n, self.dims[-1])
        lnl = np.empty(n, np.float32)
        with self.ctx.lock:
            check(self.lib.v21_mlp_loglike_fwd(self.h, x.ctypes.data_as(_P), dt, n, _opt(dp), nd, _fptr(lnl), precision_id(precision), flags))
        return lnl

    def loglike_fwd_dev(self, d_x, ldx, n, d_lnl, d_data=None, n_data=0, precision="f32", flags=0):
        """v21_mlp_loglike_fwd_dev: device addresses, asynchronous on the context's stream"""
        check(self.lib.v21_mlp_loglike_fwd_dev(self.h, _P(d_x), ldx, n, _opt(d_data), n_data, _P(d_lnl), precision_id(precision), flags))

    def last_lnl_route(self):
        """(route name of the last loglike_fwd / loglike_fwd_dev call, {route name: calls since creation})."""
        (last,), (counts,) = _last_route(self.lib.v21_mlp_last_lnl_route, self.h, [LNL_ROUTES_RT], slots=4)
        return last, counts

    def route_loglike_fwd(self, precision, n, n_data=0, flags=0):
        """the route a loglike_fwd call of n rows against n_data data rows (0: the record) takes on this stack now"""
        return route_loglike_fwd(self.dims, self.act, precision, n, n_data, self.nuisance_modes(), flags)

    def jacobian_dev(self, d_x, ldx, n, d_y, ldy, d_jac, precision="f32", flags=0):
        check(self.lib.v21_mlp_jacobian_dev(self.h, _P(d_x), ldx, n, _opt(d_y), ldy, _P(d_jac), precision_id(precision), flags))

    def loglike_dev(self, d_x, ldx, n, d_lnl, d_grad, precision="f32", flags=0):
        check(self.lib.v21_mlp_loglike_dev(self.h, _P(d_x), ldx, n, _P(d_lnl), _opt(d_grad), precision_id(precision), flags))

    def fisher(self, x, precision="f32", flags=0, lnl=False, grad=False):
        """host (n, in) -> F (n, in, in) float32, F = J^T W J with W the inverse variances of the likelihood record
        (include/v21.h: v21_mlp_fisher); with lnl / grad also ln L (n,) / its gradient (n, in): (F, lnl[, grad])."""
        x, dt = self._rows(x)
        n, din = x.shape[0], self.dims[0]
        F = np.empty((n, din, din), np.float32)
        lv = np.empty(n, np.float32) if lnl else None
        g = np.empty((n, din), np.float32) if grad else None
        with self.ctx.lock:
            check(self.lib.v21_mlp_fisher(self.h, x.ctypes.data_as(_P), dt, n, _fptr(F), _opt(lv), _opt(g), precision_id(precision), flags))
        return (F,) + tuple(a for a in (lv, g) if a is not None) if (lnl or grad) else F

    @staticmethod
    def fit_opts(max_iter=None, lambda0=None, xtol=None, check_every=None):
        o = dict(FIT_DEFAULTS)
        for k, v in (("max_iter", max_iter), ("lambda0", lambda0), ("xtol", xtol), ("check_every", check_every)):
            if v is not None:
                o[k] = v
        return FitOpts(int(o["max_iter"]), float(o["lambda0"]), float(o["xtol"]), int(o["check_every"]))

    def fit(self, x0, precision="f32", flags=0, data=None, max_iter=None, lambda0=None, xtol=None, check_every=None,
            fisher=False):
        """Projected Levenberg-Marquardt maximum-likelihood fit of every start row (include/v21.h: v21_mlp_fit; needs the
        input transform and a likelihood record).  x0: (n, in) raw starts, float32 or float64; data: None (the record's
        data) or (n_data, out) with n % n_data == 0, row i fitting data row i // (n // n_data).
        -> dict x_hat (n, in) in x0's dtype, lnl, lnl_start (n,) float32, status (n,) int32 [, fisher (n, in, in)]."""
        x, dt = self._rows(x0)
        n, din, dout = x.shape[0], self.dims[0], self.dims[-1]
        if din > 8:
            raise ValueError("fit: %d parameters (at most 8)" % din)
        dp, nd = _data_rows("fit", data, n, dout)
        opts = self.fit_opts(max_iter, lambda0, xtol, check_every)
        xh = np.empty_like(x)
        lnl, l0, status = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32)
        F = np.empty((n, din, din), np.float32) if fisher else None
        with self.ctx.lock:
            check(self.lib.v21_mlp_fit(self.h, x.ctypes.data_as(_P), dt, n, _opt(dp), nd, C.byref(opts),
                                       xh.ctypes.data_as(_P), _fptr(lnl), _fptr(l0), _opt(F),
                                       status.ctypes.data_as(C.POINTER(C.c_int32)), precision_id(precision), flags))
        out = {"x_hat": xh, "lnl": lnl, "lnl_start": l0, "status": status}
        if fisher:
            out["fisher"] = F
        return out

    @staticmethod
    def map_opts(use_prior=False, hold=None, in_dim=8):
        """v21_map_opts; ValueError for what the library would refuse.  hold: None, or one 0 / 1 (or bool) per input column"""
        if use_prior not in (0, 1, False, True):
            raise ValueError("fit_map: use_prior = %r (0 or 1)" % (use_prior,))
        o = MapOpts(int(use_prior), (C.c_int * 8)())
        if hold is not None:
            h = np.asarray(hold)
            if h.shape != (in_dim,):
                raise ValueError("fit_map: hold must have one entry per input column (%d), got %r" % (in_dim, np.shape(hold)))
            for i, v in enumerate(h.tolist()):
                if v not in (0, 1, False, True):
                    raise ValueError("fit_map: hold[%d] = %r (0 or 1)" % (i, v))
                o.hold[i] = int(v)
        return o

    def fit_map(self, x0, precision="f32", flags=0, data=None, max_iter=None, lambda0=None, xtol=None, check_every=None,
                fisher=False, use_prior=False, hold=None, outputs=MAP_OUTPUTS):
        """``fit`` on ln L + ln p of the stack's prior record (use_prior; include/v21.h: v21_mlp_fit_map) with the columns
        of ``hold`` (one 0 / 1 per input column) kept at their clamped start.  -> fit's dict and, of ``outputs``: lnp (n,)
        float64 (unnormalised, over the free normal columns), laplace (n,) float64 (the Laplace approximation of
        ln of the integral of L p over the free columns), prec_u (n, in, in) float32."""
        x, dt = self._rows(x0)
        n, din, dout = x.shape[0], self.dims[0], self.dims[-1]
        if din > 8:
            raise ValueError("fit_map: %d parameters (at most 8)" % din)
        dp, nd = _data_rows("fit_map", data, n, dout)
        opts = self.fit_opts(max_iter, lambda0, xtol, check_every)
        mo = self.map_opts(use_prior, hold, din)
        unknown = [k for k in outputs if k not in MAP_OUTPUTS]
        if unknown:
            raise ValueError("fit_map: unknown output %r (of %s)" % (unknown[0], ", ".join(MAP_OUTPUTS)))
        xh = np.empty_like(x)
        lnl, l0, status = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32)
        F = np.empty((n, din, din), np.float32) if fisher else None
        shapes = {"lnp": ((n,), np.float64), "laplace": ((n,), np.float64), "prec_u": ((n, din, din), np.float32)}
        extra = {k: np.empty(*shapes[k]) for k in MAP_OUTPUTS if k in outputs}
        mout = MapOut(*[extra[k].ctypes.data if k in extra else None for k in MAP_OUTPUTS])
        with self.ctx.lock:
            check(self.lib.v21_mlp_fit_map(self.h, x.ctypes.data_as(_P), dt, n, _opt(dp), nd, C.byref(opts), C.byref(mo),
                                           xh.ctypes.data_as(_P), _fptr(lnl), _fptr(l0), _opt(F),
                                           status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(mout), precision_id(precision), flags))
        out = {"x_hat": xh, "lnl": lnl, "lnl_start": l0, "status": status}
        if fisher:
            out["fisher"] = F
        out.update(extra)
        return out

    def fit_map_dev(self, d_x0, ldx, n, d_data, n_data, d_x_hat, d_lnl, d_lnl_start=None, d_fisher=None, d_status=None, out=None,
                    use_prior=False, hold=None, precision="f32", flags=0, **opts):
        """v21_mlp_fit_map_dev: device addresses (out: {name of MAP_OUTPUTS: address}), on the context's stream"""
        o, mo = self.fit_opts(**opts), self.map_opts(use_prior, hold, self.dims[0])
        mout = MapOut(*[(out or {}).get(k) for k in MAP_OUTPUTS])
        check(self.lib.v21_mlp_fit_map_dev(self.h, _P(d_x0), ldx, n, _opt(d_data), n_data, C.byref(o), C.byref(mo), _P(d_x_hat),
                                           _P(d_lnl), _opt(d_lnl_start), _opt(d_fisher), _opt(d_status), C.byref(mout),
                                           precision_id(precision), flags))

    def fisher_dev(self, d_x, ldx, n, d_fisher, d_lnl=None, d_grad=None, precision="f32", flags=0):
        check(self.lib.v21_mlp_fisher_dev(self.h, _P(d_x), ldx, n, _P(d_fisher), _opt(d_lnl), _opt(d_grad), precision_id(precision), flags))

    def fit_dev(self, d_x0, ldx, n, d_data, n_data, d_x_hat, d_lnl, d_lnl_start=None, d_fisher=None, d_status=None,
                precision="f32", flags=0, **opts):
        o = self.fit_opts(**opts)
        check(self.lib.v21_mlp_fit_dev(self.h, _P(d_x0), ldx, n, _opt(d_data), n_data, C.byref(o), _P(d_x_hat), _P(d_lnl),
                                       _opt(d_lnl_start), _opt(d_fisher), _opt(d_status), precision_id(precision), flags))

    @staticmethod
    def sample_opts(n_steps=None, n_warmup=None, thin=None, eps0=None, ridge=None, target_accept=None, seed=None, chain0=None,
                    step0=None):
        """v21_sample_opts with the defaults of SAMPLE_DEFAULTS for None; ValueError for what the library would refuse"""
        o = dict(SAMPLE_DEFAULTS)
        o.update({k: v for k, v in (("n_steps", n_steps), ("n_warmup", n_warmup), ("thin", thin), ("eps0", eps0), ("ridge", ridge),
                                    ("target_accept", target_accept), ("seed", seed), ("chain0", chain0), ("step0", step0))
                  if v is not None})
        _step_opts("sample", o)
        for k in ("eps0", "ridge"):
            if not (float(o[k]) > 0 and np.isfinite(float(o[k]))):
                raise ValueError("sample: %s = %r (positive and finite)" % (k, o[k]))
        if not 0.0 < float(o["target_accept"]) < 1.0:
            raise ValueError("sample: target_accept = %r (inside (0, 1))" % (o["target_accept"],))
        return SampleOpts(int(o["n_steps"]), int(o["n_warmup"]), int(o["thin"]), float(o["eps0"]), float(o["ridge"]),
                          float(o["target_accept"]), int(o["seed"]), int(o["chain0"]), int(o["step0"]))

    def sample(self, x0, precision="f32", flags=0, data=None, eps_start=None, samples=True, diagnostics=False, **opts):
        """Posterior sampling: one Fisher-preconditioned MALA chain per start row, on the device (include/v21.h:
        v21_mlp_sample; needs the input transform and a likelihood record).  The target is ln L of the record under a
        uniform prior on the training box in par_transform's coordinates u (log-uniform in a log10 column's raw value).
        x0: (n, in) raw starts, float32 or float64; data as for fit; eps_start: None or (n,) per-chain step sizes
        (instead of eps0); opts: n_steps, n_warmup, thin, eps0, ridge, target_accept, seed, chain0, step0 (SAMPLE_DEFAULTS).
        -> dict x_last (n, in) in x0's dtype, lnl_last (n,) float32, eps_last, accept_rate (n,), mean_u (n, in), cov_u
        (n, in, in) float64 -- the per-chain moments of u over the n_steps kept transitions -- and, with samples and
        thin > 0, samples (n, n_steps // thin, in) in x0's dtype and samples_lnl; with diagnostics, last_prop_u (n, in)
        float32 and last_log_alpha (n,) float64 of the last transition."""
        x, dt, n, dp, nd, o, es, res = self._sample_call("sample", x0, data, lambda *_: self.sample_opts(**opts), samples, diagnostics, eps_start)
        out = SampleOut(**{k: v.ctypes.data for k, v in res.items()})
        with self.ctx.lock:
            check(self.lib.v21_mlp_sample(self.h, x.ctypes.data_as(_P), dt, n, _opt(dp), nd, C.byref(o),
                                          es.ctypes.data_as(_P) if es is not None else None, C.byref(out), precision_id(precision), flags))
        return res

    def _sample_call(self, what, x0, data, opts, samples, diagnostics, eps_start=None):
        """what the host forms of the three samplers share: the rows, the data matrix, the options -- opts(n, n_data,
        in_dim) -> the options struct --, the start step sizes and the result arrays of the out struct
        -> (x, dtype id, n, data, n_data, opts, eps_start, results)"""
        x, dt = self._rows(x0)
        n, din = x.shape[0], self.dims[0]
        if din > 8:
            raise ValueError("%s: %d parameters (at most 8)" % (what, din))
        dp, nd = _data_rows(what, data, n, self.dims[-1])
        o = opts(n, nd, din)
        es = None
        if eps_start is not None:
            es = np.ascontiguousarray(eps_start, dtype=np.float64)
            if es.shape != (n,) or not np.all(es > 0):
                raise ValueError("%s: eps_start must be (%d,) positive step sizes" % (what, n))
        if isinstance(o, EnsembleOpts):
            res = _sample_results(x, o, samples, diagnostics, diag_rows=[("last_partner", np.int32)])
        else:
            res = _sample_results(x, o, samples, diagnostics, rows=[("eps_last", np.float64)])
        return x, dt, n, dp, nd, o, es, res

    def sample_dev(self, d_x0, ldx, n, d_data, n_data, out, d_eps_start=None, precision="f32", flags=0, **opts):
        """v21_mlp_sample_dev: out is a dict of device addresses by the names of SAMPLE_OUTPUTS (x_last required; samples
        float32); asynchronous on the context's stream."""
        o = self.sample_opts(**opts)
        so = SampleOut(**{k: int(v) for k, v in out.items() if v})
        check(self.lib.v21_mlp_sample_dev(self.h, _P(d_x0), ldx, n, _opt(d_data), n_data, C.byref(o), _opt(d_eps_start), C.byref(so),
                                          precision_id(precision), flags))

    @staticmethod
    def temper_opts(n_temps=1, betas=None, swap_every=0, n=None, n_data=0):
        """v21_temper_opts: n_temps rungs at the inverse temperatures betas (None: 1 for one rung), a swap event every
        swap_every transitions (0: never); ValueError for what the library would refuse -- with n (and n_data, 0: the
        record's data) also the rows of a call that are no whole ladders, or whose ladders would straddle two data rows"""
        if int(n_temps) != n_temps or not 1 <= int(n_temps) <= 32:
            raise ValueError("sample_tempered: n_temps = %r (1 .. 32)" % (n_temps,))
        T = int(n_temps)
        if betas is None:
            if T != 1:
                raise ValueError("sample_tempered: %d rungs need their betas" % T)
            betas = [1.0]
        b = np.asarray(betas, np.float64)
        if b.shape != (T,):
            raise ValueError("sample_tempered: betas must be (%d,), got %r" % (T, b.shape))
        if not np.all((b >= 0.0) & (b <= 1.0)) or not np.all(b[1:] < b[:-1]):
            raise ValueError("sample_tempered: betas = %r (inside [0, 1], strictly decreasing)" % (b.tolist(),))
        if int(swap_every) != swap_every or not 0 <= int(swap_every) < 2 ** 31:
            raise ValueError("sample_tempered: swap_every = %r (a non-negative integer)" % (swap_every,))
        _whole_groups("sample_tempered", "ladders", n, n_data, T)
        return TemperOpts(T, (C.c_double * 32)(*b.tolist()), int(swap_every))

    def sample_tempered(self, x0, n_temps=1, betas=None, swap_every=0, precision="f32", flags=0, data=None, eps_start=None, samples=True,
                        diagnostics=False, **opts):
        """Parallel-tempered posterior sampling (include/v21.h: v21_mlp_sample_tempered): n_temps consecutive rows of x0
        form one ladder, row r at inverse temperature betas[r % n_temps]; every swap_every transitions neighbouring rungs
        of a ladder propose to exchange their states.  Everything else as ``sample``, whose results come back for every
        row (a row is a rung: with betas[0] = 1 the rows 0, n_temps, 2 n_temps .. are the posterior chains), and beside
        them mean_lnl, var_lnl (the un-tempered ln L over the kept transitions) and swap_accept (the pair of this row and
        the next), all (n,) float64.  With data, the rows of one spectrum must be whole ladders."""
        self.temper_opts(n_temps, betas, swap_every)
        x, dt, n, dp, nd, o, es, res = self._sample_call("sample", x0, data, lambda *_: self.sample_opts(**opts), samples, diagnostics, eps_start)
        t = self.temper_opts(n_temps, betas, swap_every, n, nd)
        out = SampleOut(**{k: v.ctypes.data for k, v in res.items()})
        tres = {k: np.empty(n, np.float64) for k in TEMPER_OUTPUTS}
        tout = TemperOut(**{k: v.ctypes.data for k, v in tres.items()})
        with self.ctx.lock:
            check(self.lib.v21_mlp_sample_tempered(self.h, x.ctypes.data_as(_P), dt, n, _opt(dp), nd, C.byref(o), C.byref(t),
                                                   es.ctypes.data_as(_P) if es is not None else None, C.byref(out), C.byref(tout),
                                                   precision_id(precision), flags))
        res.update(tres)
        return res

    def sample_tempered_dev(self, d_x0, ldx, n, d_data, n_data, out, tout=None, n_temps=1, betas=None, swap_every=0, d_eps_start=None,
                            precision="f32", flags=0, **opts):
        """v21_mlp_sample_tempered_dev: out as for sample_dev, tout a dict of device addresses by the names of
        TEMPER_OUTPUTS (or None); asynchronous on the context's stream."""
        o = self.sample_opts(**opts)
        t = self.temper_opts(n_temps, betas, swap_every)
        so = SampleOut(**{k: int(v) for k, v in out.items() if v})
        to = TemperOut(**{k: int(v) for k, v in (tout or {}).items() if v})
        check(self.lib.v21_mlp_sample_tempered_dev(self.h, _P(d_x0), ldx, n, _opt(d_data), n_data, C.byref(o), C.byref(t), _opt(d_eps_start),
                                                   C.byref(so), C.byref(to), precision_id(precision), flags))

    @staticmethod
    def ensemble_opts(n_walkers=None, a=None, n_steps=None, n_warmup=None, thin=None, seed=None, chain0=None, step0=None, n=None,
                      n_data=0, in_dim=None):
        """v21_ensemble_opts with the defaults of ENSEMBLE_DEFAULTS for None; ValueError for what the library would refuse
        -- with in_dim also an ensemble too small for its dimension, with n (and n_data, 0: the record's data) also the
        rows of a call that are no whole ensembles, or whose ensembles would straddle two data rows"""
        o = dict(ENSEMBLE_DEFAULTS)
        o.update({k: v for k, v in (("n_walkers", n_walkers), ("a", a), ("n_steps", n_steps), ("n_warmup", n_warmup), ("thin", thin),
                                    ("seed", seed), ("chain0", chain0), ("step0", step0)) if v is not None})
        _step_opts("sample_ensemble", o, more=("n_walkers",))
        if not (float(o["a"]) > 1.0 and np.isfinite(float(o["a"]))):
            raise ValueError("sample_ensemble: a = %r (above 1 and finite)" % (o["a"],))
        W = int(o["n_walkers"])
        lo = 2 * (int(in_dim) + 1) if in_dim is not None else 2
        if W % 2 or not lo <= W <= ENSEMBLE_MAX_WALKERS:
            raise ValueError("sample_ensemble: n_walkers = %d (even, %d .. %d)" % (W, lo, ENSEMBLE_MAX_WALKERS))
        _whole_groups("sample_ensemble", "ensembles", n, n_data, W)
        return EnsembleOpts(W, float(o["a"]), int(o["n_steps"]), int(o["n_warmup"]), int(o["thin"]), int(o["seed"]), int(o["chain0"]),
                            int(o["step0"]))

    def sample_ensemble(self, x0, n_walkers=64, precision="f32", flags=0, data=None, samples=True, diagnostics=False, **opts):
        """Posterior sampling with the affine-invariant ensemble sampler (Goodman & Weare's stretch move) on forward-only
        ln L, on the device (include/v21.h: v21_mlp_sample_ensemble; needs the input transform and a likelihood record).
        n_walkers consecutive rows of x0 form one ensemble (even, at least 2 (in + 1), at most 512); the target is
        ``sample``'s.  x0: (n, in) raw starts, float32 or float64; data as for fit (the rows of one spectrum must be whole
        ensembles); opts: a, n_steps, n_warmup, thin, seed, chain0, step0 (ENSEMBLE_DEFAULTS).
        -> dict x_last (n, in) in x0's dtype, lnl_last (n,) float32, accept_rate (n,), mean_u (n, in), cov_u (n, in, in)
        float64 -- the per-walker moments of u over the n_steps kept sweeps -- and, with samples and thin > 0, samples
        (n, n_steps // thin, in) in x0's dtype and samples_lnl; with diagnostics, last_prop_u (n, in) float32,
        last_log_alpha (n,) float64 and last_partner (n,) int32 of the last sweep."""
        x, dt, n, dp, nd, o, _, res = self._sample_call(
            "sample_ensemble", x0, data, lambda n, nd, din: self.ensemble_opts(n_walkers, n=n, n_data=nd, in_dim=din, **opts), samples, diagnostics)
        out = EnsembleOut(**{k: v.ctypes.data for k, v in res.items()})
        with self.ctx.lock:
            check(self.lib.v21_mlp_sample_ensemble(self.h, x.ctypes.data_as(_P), dt, n, _opt(dp), nd, C.byref(o), C.byref(out),
                                                   precision_id(precision), flags))
        return res

    def sample_ensemble_dev(self, d_x0, ldx, n, d_data, n_data, out, n_walkers=64, precision="f32", flags=0, **opts):
        """v21_mlp_sample_ensemble_dev: out is a dict of device addresses by the names of ENSEMBLE_OUTPUTS (x_last required;
        samples float32); asynchronous on the context's stream."""
        o = self.ensemble_opts(n_walkers, **opts)
        so = EnsembleOut(**{k: int(v) for k, v in out.items() if v})
        check(self.lib.v21_mlp_sample_ensemble_dev(self.h, _P(d_x0), ldx, n, _opt(d_data), n_data, C.byref(o), C.byref(so),
                                                   precision_id(precision), flags))

    def route_ensemble(self, precision, n, n_walkers, n_data=0, flags=0, host_form=False):
        """(route, chunk rows) a sample_ensemble call of n rows in ensembles of n_walkers takes on this stack now"""
        return route_ensemble(self.dims, self.act, precision, n, n_walkers, n_data, self.nuisance_modes(), flags, host_form)

    @staticmethod
    def nested_opts(n_live=None, n_repeats=None, n_iter=None, gamma=None, seed=None, iter0=None, chain0=None, n=None, n_data=0,
                    in_dim=None):
        """v21_nested_opts with the defaults of NESTED_DEFAULTS for None; ValueError for what the library would refuse --
        with in_dim also a move counter that would overflow at the default n_repeats, with n (and n_data, 0:
        the record's data) also the rows of a call that are no whole runs, or whose runs would straddle two data rows"""
        o = dict(NESTED_DEFAULTS)
        o.update({k: v for k, v in (("n_live", n_live), ("n_repeats", n_repeats), ("n_iter", n_iter), ("gamma", gamma), ("seed", seed),
                                    ("iter0", iter0), ("chain0", chain0)) if v is not None})
        _count_opts("sample_nested", o, ("n_live", "n_repeats", "n_iter", "seed", "iter0", "chain0"),
                    {"n_repeats": 2 ** 31, "n_iter": 2 ** 31, "seed": 2 ** 64, "iter0": 2 ** 32})
        rep = int(o["n_repeats"]) or 3 * (int(in_dim) if in_dim is not None else 1)
        if (int(o["iter0"]) + int(o["n_iter"])) * rep >= 2 ** 32:
            raise ValueError("sample_nested: (iter0 + n_iter) n_repeats must stay below 2^32")
        if not 0.0 <= float(o["gamma"]) <= 1e6:
            raise ValueError("sample_nested: gamma = %r (0 .. 1e6; 0: the default)" % (o["gamma"],))
        N = int(o["n_live"])
        if N % 2 or not NESTED_MIN_LIVE <= N <= NESTED_MAX_LIVE:
            raise ValueError("sample_nested: n_live = %d (even, %d .. %d)" % (N, NESTED_MIN_LIVE, NESTED_MAX_LIVE))
        _whole_groups("sample_nested", "runs", n, n_data, N)
        return NestedOpts(N, int(o["n_repeats"]), int(o["n_iter"]), float(o["gamma"]), int(o["seed"]), int(o["iter0"]), int(o["chain0"]))

    def sample_nested(self, u0=None, n=None, n_live=256, precision="f32", flags=0, data=None, dead=True, diagnostics=False, **opts):
        """Nested sampling on forward-only ln L, on the device (include/v21.h: v21_mlp_sample_nested; needs a likelihood
        record): n_live consecutive rows are one run, the live points of one spectrum (even, 16 .. 512; an evidence needs 8 in or more).
        Everything is in u = par_transform's coordinates, the prior uniform on [-1, 1]^in.  u0: (n, in) live points to
        start from (float32 or float64; a run continues exactly from an earlier live_u with iter0 moved on), or None with
        n: drawn uniform from the seed.  data as for fit (the rows of one spectrum must be whole runs); opts: n_repeats,
        n_iter, gamma, seed, iter0, chain0 (NESTED_DEFAULTS).
        -> dict live_u (n, in) in u0's dtype (float64 for None), live_lnl (n,) float32, accept_rate (runs, n_live / 2) and,
        with dead, dead_u (n_iter, runs, n_live / 2, in), dead_lnl, lstar (n_iter, runs); with diagnostics, last_partner
        (runs, n_live / 2, 2) int32 and last_prop_u (runs, n_live / 2, in) float32 of the last move."""
        din = self.dims[0]
        if din > 8:
            raise ValueError("sample_nested: %d parameters (at most 8)" % din)
        if u0 is None:
            if n is None:
                raise ValueError("sample_nested: start rows or their number")
            x, dt, n = None, 1, int(n)
        else:
            x, dt = self._rows(u0)
            n = x.shape[0]
        dp, nd = _data_rows("sample_nested", data, n, self.dims[-1])
        o = self.nested_opts(n_live, n=n, n_data=nd, in_dim=din, **opts)
        runs, k, T, ut = n // o.n_live, o.n_live // 2, o.n_iter, (np.float64 if x is None else x.dtype)
        res = {"live_u": np.empty((n, din), ut), "live_lnl": np.empty(n, np.float32), "accept_rate": np.empty((runs, k), np.float64)}
        if dead:
            res.update({"dead_u": np.empty((T, runs, k, din), ut), "dead_lnl": np.empty((T, runs, k), np.float32),
                        "lstar": np.empty((T, runs), np.float32)})
        if diagnostics:
            res.update({"last_partner": np.empty((runs, k, 2), np.int32), "last_prop_u": np.empty((runs, k, din), np.float32)})
        out = NestedOut(**{key: v.ctypes.data for key, v in res.items()})
        with self.ctx.lock:
            check(self.lib.v21_mlp_sample_nested(self.h, x.ctypes.data_as(_P) if x is not None else None, dt, n, _opt(dp), nd, C.byref(o),
                                                 C.byref(out), precision_id(precision), flags))
        return res

    def sample_nested_dev(self, d_u0, ldx, n, d_data, n_data, out, n_live=256, precision="f32", flags=0, **opts):
        """v21_mlp_sample_nested_dev: d_u0 a device address or None (drawn starts), out a dict of device addresses by the
        names of NESTED_OUTPUTS (live_u required; dead_u and live_u float32); asynchronous on the context's stream."""
        o = self.nested_opts(n_live, in_dim=self.dims[0], **opts)
        so = NestedOut(**{k: int(v) for k, v in out.items() if v})
        check(self.lib.v21_mlp_sample_nested_dev(self.h, _P(d_u0) if d_u0 else None, ldx, n, _opt(d_data), n_data, C.byref(o), C.byref(so),
                                                 precision_id(precision), flags))

    def route_nested(self, precision, n, n_live, n_data=0, flags=0, host_form=False):
        """(route, chunk rows) a sample_nested call of n rows in runs of n_live takes on this stack now"""
        return route_nested(self.dims, self.act, precision, n, n_live, n_data, self.nuisance_modes(), flags, host_form)

    def last_jac_route(self):
        """(route name of the last Jacobian / log-likelihood call, {route name: calls since creation})."""
        (last,), (counts,) = _last_route(self.lib.v21_mlp_last_jac_route, self.h, [JAC_ROUTES], slots=4)
        return last, counts

    def forward_clocked(self, d_x, ldx, n, d_y, ldy, d_stamps, precision="f16", flags=0):
        """forward_dev through the clock-stamped instantiation of the headline stack's kernel (include/v21.h:
        v21_debug_forward_clocked); d_stamps: device buffer of 5 uint64 per 128-row workgroup."""
        check(self.lib.v21_debug_forward_clocked(self.h, _P(d_x), ldx, n, _P(d_y), ldy, precision_id(precision), flags, _P(d_stamps)))

    def forward_dev(self, d_x, ldx, n, d_y, ldy, precision="f32", flags=0):
        check(self.lib.v21_mlp_forward_dev(self.h, _P(d_x), ldx, n, _P(d_y), ldy, precision_id(precision), flags))


def _prebuild(dims, act, kernel, directory):
    check(load_library().v21_jit_prebuild(*_layers(dims, act), kernel, directory.encode() if directory else None))


def jit_prebuild_train(dims, act, precision, directory=None):
    """jit_prebuild for the fused TRAINING kernel of (dims, act, f16 | bf16) (include/v21.h: v21_trainer_jit)."""
    _prebuild(dims, act, precision_id(precision) | 16, directory)


def jit_prebuild_jacobian(dims, act, precision, directory=None):
    """jit_prebuild for the fused JACOBIAN kernel of (dims, act, precision) (include/v21.h: v21_mlp_jit_jacobian)."""
    _prebuild(dims, act, precision_id(precision) | 32, directory)


def jit_prebuild_loglike(dims, act, precision, directory=None):
    """jit_prebuild for the fused forward-only ln L kernel of (dims, act, precision) (include/v21.h: v21_mlp_jit_loglike)."""
    _prebuild(dims, act, precision_id(precision) | 64, directory)


def jit_prebuild(dims, act, precision, directory=None):
    """Compile the fused kernel of (dims, act, precision) into `directory` (None: kernel_cache/ next to libv21.so).
    Needs hiprtc but no GPU.  Call it from a process that has not loaded ANOTHER LLVM (importing torch does: hiprtc then
    finds that copy's option table, which lacks the AMDGPU flags, and LLVM ends the process) -- a build step, as
    __graft_entry__.build() uses it; at run time the library compiles in a child process of its own (csrc/jitc_main.cpp)."""
    _prebuild(dims, act, precision_id(precision), directory)


class Trainer(_Owned):
    """Adam trainer bound to a Stack (v21_trainer)."""

    def __init__(self, stack, precision="f32", max_batch=256):
        self.stack, self.lib, self.ctx = stack, stack.lib, stack.ctx
        h = _P()
        check(self.lib.v21_trainer_create(stack.h, precision_id(precision), int(max_batch), C.byref(h)))
        self.h = h
        self._own(self.lib.v21_trainer_destroy, [stack])
        self.max_batch = int(max_batch)
        self._resident = {}   # set_data: split -> (shape, hash) of the buffers the device holds
        self.n_train = None   # rows of the training split, once set_data(0, ...) has run

    def set_adam(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
        cfg = Adam(lr, beta1, beta2, eps)
        check(self.lib.v21_trainer_set_adam(self.h, C.byref(cfg)))

    def set_lr(self, lr):
        check(self.lib.v21_trainer_set_lr(self.h, float(lr)))

    def get_lr(self):
        v = C.c_float(0)
        check(self.lib.v21_trainer_get_lr(self.h, C.byref(v)))
        return v.value

    def set_data(self, which, x, y, row_weight):
        x = np.ascontiguousarray(x, dtype=np.float32)
        rw = np.ascontiguousarray(row_weight, dtype=np.float32)
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float32)
            assert y.shape[0] == x.shape[0]
        assert rw.shape == (x.shape[0],)
        # A second train() on the same arrays (the reference's recipe: emulator.py:739-764 re-feeds its numpy arrays
        # on every call) finds its split resident: (shape, 128-bit hash of every byte) of the three buffers decides.
        # One pass of the hash is ~2 ms for the reference's 44 MB against ~6.5 ms of pageable upload.
        from .preprocess import _digest
        key = tuple((a.shape, _digest(a.reshape(-1).view(np.uint8).data)) if a is not None else None for a in (x, y, rw))
        if self._resident.get(which) == key:
            return
        self._resident.pop(which, None)
        check(self.lib.v21_trainer_set_data(self.h, which, _fptr(x), _opt(y), _fptr(rw), x.shape[0]))
        self._resident[which] = key
        if which == 0:
            self.n_train = int(x.shape[0])

    def run_epoch(self, perm, batch):
        loss = C.c_double(0)
        rows = _row_table(perm, self.n_train, "Trainer.run_epoch")
        with self.ctx.lock:
            check(self.lib.v21_trainer_run_epoch(self.h, rows, int(batch), C.byref(loss)))
        return loss.value

    def evaluate(self, which, batch):
        loss = C.c_double(0)
        with self.ctx.lock:
            check(self.lib.v21_trainer_eval(self.h, which, int(batch), C.byref(loss)))
        return loss.value

    def data_dev(self, which=0):
        """-> (d_x, d_y, d_rw, n): device pointers of the resident split (d_y == d_x when it was set with y=None), for custom
        loops that step on slices of it with step_dev (include/v21.h: v21_trainer_get_data_dev)."""
        x, y, rw, n = _P(), _P(), _P(), C.c_int64(0)
        check(self.lib.v21_trainer_get_data_dev(self.h, int(which), C.byref(x), C.byref(y), C.byref(rw), C.byref(n)))
        return x.value, y.value, rw.value, n.value

    def step_dev(self, d_x, d_y, d_rw, n_rows, global_rows=None):
        check(self.lib.v21_trainer_step_dev(self.h, _P(d_x), _opt(d_y), _P(d_rw), int(n_rows),
                                            int(global_rows if global_rows is not None else n_rows)))

    def last_step_loss(self):
        v = C.c_double(0)
        check(self.lib.v21_trainer_last_step_loss(self.h, C.byref(v)))
        return v.value

    def get_state(self):
        n = self.stack.num_params
        m, v, it = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
        check(self.lib.v21_trainer_get_state(self.h, C.byref(it), _fptr(m), _fptr(v), n))
        return it.value, m, v

    def set_state(self, it, m=None, v=None):
        n = self.stack.num_params
        m = None if m is None else np.ascontiguousarray(m, np.float32)
        v = None if v is None else np.ascontiguousarray(v, np.float32)
        check(self.lib.v21_trainer_set_state(self.h, int(it), _opt(m), _opt(v), n))

    def set_vae(self, kl_weight, sample=True, seed=0):
        """Variational mode of a stack with an ACT_GAUSS layer (include/v21.h: v21_trainer_set_vae)."""
        check(self.lib.v21_trainer_set_vae(self.h, float(kl_weight), 1 if sample else 0, int(seed) & (2**64 - 1)))

    def use_graph(self, enable=True):
        """Captured-step replay (hipGraph), opt-in: one rank, no variational layer.  Same kernels, same
        arithmetic, bit-identical results; the host enqueues one graph launch per step instead of 3-14 kernels
        (measured r2: the steps are GPU-bound, so this frees the host thread but does not shorten a step)."""
        check(self.lib.v21_trainer_use_graph(self.h, 1 if enable else 0))

    def check_chain_jobs(self, fw_bytes=-1, bw_bytes=-1):
        """Diagnostics: validate the small-batch f32 chain's job table against packed streams of the given sizes
        (bytes; -1 = the allocated ones).  Raises EngineError where a row points outside."""
        check(self.lib.v21_debug_check_chain_jobs(self.h, int(fw_bytes), int(bw_bytes)))

    def route_counters(self):
        """Diagnostics: eager 16-bit steps so far by route: dict(chain=, fused=, stream_packs=, stream_adam=) -- steps through
        the 32-row chain, through the fused training kernel, fused steps that launched the stream pack first, Adam passes
        that wrote the fused kernel's stream (include/v21.h: v21_debug_trainer_counters)."""
        out = (C.c_longlong * 4)()
        check(self.lib.v21_debug_trainer_counters(self.h, out))
        return dict(zip(("chain", "fused", "stream_packs", "stream_adam"), (int(v) for v in out)))

    def jit(self, wait_ms=-1):
        """The fused training kernel of THIS trainer's stack (include/v21.h: v21_trainer_jit): wait up to `wait_ms` (< 0: until
        compiled) for its run-time instantiation.  -> "ready" / "compiling"; raises EngineError when the trainer cannot have one."""
        s = C.c_int(0)
        check(self.lib.v21_trainer_jit(self.h, int(wait_ms), C.byref(s)))
        return "ready" if s.value == 1 else "compiling"

    def phase_timing(self, steps, cut=4):
        """Stamp the next `steps` eager steps with two HIP events: the step's start and cut point `cut` (include/v21.h:
        v21_trainer_phase_timing); steps = 0: off."""
        check(self.lib.v21_trainer_phase_timing(self.h, int(steps), int(cut)))

    def phase_times(self):
        """-> (median microseconds from a step's start to the cut point, stamped steps) since the last call."""
        ms, n = C.c_double(0.0), C.c_int(0)
        check(self.lib.v21_trainer_phase_times(self.h, C.byref(ms), C.byref(n)))
        return 1e3 * ms.value, n.value

    def phase_profile(self, step, steps=50):
        """Where a step's time goes: `step()` (a callable that takes ONE optimizer step on this trainer) is run `steps`
        times per cut point with two HIP events per step, and the phases are the differences of the four cumulative times
        (the marker's own cost -- an event is a packet in the stream, ~5 us when nothing separates two -- cancels in them;
        the first phase still carries one marker: `marker_us` = the stamped whole step minus `unstamped_step_us` when the
        caller supplies the latter says how much that is).  -> dict of microseconds."""
        cum = []
        for cut in (1, 2, 3, 4):
            self.phase_timing(steps, cut)
            for _ in range(steps):
                step()
            us, n = self.phase_times()
            cum.append(us if n else float("nan"))
        self.phase_timing(0)
        return {"forward_and_activation_gradients_us": cum[0], "weight_gradients_us": cum[1] - cum[0], "exchange_exposed_us": cum[2] - cum[1],
                "adam_and_repack_us": cum[3] - cum[2], "stamped_step_us": cum[3], "steps_per_cut": steps,
                "note": "differences of cumulative start-to-cut times of four separate stamped runs (two HIP events per step); the first "
                        "phase and stamped_step_us carry one marker's cost (stamped_step_us minus the leg's unstamped ms_per_step); "
                        "exchange_exposed = the part of the gradient exchange no weight-gradient launch covers; single-rank steps whose "
                        "gradients and Adam are ONE launch report it under adam_and_repack"}

    def last_route(self):
        """((forward route, update route) of the last eager step, {(fwd or upd) route name: steps since creation}) -- written
        where the kernels are launched (include/v21.h: v21_trainer_last_route)."""
        last, (counts, upd) = _last_route(self.lib.v21_trainer_last_route, self.h, [TRAIN_FWD_ROUTES, TRAIN_UPD_ROUTES])
        counts.update(("upd:" + k, v) for k, v in upd.items())
        return tuple(last), counts

    def enable_stamps(self, on=True):
        """Cycle stamps of the chain kernel's phases (diagnostics; off by default: they cost 2-3 us per step)."""
        check(self.lib.v21_trainer_enable_stamps(self.h, 1 if on else 0))

    def chain_stamps(self, n=40):
        out = (C.c_uint64 * n)()
        check(self.lib.v21_trainer_chain_stamps(self.h, out, n))
        return np.array(out[:], dtype=np.uint64)

    def get_grad(self):
        g = np.empty(self.stack.num_params, np.float32)
        check(self.lib.v21_trainer_get_grad(self.h, _fptr(g), g.size))
        return g


class Joint(_Owned):
    """Autoencoder + latent emulator stepping together on the same rows (v21_joint_*; BASELINE configs[2])."""

    def __init__(self, ae_trainer, em_trainer, latent_layer):
        self.lib, self.ctx = ae_trainer.lib, ae_trainer.ctx
        self.trainers = (ae_trainer, em_trainer)  # keep them alive
        h = _P()
        check(self.lib.v21_joint_create(ae_trainer.h, em_trainer.h, int(latent_layer), C.byref(h)))
        self.h = h
        self._own(self.lib.v21_joint_destroy, self.trainers)

    def run_epoch(self, perm, batch):
        """-> (autoencoder epoch loss, emulator epoch loss)"""
        out = (C.c_double * 2)()
        rows = _row_table(perm, self.trainers[0].n_train, "Joint.run_epoch")
        with self.ctx.lock:
            check(self.lib.v21_joint_run_epoch(self.h, rows, int(batch), out))
        return float(out[0]), float(out[1])

    def evaluate(self):
        """-> (autoencoder validation loss, emulator validation loss against the current encoder's latents)"""
        out = (C.c_double * 2)()
        with self.ctx.lock:
            check(self.lib.v21_joint_eval(self.h, out))
        return float(out[0]), float(out[1])


class Sweep(_Owned):
    """Several Trainers stepped in lock step on one shared batch stream (v21_sweep);
    trainer 0 holds the training set."""

    def __init__(self, trainers):
        self.trainers = list(trainers)
        self.lib, self.ctx = self.trainers[0].lib, self.trainers[0].ctx
        arr = (_P * len(self.trainers))(*[t.h.value for t in self.trainers])
        h = _P()
        check(self.lib.v21_sweep_create(arr, len(self.trainers), C.byref(h)))
        self.h = h
        self._own(self.lib.v21_sweep_destroy, self.trainers)

    def run_epoch(self, perm, batch):
        losses = (C.c_double * len(self.trainers))()
        rows = _row_table(perm, self.trainers[0].n_train, "Sweep.run_epoch")
        with self.ctx.lock:
            check(self.lib.v21_sweep_run_epoch(self.h, rows, int(batch), losses))
        return [float(v) for v in losses]
