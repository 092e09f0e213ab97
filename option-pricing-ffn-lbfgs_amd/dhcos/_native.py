"""ctypes binding of libdhcos.so (the gfx950 C-ABI declared in include/dhcos.h).

The library is loaded lazily on first use from this package directory (built in-tree by
``make -C option-pricing-ffn-lbfgs_amd/csrc`` or ``__graft_entry__.build()``).  There is no CPU
fallback: if the library or a gfx950 device is missing, every compute entry point raises
``NativeError``.

HIP runtime sharing: torch-ROCm ships its own libamdhip64.so.  If a process uses both torch (e.g.
bench.py, torch.distributed) and this library, torch must be imported *before* the first call here
so that both bind to one HIP runtime; ``runtime_shared_with_torch()`` checks it.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DHCOS_LIB", os.path.join(_HERE, "libdhcos.so"))

# the header's sizes and enums (tests/test_native_abi.py holds them to include/dhcos.h)
PARAM_STRIDE = 16
MAX_N = 2048                   # longest series of the table (fast) path (DH_MAX_N)
MAX_N_PER_TERM = 65536         # longest accepted; longer than MAX_N runs the per-term path
STRIKE_ABSOLUTE = 0
STRIKE_PCT_SPOT = 1
PATH_AUTO, PATH_SPLIT, PATH_FUSED, PATH_GEN = 0, 1, 2, 3   # PATH_GEN: reported only (AUTO)
FG_SLOTS = 4                   # request slots of dh_surface_fg_begin / _end (DH_FG_SLOTS)
GEN_LOC_WORDS = 627            # DH_GEN_LOC_WORDS: key[624], pos, has_gauss, cached gauss
COMM_ID_BYTES = 128
MC_KINDS = {"european": 0, "asian": 1, "up_and_out": 2, "down_and_out": 3}   # DH_MC_*
MC_MAX_OPTIONS = 64            # DH_MC_MAX_OPTIONS
MC_POISSON_CAP = 16            # DH_MC_POISSON_CAP
MC_VR_ANTITHETIC, MC_VR_CONTROL = 1, 2     # DH_MC_VR_*: the flags of dh_mc_price_vr
MC_VR_COS_N, MC_VR_COS_L = 256, 10.0       # DH_MC_VR_COS_*: the COS series of the control means
# the planes of dh_mc_greeks, in the order of the header's DH_MC_GREEK_* enum (DH_MC_N_GREEKS)
MC_GREEKS = ("price", "delta", "gamma", "vega_v01", "vega_v02")
LSM_MAX_OPTIONS = 16           # DH_LSM_MAX_OPTIONS
LSM_BASIS = 10                 # DH_LSM_BASIS: regression terms
LSM_MIN_ITM = 64               # DH_LSM_MIN_ITM: in-the-money paths a date needs to be fitted
LSM_SLOTS = 128                # DH_LSM_SLOTS: blocks per (set, option) of a backward launch
LSM_MAX_GIB = 16               # DH_LSM_MAX_GIB: cap of the path store
FFN_OUT = 13                   # DH_FFN_OUT: the warm-start network's outputs, the optimiser's x
FFN_TM = 32                    # DH_FFN_TM: markets per block of ffn_forward_kernel
FFN_MAX_HIDDEN = 6             # DH_FFN_MAX_HIDDEN
FFN_MAX_WIDTH = 512            # DH_FFN_MAX_WIDTH: hidden widths are multiples of 32 up to this
FFN_MAX_IN = 64                # DH_FFN_MAX_IN: features and prices per market at most
STAMPS_PER_BLOCK = 32          # kStamps of the DH_STAMPS build (csrc/dh_kernels.hip)
# the planes of dh_surface_greeks / dh_greeks_pairs, in the order of the header's DH_GREEK_* enum
GREEKS = ("price", "delta", "gamma", "dual_delta", "vega1", "vega2")
# the planes of dh_surface_greeks_full / dh_greeks_full_pairs: GREEKS, then DH_GREEK_DPRICE_DT ...
# DH_GREEK_LOCAL_VAR (DH_N_GREEKS_FULL planes)
GREEKS_FULL = GREEKS + ("dprice_dT", "rho", "dual_gamma", "local_var")
# the planes of dh_surface_param_sens / dh_param_sens_pairs: the price, then the record's thirteen
# model parameters (DH_N_PARAM_SENS planes); the longest series they take (DH_PARAM_GRAD_MAX_N)
PARAM_SENS = ("price", "v1_0", "kappa1", "theta1", "sigma1", "rho1", "v2_0", "kappa2", "theta2",
              "sigma2", "rho2", "lambda_j", "mu_j", "sigma_j")
PARAM_GRAD_MAX_N = 1024
# dh_lb_result.task of a Levenberg-Marquardt start (the header's DH_LM_* enum) -> its message
LM_MESSAGES = {1: "CONVERGENCE: MAX GRADIENT COMPONENT <= GTOL",
               2: "CONVERGENCE: RELATIVE REDUCTION OF F <= FTOL",
               3: "CONVERGENCE: STEP <= XTOL",
               4: "STOP: ACCEPTED STEPS REACHED MAXITER",
               5: "STOP: REQUESTS REACHED MAXFUN",
               6: "ABNORMAL: DAMPING PAST ITS CEILING",
               7: "ABNORMAL: INVALID LOSS AT X0"}

_dp = C.POINTER(C.c_double)
_i8p = C.POINTER(C.c_int8)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u32p = C.POINTER(C.c_uint32)
_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p


class LbOptions(C.Structure):
    """dh_lb_options (include/dhcos.h)."""
    _fields_ = [("maxiter", C.c_int32), ("maxfun", C.c_int32), ("maxls", C.c_int32),
                ("chunk", C.c_int32), ("ftol", C.c_double), ("gtol", C.c_double)]


class LbResult(C.Structure):
    """dh_lb_result (include/dhcos.h): one finished L-BFGS-B start."""
    _fields_ = [("x", C.c_double * 13), ("fun", C.c_double), ("best_loss", C.c_double),
                ("t_done", C.c_double), ("nit", C.c_int32), ("nfev", C.c_int32),
                ("task", C.c_int32), ("warnflag", C.c_int32), ("n_calls", C.c_int32),
                ("pad", C.c_int32)]


class McOption(C.Structure):
    """dh_mc_option (include/dhcos.h): one option of the Monte Carlo pricer."""
    _fields_ = [("kind", C.c_int32), ("is_call", C.c_int32), ("strike", C.c_double),
                ("maturity", C.c_double), ("barrier", C.c_double)]


class LsmOption(C.Structure):
    """dh_lsm_option (include/dhcos.h): one American / Bermudan option of dh_lsm_price."""
    _fields_ = [("is_call", C.c_int32), ("pad", C.c_int32), ("strike", C.c_double),
                ("maturity", C.c_double)]


_int, _i64, _dbl = C.c_int, C.c_int64, C.c_double          # the header's int, int64_t, double
_lbo, _lbr, _mco = C.POINTER(LbOptions), C.POINTER(LbResult), C.POINTER(McOption)
_lso = C.POINTER(LsmOption)

# name -> (restype, argtypes); mirrors include/dhcos.h one to one, in its order
SIGNATURES = {
    # ---- context
    "dh_version": (_int, []),
    "dh_last_error": (C.c_char_p, []),
    "dh_device_count": (_int, [_i32p]),
    "dh_ctx_create": (_int, [_int, C.POINTER(_vp)]),
    "dh_ctx_destroy": (_int, [_vp]),
    "dh_ctx_synchronize": (_int, [_vp]),
    "dh_ctx_stream": (_vp, [_vp]),
    "dh_ctx_set_exact": (_int, [_vp, _int]),
    "dh_ctx_set_tail_cut": (_int, [_vp, _int]),
    "dh_ctx_set_path": (_int, [_vp, _int]),
    "dh_ctx_last_path": (_int, [_vp]),
    "dh_ctx_debug_stamps": (_int, [_vp, _int]),
    "dh_ctx_read_stamps": (_int, [_vp, C.POINTER(C.c_ulonglong), _i64, _i64p]),
    # ---- option surfaces
    "dh_surface_create": (_int, [_vp, _dp, _dp, _i8p, _dp, _int, _int, C.POINTER(_vp)]),
    "dh_surface_destroy": (_int, [_vp]),
    "dh_surface_size": (_int, [_vp, _i32p, _i32p]),
    "dh_surface_stage_spot": (_int, [_vp, _dbl]),
    "dh_surface_price": (_int, [_vp, _vp, _dp, _i64, _int, _dbl, _dp]),
    "dh_surface_price_cols": (_int, [_vp, _vp, _dp, _dp, _dbl, _i64, _int, _dbl, _dp]),
    "dh_host_register": (_int, [_vp, C.c_size_t]),
    "dh_host_unregister": (_int, [_vp]),
    # the per-iteration calibration call takes raw addresses (ndarray.ctypes.data): half the
    # marshalling cost of data_as() pointers
    "dh_surface_loss": (_int, [_vp, _vp, _vp, _int, _int, _dbl, _vp, _vp, _vp]),
    "dh_surface_price_dev": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp, _vp]),
    "dh_surface_loss_dev": (_int, [_vp, _vp, _vp, _int, _int, _dbl, _vp, _vp, _vp, _vp]),
    "dh_surface_fg": (_int, [_vp, _vp, _vp, _vp, _int, _dbl, _dbl, _int, _dbl, _vp, _vp, _vp]),
    "dh_surface_fg_begin": (_int, [_vp, _vp, _vp, _vp, _int, _dbl, _dbl, _int, _dbl, _int]),
    "dh_surface_fg_end": (_int, [_vp, _vp, _int, _int, _vp, _vp, _vp]),
    "dh_surface_fg_cancel": (_int, [_vp, _int]),
    # ---- device-resident multi-start L-BFGS-B
    "dh_calibrate_lbfgs": (_int, [_vp, _vp, _dp, _int, _dbl, _dbl, _int, _dbl, _lbo, _lbr,
                                  _i32p]),
    "dh_ctx_set_lb_trace": (_int, [_vp, _i64]),
    "dh_ctx_read_lb_trace": (_int, [_vp, _dp, _i64, _i64p]),
    # ---- one-shot forms
    "dh_price_batch": (_int, [_vp, _dp, _i64, _dp, _dp, _i8p, _int, _int, _dbl, _dp]),
    "dh_loss_batch": (_int, [_vp, _dp, _int, _dp, _dp, _i8p, _dp, _int, _dbl, _dbl, _int, _dbl,
                             _dp, _i32p]),
    # ---- generator batch path: host RNG
    "dh_gen_draw": (_int, [_u32p, _i32p, _i32p, _dp, _i64, _dp, _dp, _int, _dbl, _dbl, _dbl,
                           _dbl, _dbl, _dp, _dp, _dp]),
    "dh_gen_draw_progress": (_int, [_u32p, _i32p, _i32p, _dp, _i64, _dp, _dp, _int, _dbl, _dbl,
                                    _dbl, _dbl, _dbl, _dp, _dp, _dp, _i64p]),
    # ---- sharded draw
    "dh_gen_locate": (_int, [_u32p, _i32p, _i32p, _dp, _i64, _int, _vp, _i64, _dp]),
    "dh_gen_draw_located": (_int, [_dp, _vp, _i64, _i64, _dp, _dp, _int, _dbl, _dbl, _dbl, _dp,
                                   _dp, _dp]),
    "dh_gen_sweep": (_int, [_dp, _dp, _i64, _i64, _dbl, _dbl, _dp]),
    "dh_gen_drawn_samples": (_int, [_i64p]),
    "dh_gen_dates": (_int, [_i64, _i64, _vp]),
    "dh_gen_assemble": (_int, [_dp, _dp, _dp, _dp, _i64, _int, _dp, _dp, _dp]),
    "dh_gen_device": (_int, [_vp, _vp, _u32p, _i32p, _i32p, _dp, _i64, _dp, _dp, _dbl, _dbl,
                             _dbl, _dbl, _dbl, _dbl, _int, _dbl, _dp, _i64, _vp, _vp, _vp, _vp,
                             _vp, _vp, _vp, _dp]),
    "dh_gen_log": (_int, [_vp, _vp, _i64, _vp]),
    "dh_math_probe": (_int, [_vp, _int, _vp, _vp, _i64, _vp, _vp]),
    "dh_host_alloc": (_int, [C.c_size_t, C.POINTER(_vp)]),
    "dh_host_free": (_int, [_vp]),
    "dh_host_cache_trim": (_int, []),
    # ---- paired pricing
    "dh_price_pairs": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _dbl, _vp]),
    # ---- analytic Greeks of the COS price
    "dh_surface_greeks": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp]),
    "dh_surface_greeks_dev": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp, _vp]),
    "dh_greeks_pairs": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _dbl, _vp]),
    # ---- the full Greeks: maturity, rate, dual gamma, local variance
    "dh_surface_greeks_full": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp]),
    "dh_surface_greeks_full_dev": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp, _vp]),
    "dh_greeks_full_pairs": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _dbl, _vp]),
    # ---- analytic parameter sensitivities, the loss and its gradient
    "dh_surface_param_sens": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp]),
    "dh_surface_param_sens_dev": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp, _vp]),
    "dh_param_sens_pairs": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _dbl, _vp]),
    "dh_surface_loss_grad": (_int, [_vp, _vp, _vp, _int, _dbl, _dbl, _int, _dbl, _vp, _vp, _vp]),
    "dh_surface_loss_grad_dev": (_int, [_vp, _vp, _vp, _int, _dbl, _dbl, _int, _dbl, _vp, _vp,
                                        _vp, _vp]),
    "dh_surface_loss_grad_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int,
                                         _dbl, _vp, _vp, _vp]),
    "dh_surface_loss_grad_rows_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _dbl,
                                             _vp, _vp, _vp, _vp]),
    # ---- Black-Scholes implied volatility
    "dh_implied_vol": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "dh_implied_vol_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "dh_surface_implied_vol": (_int, [_vp, _vp, _vp, _i64, _int, _dbl, _vp, _vp]),
    # ---- calibration objective in implied-vol space
    "dh_surface_set_iv_market": (_int, [_vp, _vp, _vp]),
    "dh_surface_iv_sse_dev": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
    "dh_surface_loss_iv_dev": (_int, [_vp, _vp, _vp, _int, _int, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "dh_surface_loss_iv": (_int, [_vp, _vp, _vp, _int, _int, _dbl, _vp, _vp, _vp, _vp]),
    # ---- many markets on one option grid
    "dh_surface_loss_rows_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp]),
    "dh_surface_loss_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _dbl, _vp, _vp,
                                    _vp]),
    "dh_calibrate_lbfgs_batch": (_int, [_vp, _vp, _dp, _dp, _dp, _int, _dp, _i32p, _int, _int,
                                        _dbl, _lbo, _lbr, _i32p]),
    # ---- many markets on one grid, in implied-vol space
    "dh_surface_iv_sse_rows_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp,
                                          _vp]),
    "dh_surface_loss_iv_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _dbl, _vp,
                                       _vp, _vp, _vp]),
    "dh_calibrate_lbfgs_batch_iv": (_int, [_vp, _vp, _dp, _dp, _dp, _dp, _int, _dp, _i32p, _int,
                                           _int, _dbl, _lbo, _lbr, _i32p]),
    # ---- many markets on one grid, with the analytic gradient
    "dh_calibrate_lbfgs_batch_grad": (_int, [_vp, _vp, _dp, _dp, _dp, _int, _dp, _i32p, _int,
                                             _int, _dbl, _lbo, _lbr, _i32p]),
    # ---- the vol objective with its exact gradient
    "dh_surface_iv_grad_rows_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp,
                                           _vp, _vp, _vp, _vp, _vp]),
    "dh_surface_loss_iv_grad_rows_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int,
                                                _int, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "dh_surface_loss_iv_grad_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int,
                                            _int, _dbl, _vp, _vp, _vp, _vp]),
    "dh_calibrate_lbfgs_batch_iv_grad": (_int, [_vp, _vp, _dp, _dp, _dp, _dp, _int, _dp, _i32p,
                                                _int, _int, _dbl, _lbo, _lbr, _i32p]),
    # ---- Gauss-Newton Hessian and Levenberg-Marquardt
    "dh_surface_gauss_newton_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int,
                                            _dbl, _vp, _vp, _vp, _vp]),
    "dh_surface_gauss_newton_rows_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int,
                                                _dbl, _vp, _vp, _vp, _vp, _vp]),
    "dh_calibrate_lm_batch": (_int, [_vp, _vp, _dp, _dp, _dp, _int, _dp, _i32p, _int, _int, _dbl,
                                     _lbo, _lbr, _i32p]),
    # ---- warm-start network
    "dh_ffn_create": (_int, [_vp, _int, _i32p, _f32p, _f32p, _dp, _int, _dp, _dp, _dp, _dp,
                             C.POINTER(_vp)]),
    "dh_ffn_destroy": (_int, [_vp]),
    "dh_ffn_forward": (_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "dh_ffn_forward_dev": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    # ---- building blocks
    "dh_cf": (_int, [_vp, _dp, _dp, _int, _dbl, _dp, _dp]),
    "dh_cf_complex": (_int, [_vp, _dp, _dp, _dp, _int, _dbl, _dp, _dp]),
    "dh_trunc_range": (_int, [_vp, _dp, _dp, _dp, _i64, _dbl, _dp, _dp]),
    "dh_cos_coeffs": (_int, [_vp, _i32p, _int, _dbl, _dbl, _dbl, _dbl, _dp, _dp]),
    # ---- multi-GPU: RCCL communicator
    "dh_comm_id": (_int, [_vp]),
    "dh_comm_create": (_int, [_vp, _vp, _int, _int, C.POINTER(_vp)]),
    "dh_comm_destroy": (_int, [_vp]),
    "dh_comm_broadcast": (_int, [_vp, _vp, _i64, _int]),
    "dh_comm_allgather": (_int, [_vp, _vp, _i64, _vp]),
    "dh_allgather_best": (_int, [_vp, _vp, _int, _int, _int, _int, _vp, _i32p]),
    "dh_best_start": (_int, [_vp, _i64, _int, _int, _int, _i32p]),
    # ---- Monte Carlo path pricer
    "dh_mc_price": (_int, [_vp, _vp, _i64, _mco, _int, _i64, _int, C.c_uint64, _vp, _vp]),
    "dh_mc_price_dev": (_int, [_vp, _vp, _i64, _mco, _int, _i64, _int, C.c_uint64, _vp, _vp,
                               _vp]),
    "dh_mc_paths": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _i64, _int, C.c_uint64, _vp]),
    # ---- its antithetic pairs and control variates
    "dh_mc_price_vr": (_int, [_vp, _vp, _i64, _mco, _int, _i64, _int, C.c_uint64, _int, _vp, _vp,
                              _vp, _vp, _vp, _vp]),
    "dh_mc_price_vr_dev": (_int, [_vp, _vp, _i64, _mco, _int, _i64, _int, C.c_uint64, _int, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_mc_paths_vr": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _i64, _int, C.c_uint64, _int,
                              _vp]),
    # ---- its delta, gamma and v0 vegas from coupled paths
    "dh_mc_greeks": (_int, [_vp, _vp, _i64, _mco, _int, _i64, _int, C.c_uint64, _dbl, _dbl, _vp,
                            _vp]),
    "dh_mc_greeks_dev": (_int, [_vp, _vp, _i64, _mco, _int, _i64, _int, C.c_uint64, _dbl, _dbl,
                                _vp, _vp, _vp]),
    # ---- American and Bermudan options by least-squares Monte Carlo
    "dh_lsm_price": (_int, [_vp, _vp, _i64, _lso, _int, _i64, _int, _int, C.c_uint64, _vp, _vp,
                            _vp, _vp, _vp, _vp]),
    "dh_lsm_price_dev": (_int, [_vp, _vp, _i64, _lso, _int, _i64, _int, _int, C.c_uint64, _vp, _vp,
                                _vp, _vp, _vp, _vp, _vp]),
}


class NativeError(RuntimeError):
    """Raised for any failure of the native (HIP) path; there is no fallback."""


_lib = None
_lib_lock = threading.Lock()


def load():
    """Load libdhcos.so (once) and attach the C signatures."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NativeError(
                    f"libdhcos.so not found at {LIB_PATH}; build it with "
                    "`make -C option-pricing-ffn-lbfgs_amd/csrc` (hipcc, gfx950)")
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def _check(rc):
    if rc != 0:
        msg = load().dh_last_error()
        raise NativeError(f"libdhcos error {rc}: {msg.decode() if msg else ''}")


def runtime_shared_with_torch() -> bool:
    """True unless two different libamdhip64 images are mapped into this process."""
    try:
        with open("/proc/self/maps") as fh:
            paths = {ln.split()[-1] for ln in fh if "libamdhip64" in ln}
    except OSError:
        return True
    return len({os.path.realpath(p) for p in paths}) <= 1


def device_count() -> int:
    n = C.c_int32(0)
    rc = load().dh_device_count(C.byref(n))
    return n.value if rc == 0 else 0


# ---- marshalling steps shared by the wrappers below: a _vp argument of SIGNATURES takes a raw
# address (ndarray.ctypes.data, a device address, _addr() where it may be NULL), a typed pointer
# argument takes _ptr()
def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a, ty=_dp):
    return a.ctypes.data_as(ty)


def _records(a):
    """Param records as a contiguous float64 [P, PARAM_STRIDE]."""
    return _f64(a).reshape(-1, PARAM_STRIDE)


def _flags(is_call, n):
    """Option flags (call = non-zero) as a contiguous int8 [n]."""
    return np.ascontiguousarray(is_call, dtype=np.int8).reshape(n)


def _addr(a, n=1):
    """Raw address of ndarray / integer address a, or None (NULL) if a is None or 0, or n is 0."""
    if a is None or not n:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else (int(a) or None)


def _out_array(a, shape, exc, msg, writeable=True):
    """a if a C-contiguous (writeable) float64 ndarray of shape, else exc(msg); None: a new one."""
    if a is None:
        return np.empty(shape)
    if (not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shape
            or not a.flags.c_contiguous or (writeable and not a.flags.writeable)):
        raise exc(msg)
    return a


def _fd_model(model, S):
    """An FD request's ``model`` (None, or [2, S, 13]) as a contiguous float64 array."""
    if model is not None:
        model = _f64(model)
        if model.shape != (2, S, 13):
            raise ValueError(f"model must be [2, {S}, 13], got {model.shape}")
    return model


def _stream_handle(who, stream):
    """stream (a torch stream, a raw hipStream_t, None) as a raw handle: None -> 0, null refused."""
    st = 0 if stream is None else int(getattr(stream, "cuda_stream", stream))
    if stream is not None and st == 0:
        raise ValueError(f"{who}: the default (null) stream cannot be named; pass a "
                         "non-default stream, or None for the context's stream")
    return st


def _loss_outputs(S, M, want_prices, want_iv=None):
    """-> sse [S], n_bad [S], prices, iv [S, M] (None unless wanted) and the wrapper's return tuple:
    (sse, n_bad, prices or None) in price space (want_iv None), only what is wanted in vol space."""
    outs = (np.empty(S), np.empty(S, dtype=np.int32),
            np.empty((S, M)) if want_prices else None, np.empty((S, M)) if want_iv else None)
    return (*outs, outs[:3] if want_iv is None else tuple(o for o in outs if o is not None))


def _lbfgs(name, ctx, surf, S, args, maxiter, maxfun, maxls, chunk, ftol, gtol):
    """Run a dh_calibrate_lbfgs* export; args: those between surface and options -> (results, n)."""
    opt = LbOptions(int(maxiter), int(maxfun), int(maxls), int(chunk), float(ftol), float(gtol))
    res = (LbResult * max(S, 1))()
    nl = C.c_int32(0)
    with ctx._lock:
        _check(getattr(load(), name)(ctx.handle, surf.handle, *args, C.byref(opt), res,
                                     C.byref(nl)))
    return list(res)[:S], nl.value


class _RngState:
    """NumPy's legacy RandomState state (np.random's, or a ``get_state()``-style tuple) as the
    cells the dh_gen_* exports advance in place: key [624] uint32, pos, has_gauss, cached."""

    def __init__(self, state=None):
        name, key, pos, has_gauss, cached = np.random.get_state() if state is None else state
        if name != "MT19937":
            raise NativeError(f"unsupported bit generator {name}")
        self.key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        self.pos, self.has_gauss = C.c_int32(int(pos)), C.c_int32(int(has_gauss))
        self.cached = C.c_double(float(cached))

    def args(self):
        """The four state arguments of a dh_gen_* export."""
        return (_ptr(self.key, _u32p), C.byref(self.pos), C.byref(self.has_gauss),
                C.byref(self.cached))

    def values(self):
        """-> (key, pos, has_gauss, cached) as advanced."""
        return self.key, self.pos.value, self.has_gauss.value, self.cached.value

    def restore(self):
        """Make the advanced state np.random's."""
        np.random.set_state(("MT19937",) + self.values())


class _Handle:
    """Owner of one library object, its handle in ``_h`` (None once closed): the ``handle``
    property, and the subclass's ``close()`` when the owner is collected."""
    _h = None

    @property
    def handle(self):
        return self._h

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """A device context: one HIP stream + grow-only device scratch (dh_ctx)."""

    def __init__(self, device: int = 0):
        lib = load()
        h = _vp()
        _check(lib.dh_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._lock = threading.Lock()
        # the request slots of dh_surface_fg_begin / _end belong to the context: the start
        # count of the request in flight in each (None = idle), which sizes fg_end's outputs
        self._fg_s = [None] * FG_SLOTS
        self._settings = {}            # set_exact / set_tail_cut / set_path, for slot contexts

    @property
    def stream(self) -> int:
        return load().dh_ctx_stream(self._h) or 0

    def set_exact(self, on: bool):
        """Validation mode: price every option by the per-term reference-order path."""
        _check(load().dh_ctx_set_exact(self._h, 1 if on else 0))
        self._settings["set_exact"] = bool(on)

    def set_tail_cut(self, on: bool):
        """Adaptive tail of the angle sums (default on); off sums every term k < N."""
        _check(load().dh_ctx_set_tail_cut(self._h, 1 if on else 0))
        self._settings["set_tail_cut"] = bool(on)

    def set_path(self, path: int):
        """Request kernels: PATH_AUTO (default), PATH_SPLIT (table + option launches),
        or PATH_FUSED (one launch per request where every maturity group is one tile)."""
        _check(load().dh_ctx_set_path(self._h, int(path)))
        self._settings["set_path"] = int(path)

    @property
    def last_path(self) -> int:
        """PATH_FUSED, PATH_SPLIT or PATH_GEN: the kernels of the last fast-path request (0
        before any)."""
        return int(load().dh_ctx_last_path(self._h))

    def debug_stamps(self, on: bool):
        """Diagnostic build only: record per-block phase stamps of the next COS launches."""
        _check(load().dh_ctx_debug_stamps(self._h, 1 if on else 0))

    def read_stamps(self):
        n = C.c_int64(0)
        _check(load().dh_ctx_read_stamps(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            _check(load().dh_ctx_read_stamps(self._h, _ptr(out, C.POINTER(C.c_ulonglong)),
                                             n.value, C.byref(n)))
        return out.reshape(-1, STAMPS_PER_BLOCK)

    def set_lb_trace(self, cap: int):
        """Diagnostics: record up to cap consumed requests of the next calibrate_lbfgs calls."""
        _check(load().dh_ctx_set_lb_trace(self._h, int(cap)))

    def read_lb_trace(self):
        """-> [n, 40] records [start, request, f, x[13], g[13], 0, 0, 0, stamps[6], 0, 0] of the
        last call (stamps only in the DH_STAMPS build)."""
        n = C.c_int64(0)
        _check(load().dh_ctx_read_lb_trace(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 40))
        if n.value:
            _check(load().dh_ctx_read_lb_trace(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def synchronize(self):
        _check(load().dh_ctx_synchronize(self._h))

    def slot_context(self, k: int) -> "Context":
        """Request slot k's context for a pipelined host driver: this context for slot 0, else a
        context of its own on the same device, cached (its own stream and scratch, so two groups'
        requests may run on the GPU at once), carrying this context's settings (exact mode, tail
        cut, path)."""
        if k == 0:
            return self
        cache = self.__dict__.setdefault("_slot_ctxs", {})
        c = cache.get(k)
        if c is None:
            c = cache[k] = Context(self.device)
        for name, v in self._settings.items():
            if c._settings.get(name) != v:
                getattr(c, name)(v)
        return c

    def fg_cancel(self, slot):
        """dh_surface_fg_cancel: wait for slot's request (if any) and discard it."""
        with self._lock:
            try:
                _check(load().dh_surface_fg_cancel(self._h, int(slot)))
            finally:
                self._fg_s[int(slot)] = None

    def close(self):
        for surf in self.__dict__.pop("_grid_surfaces", {}).values():   # generator.price_grid's
            surf.close()
        for c in self.__dict__.pop("_slot_ctxs", {}).values():
            c.close()
        for ref in self.__dict__.pop("_ffns", []):      # networks resident on this context
            ffn = ref()
            if ffn is not None:
                ffn.close()
        if self._h:
            load().dh_ctx_destroy(self._h)
            self._h = None

    # ---- pricing primitives -------------------------------------------------------------
    def price_pairs(self, params, K, T, is_call, N=128, L=10.0):
        params = _records(params)
        P = params.shape[0]
        K, T = _f64(K).reshape(P), _f64(T).reshape(P)
        ic = _flags(is_call, P)
        out = np.empty(P)
        with self._lock:
            _check(load().dh_price_pairs(self._h, params.ctypes.data, K.ctypes.data, T.ctypes.data,
                                         ic.ctypes.data, P, int(N), float(L), out.ctypes.data))
        return out

    def greeks_pairs(self, params, K, T, is_call, N=128, L=10.0):
        """dh_greeks_pairs: the planes GREEKS of option i under param record i -> [6, n]."""
        params = _records(params)
        n = params.shape[0]
        K, T = _f64(K).reshape(n), _f64(T).reshape(n)
        ic = _flags(is_call, n)
        out = np.empty((len(GREEKS), n))
        with self._lock:
            _check(load().dh_greeks_pairs(self._h, _addr(params, n), _addr(K, n), _addr(T, n),
                                          _addr(ic, n), n, int(N), float(L), _addr(out, n)))
        return out

    def greeks_full_pairs(self, params, K, T, is_call, N=128, L=10.0):
        """dh_greeks_full_pairs: the planes GREEKS_FULL of option i under param record i
        -> [10, n]."""
        params = _records(params)
        n = params.shape[0]
        K, T = _f64(K).reshape(n), _f64(T).reshape(n)
        ic = _flags(is_call, n)
        out = np.empty((len(GREEKS_FULL), n))
        with self._lock:
            _check(load().dh_greeks_full_pairs(self._h, _addr(params, n), _addr(K, n), _addr(T, n),
                                               _addr(ic, n), n, int(N), float(L), _addr(out, n)))
        return out

    def param_sens_pairs(self, params, K, T, is_call, N=128, L=10.0):
        """dh_param_sens_pairs: the planes PARAM_SENS of option i under param record i
        -> [14, n]."""
        params = _records(params)
        n = params.shape[0]
        K, T = _f64(K).reshape(n), _f64(T).reshape(n)
        ic = _flags(is_call, n)
        out = np.empty((len(PARAM_SENS), n))
        with self._lock:
            _check(load().dh_param_sens_pairs(self._h, _addr(params, n), _addr(K, n), _addr(T, n),
                                              _addr(ic, n), n, int(N), float(L), _addr(out, n)))
        return out

    def price_batch(self, params, K, T, is_call, N=128, L=10.0):
        """dh_price_batch: out [P, M] for every (param set, option); a surface per call."""
        params = _records(params)
        P = params.shape[0]
        K, T = _f64(K).reshape(-1), _f64(T).reshape(-1)
        M = K.size
        ic = _flags(is_call, M)
        out = np.empty((P, M))
        with self._lock:
            _check(load().dh_price_batch(self._h, _ptr(params), P, _ptr(K), _ptr(T),
                                         _ptr(ic, _i8p), M, int(N), float(L), _ptr(out)))
        return out

    def loss_batch(self, X, K, T, is_call, mkt, S0, r, N=128, L=10.0):
        """dh_loss_batch: compute_loss of every row of unconstrained X [S, 13] over the market
        (K, T, is_call, mkt) -> (loss [S], n_invalid [S]); a surface per call."""
        X = _f64(X).reshape(-1, 13)
        S = X.shape[0]
        K, T, mkt = _f64(K).reshape(-1), _f64(T).reshape(-1), _f64(mkt).reshape(-1)
        M = K.size
        ic = _flags(is_call, M)
        loss, bad = np.empty(S), np.empty(S, dtype=np.int32)
        with self._lock:
            _check(load().dh_loss_batch(self._h, _ptr(X), S, _ptr(K), _ptr(T), _ptr(ic, _i8p),
                                        _ptr(mkt), M, float(S0), float(r), int(N), float(L),
                                        _ptr(loss), _ptr(bad, _i32p)))
        return loss, bad

    def price_one(self, rec16, K, T, is_call, N=128, L=10.0):
        """One option under one param record (DoubleHeston.pricing): dh_price_pairs with P = 1,
        raw addresses (the per-call marshalling is most of a single price's host cost)."""
        rec = _f64(rec16)
        kt = np.array([K, T])
        ic = np.array([1 if is_call else 0], dtype=np.int8)
        out = np.empty(1)
        with self._lock:
            _check(load().dh_price_pairs(self._h, rec.ctypes.data, kt.ctypes.data,
                                         kt.ctypes.data + 8, ic.ctypes.data, 1, int(N), float(L),
                                         out.ctypes.data))
        return out[0]

    def implied_vol(self, price, S0, K, T, r, q, is_call):
        """dh_implied_vol: Black-Scholes implied vols of n quotes, every argument an array of n
        (float64; is_call int8 / bool) -> sigma [n] (NaN where no vol exists, include/dhcos.h)."""
        cols = [_f64(a).reshape(-1) for a in (price, S0, K, T, r, q)]
        n = cols[0].size
        ic = _flags(is_call, -1)
        if any(c.size != n for c in cols) or ic.size != n:
            raise ValueError("implied_vol: every argument must have the same length")
        out = np.empty(n)
        with self._lock:
            _check(load().dh_implied_vol(self._h, *(_addr(c, n) for c in cols), _addr(ic, n), n,
                                         _addr(out, n)))
        return out

    def _check_records_tensor(self, who, records):
        """The records of a ``*_dev`` call: a contiguous float64 [P, 16] torch tensor on this
        context's device."""
        import torch
        if (records.dtype != torch.float64 or not records.is_contiguous() or records.dim() != 2
                or records.shape[1] != PARAM_STRIDE or not records.is_cuda
                or records.device.index != self.device):
            raise ValueError(f"{who}: a contiguous float64 [P, {PARAM_STRIDE}] tensor on "
                             f"cuda:{self.device}")

    def mc_price(self, records, options, n_paths, steps_per_year, seed):
        """dh_mc_price: records [P, 16], options an array of McOption -> (price, stderr), each
        [P, n_options]."""
        rec = _records(records)
        P, n_opt = rec.shape[0], len(options)
        price, err = np.empty((P, n_opt)), np.empty((P, n_opt))
        with self._lock:
            _check(load().dh_mc_price(self._h, rec.ctypes.data, P, options, n_opt, int(n_paths),
                                      int(steps_per_year), int(seed), price.ctypes.data,
                                      err.ctypes.data))
        return price, err

    def mc_price_dev(self, records, options, n_paths, steps_per_year, seed, stream=None):
        """dh_mc_price_dev: records a contiguous float64 [P, 16] torch tensor on this context's
        device -> (price, stderr) tensors [P, n_options], enqueued on ``stream`` (None: the
        context's own; the null stream cannot be named, as implied_vol_dev) without
        synchronisation."""
        import torch
        self._check_records_tensor("mc_price_dev", records)
        P, n_opt = records.shape[0], len(options)
        out = torch.empty((2, P, n_opt), dtype=torch.float64, device=records.device)
        st = _stream_handle("mc_price_dev", stream)
        with self._lock:
            _check(load().dh_mc_price_dev(self._h, records.data_ptr(), P, options, n_opt,
                                          int(n_paths), int(steps_per_year), int(seed),
                                          out[0].data_ptr(), out[1].data_ptr(), _addr(st)))
        return out[0], out[1]

    def mc_paths(self, records, obs_steps, path0, n_paths, steps_per_year, seed):
        """dh_mc_paths: records [P, 16], obs_steps int32 [n_obs] -> [P, n_paths, n_obs, 6]
        (S, v1, v2, running max, min, sum)."""
        rec = _records(records)
        obs = np.ascontiguousarray(obs_steps, dtype=np.int32).reshape(-1)
        out = np.empty((rec.shape[0], int(n_paths), obs.size, 6))
        with self._lock:
            _check(load().dh_mc_paths(self._h, rec.ctypes.data, rec.shape[0], obs.size,
                                      obs.ctypes.data, int(path0), int(n_paths),
                                      int(steps_per_year), int(seed), out.ctypes.data))
        return out

    def mc_price_vr(self, records, options, n_paths, steps_per_year, seed, flags):
        """dh_mc_price_vr: records [P, 16], options an array of McOption, flags of MC_VR_* ->
        (price, stderr, base_price, base_stderr, beta, control_mean), each [P, n_options]."""
        rec = _records(records)
        P, n_opt = rec.shape[0], len(options)
        out = np.empty((6, P, n_opt))
        with self._lock:
            _check(load().dh_mc_price_vr(self._h, rec.ctypes.data, P, options, n_opt,
                                         int(n_paths), int(steps_per_year), int(seed), int(flags),
                                         *(o.ctypes.data for o in out)))
        return tuple(out)

    def mc_price_vr_dev(self, records, options, n_paths, steps_per_year, seed, flags, stream=None):
        """dh_mc_price_vr_dev: records a contiguous float64 [P, 16] torch tensor on this context's
        device -> the six tensors of ``mc_price_vr``, enqueued on ``stream`` (None: the context's
        own; the null stream cannot be named, as mc_price_dev) without synchronisation."""
        import torch
        self._check_records_tensor("mc_price_vr_dev", records)
        P, n_opt = records.shape[0], len(options)
        out = torch.empty((6, P, n_opt), dtype=torch.float64, device=records.device)
        st = _stream_handle("mc_price_vr_dev", stream)
        with self._lock:
            _check(load().dh_mc_price_vr_dev(self._h, records.data_ptr(), P, options, n_opt,
                                             int(n_paths), int(steps_per_year), int(seed),
                                             int(flags), *(o.data_ptr() for o in out), _addr(st)))
        return tuple(out)

    def mc_paths_vr(self, records, obs_steps, path0, n_paths, steps_per_year, seed, mirror):
        """dh_mc_paths_vr: ``mc_paths`` of the paths' mirrors (``mirror``), or of the paths."""
        rec = _records(records)
        obs = np.ascontiguousarray(obs_steps, dtype=np.int32).reshape(-1)
        out = np.empty((rec.shape[0], int(n_paths), obs.size, 6))
        with self._lock:
            _check(load().dh_mc_paths_vr(self._h, rec.ctypes.data, rec.shape[0], obs.size,
                                         obs.ctypes.data, int(path0), int(n_paths),
                                         int(steps_per_year), int(seed), 1 if mirror else 0,
                                         out.ctypes.data))
        return out

    def mc_greeks(self, records, options, n_paths, steps_per_year, seed, spot_bump, v0_bump):
        """dh_mc_greeks: records [P, 16], options an array of McOption -> (value, stderr), each
        [P, n_options, len(MC_GREEKS)]."""
        rec = _records(records)
        P, n_opt = rec.shape[0], len(options)
        out = np.empty((2, P, n_opt, len(MC_GREEKS)))
        with self._lock:
            _check(load().dh_mc_greeks(self._h, rec.ctypes.data, P, options, n_opt, int(n_paths),
                                       int(steps_per_year), int(seed), float(spot_bump),
                                       float(v0_bump), out[0].ctypes.data, out[1].ctypes.data))
        return out[0], out[1]

    def mc_greeks_dev(self, records, options, n_paths, steps_per_year, seed, spot_bump, v0_bump,
                      stream=None):
        """dh_mc_greeks_dev: records a contiguous float64 [P, 16] torch tensor on this context's
        device -> (value, stderr) tensors [P, n_options, len(MC_GREEKS)], enqueued on ``stream``
        (None: the context's own; the null stream cannot be named, as mc_price_dev) without
        synchronisation."""
        import torch
        self._check_records_tensor("mc_greeks_dev", records)
        P, n_opt = records.shape[0], len(options)
        out = torch.empty((2, P, n_opt, len(MC_GREEKS)), dtype=torch.float64,
                          device=records.device)
        st = _stream_handle("mc_greeks_dev", stream)
        with self._lock:
            _check(load().dh_mc_greeks_dev(self._h, records.data_ptr(), P, options, n_opt,
                                           int(n_paths), int(steps_per_year), int(seed),
                                           float(spot_bump), float(v0_bump), out[0].data_ptr(),
                                           out[1].data_ptr(), _addr(st)))
        return out[0], out[1]

    def lsm_price(self, records, options, dates, n_paths, steps_per_year, exercise_every, seed,
                  policy=False):
        """dh_lsm_price: records [P, 16], options an array of LsmOption, dates the largest number
        of exercise dates of an option -> (price, stderr, european, european_stderr), each
        [P, n_options], then coefficients [P, n_options, dates, LSM_BASIS] and exercise_date int32
        [P, n_options, n_paths], both None unless ``policy``."""
        rec = _records(records)
        P, n_opt = rec.shape[0], len(options)
        out = np.empty((4, P, n_opt))
        coef = np.empty((P, n_opt, int(dates), LSM_BASIS)) if policy else None
        tau = np.empty((P, n_opt, int(n_paths)), dtype=np.int32) if policy else None
        with self._lock:
            _check(load().dh_lsm_price(self._h, rec.ctypes.data, P, options, n_opt, int(n_paths),
                                       int(steps_per_year), int(exercise_every), int(seed),
                                       *(o.ctypes.data for o in out), _addr(coef), _addr(tau)))
        return out[0], out[1], out[2], out[3], coef, tau

    def lsm_price_dev(self, records, options, dates, n_paths, steps_per_year, exercise_every,
                      seed, policy=False, stream=None):
        """dh_lsm_price_dev: records a contiguous float64 [P, 16] torch tensor on this context's
        device -> the tensors of ``lsm_price``, enqueued on ``stream`` (None: the context's own;
        the null stream cannot be named, as mc_price_dev) without synchronisation."""
        import torch
        self._check_records_tensor("lsm_price_dev", records)
        P, n_opt = records.shape[0], len(options)
        out = torch.empty((4, P, n_opt), dtype=torch.float64, device=records.device)
        coef = tau = None
        if policy:
            coef = torch.empty((P, n_opt, int(dates), LSM_BASIS), dtype=torch.float64,
                               device=records.device)
            tau = torch.empty((P, n_opt, int(n_paths)), dtype=torch.int32, device=records.device)
        st = _stream_handle("lsm_price_dev", stream)
        with self._lock:
            _check(load().dh_lsm_price_dev(
                self._h, records.data_ptr(), P, options, n_opt, int(n_paths), int(steps_per_year),
                int(exercise_every), int(seed), *(o.data_ptr() for o in out),
                None if coef is None else coef.data_ptr(),
                None if tau is None else tau.data_ptr(), _addr(st)))
        return out[0], out[1], out[2], out[3], coef, tau

    def implied_vol_dev(self, price, S0, K, T, r, q, is_call, out=None, stream=None):
        """dh_implied_vol_dev over torch tensors on this context's device: float64 price, S0, K,
        T, r, q and int8 is_call, contiguous, all of n elements -> sigma (``out`` or a new
        float64 tensor).  One launch enqueued on ``stream`` -- a non-default torch stream or a raw
        hipStream_t; None: the context's own stream, as the other _dev wrappers (then order it
        against torch's work with ``synchronize()``) -- without synchronisation.  torch's default
        stream has the null handle, which the C-ABI reads as the context's stream: it is refused."""
        import torch
        cols = (price, S0, K, T, r, q)
        n = price.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=price.device)
        for t, dt in [(c, torch.float64) for c in cols + (out,)] + [(is_call, torch.int8)]:
            if (t.dtype != dt or not t.is_contiguous() or t.numel() != n or not t.is_cuda
                    or t.device.index != self.device):
                raise ValueError(f"implied_vol_dev: contiguous {dt} tensors of {n} elements on "
                                 f"cuda:{self.device}")
        st = _stream_handle("implied_vol_dev", stream)
        _check(load().dh_implied_vol_dev(self._h, *(c.data_ptr() for c in cols),
                                         is_call.data_ptr(), n, out.data_ptr(), _addr(st)))
        return out

    def ffn_forward_dev(self, ffn, market, spots, x0=None, raw=None, stream=None):
        """dh_ffn_forward_dev over torch tensors on this context's device: ``ffn`` an FFN of this
        context, market a contiguous float64 [B, M], spots float64 [B] -> x0 float64 [B, 13]
        (``x0`` or a new tensor); ``raw`` (a float32 [B, 13] tensor, or None) receives the
        network's standardised output.  One launch enqueued on ``stream`` (None: the context's
        own; the null stream cannot be named, as implied_vol_dev) without synchronisation and
        without a host round trip.  The values are the caller's promise: finite prices, spots
        > 0."""
        import torch
        if ffn.ctx is not self:
            raise ValueError("ffn_forward_dev: the network belongs to another context")
        B = market.shape[0] if market.dim() == 2 else -1
        if x0 is None:
            x0 = torch.empty((max(B, 0), FFN_OUT), dtype=torch.float64, device=market.device)
        want = [(market, torch.float64, (B, ffn.M)), (spots, torch.float64, (B,)),
                (x0, torch.float64, (B, FFN_OUT))]
        if raw is not None:
            want.append((raw, torch.float32, (B, FFN_OUT)))
        for t, dt, shape in want:
            if (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda
                    or t.device.index != self.device):
                raise ValueError(f"ffn_forward_dev: contiguous tensors on cuda:{self.device}: "
                                 f"market float64 [B, {ffn.M}], spots float64 [B], x0 float64 "
                                 f"[B, {FFN_OUT}], raw float32 [B, {FFN_OUT}]")
        st = _stream_handle("ffn_forward_dev", stream)
        _check(load().dh_ffn_forward_dev(ffn.handle, market.data_ptr(), spots.data_ptr(), B,
                                         x0.data_ptr(), None if raw is None else raw.data_ptr(),
                                         _addr(st)))
        return x0

    def cf(self, params16, u, tau):
        p = _f64(params16).reshape(PARAM_STRIDE)
        u = _f64(u).reshape(-1)
        re, im = np.empty(u.size), np.empty(u.size)
        with self._lock:
            _check(load().dh_cf(self._h, _ptr(p), _ptr(u), u.size, float(tau), _ptr(re), _ptr(im)))
        return re + 1j * im

    def cf_complex(self, params16, u, tau):
        """phi at complex frequencies u (dh_cf_complex)."""
        p = _f64(params16).reshape(PARAM_STRIDE)
        u = np.asarray(u, dtype=np.complex128).reshape(-1)
        ur, ui = _f64(u.real), _f64(u.imag)
        re, im = np.empty(u.size), np.empty(u.size)
        with self._lock:
            _check(load().dh_cf_complex(self._h, _ptr(p), _ptr(ur), _ptr(ui), u.size, float(tau),
                                        _ptr(re), _ptr(im)))
        return re + 1j * im

    def trunc_range(self, params, K, T, L=10.0):
        params = _records(params)
        P = params.shape[0]
        K, T = _f64(K).reshape(P), _f64(T).reshape(P)
        a, b = np.empty(P), np.empty(P)
        with self._lock:
            _check(load().dh_trunc_range(self._h, _ptr(params), _ptr(K), _ptr(T), P, float(L),
                                         _ptr(a), _ptr(b)))
        return a, b

    def cos_coeffs(self, k, c, d, a, b):
        k = np.ascontiguousarray(k, dtype=np.int32).reshape(-1)
        chi, psi = np.empty(k.size), np.empty(k.size)
        with self._lock:
            _check(load().dh_cos_coeffs(self._h, _ptr(k, _i32p), k.size, float(c), float(d),
                                        float(a), float(b), _ptr(chi), _ptr(psi)))
        return chi, psi


def lb_batch_args(M, mkt, spots, rates, x0s, market_of):
    """The arguments of dh_calibrate_lbfgs_batch as contiguous arrays, checked as the library
    checks them (shapes here, values there too): -> (mkt [B, M], spots [B], rates [B],
    x0s [S, 13], market_of [S] int32), or ValueError."""
    mkt = _f64(mkt)
    if mkt.ndim != 2 or mkt.shape[1] != M:
        raise ValueError(f"mkt must be [B, {M}], got {mkt.shape}")
    B = mkt.shape[0]
    spots = _f64(spots).reshape(-1)
    rates = _f64(rates).reshape(-1)
    if spots.size != B or rates.size != B:
        raise ValueError("mkt, spots and rates differ in length")
    if not (np.all(np.isfinite(spots)) and np.all(spots > 0)):
        raise ValueError("every spot must be finite and > 0")
    if not np.all(np.isfinite(rates)):
        raise ValueError("every rate must be finite")
    x0s = _f64(x0s).reshape(-1, 13)
    S = x0s.shape[0]
    mof = np.asarray(market_of).reshape(-1)
    if mof.size != S:
        raise ValueError("x0s and market_of differ in length")
    if S and (mof.dtype.kind not in "iu" or mof.min() < 0 or mof.max() >= B):
        raise ValueError(f"market_of must hold integers in [0, {B})")
    return mkt, spots, rates, x0s, np.ascontiguousarray(mof, dtype=np.int32)


def iv_rows(M, mkt_iv, weights):
    """Market vols [B, M] and weights ([B, M], [M] for every market, or None for all 1) of the
    vol-space rows as contiguous arrays, checked as dh_calibrate_lbfgs_batch_iv checks them:
    weights finite and >= 0 with a positive sum per market, vols finite and >= 0 wherever the
    weight is positive (anything where it is 0).  -> (mkt_iv [B, M], weights [B, M]), or
    ValueError naming the (market, option) pairs."""
    iv = _f64(mkt_iv)
    if iv.ndim != 2 or iv.shape[1] != M:
        raise ValueError(f"market vols must be [B, {M}], got {iv.shape}")
    B = iv.shape[0]
    if weights is None:
        w = np.ones((B, M))
    else:
        w = _f64(weights)
        if w.shape == (M,):
            w = np.ascontiguousarray(np.broadcast_to(w, (B, M)))
        elif w.shape != (B, M):
            raise ValueError(f"vol weights must be [{M}] or [{B}, {M}], got {w.shape}")
    wrong = np.argwhere(~(np.isfinite(w) & (w >= 0)))
    if wrong.size:
        raise ValueError("vol weights must be finite and non-negative; (market, option) "
                         f"{wrong[:8].tolist()}")
    if M:
        zero = np.flatnonzero(~(w.sum(axis=1) > 0))
        if zero.size:
            raise ValueError(f"the vol weights of market(s) {zero[:8].tolist()} sum to zero")
    wrong = np.argwhere((w > 0) & ~(np.isfinite(iv) & (iv >= 0)))
    if wrong.size:
        raise ValueError(
            f"no implied vol for (market, option) {wrong[:8].tolist()}"
            f"{' ...' if len(wrong) > 8 else ''} (price outside its no-arbitrage bounds, or a "
            "non-finite vol); give them iv_weights of 0")
    return iv, w


class FFN(_Handle):
    """The warm-start network resident on a context's device (dh_ffn): widths = (F, hidden ...,
    13), weights / biases the layers' float32 W_l [out, in] and b_l [out] with BatchNorm folded
    in, C the float64 feature matrix [F, M], and the four standardisation vectors."""

    def __init__(self, ctx: Context, widths, weights, biases, C_mat, x_mean, x_std, y_mean, y_std):
        self.ctx = ctx
        widths = np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)
        n_layers = widths.size - 1
        if len(weights) != n_layers or len(biases) != n_layers:
            raise ValueError("one weight matrix and one bias per layer")
        ws, bs = [], []
        for l, (w, b) in enumerate(zip(weights, biases)):
            w, b = np.asarray(w), np.asarray(b)
            if (w.dtype != np.float32 or b.dtype != np.float32
                    or w.shape != (widths[l + 1], widths[l]) or b.shape != (widths[l + 1],)):
                raise ValueError(f"layer {l}: float32 W [{widths[l + 1]}, {widths[l]}] and b "
                                 f"[{widths[l + 1]}], got {w.dtype} {w.shape}, {b.dtype} {b.shape}")
            ws.append(np.ascontiguousarray(w).reshape(-1))
            bs.append(np.ascontiguousarray(b))
        w_all, b_all = np.concatenate(ws), np.concatenate(bs)
        C_mat = _f64(C_mat)
        if C_mat.ndim != 2 or C_mat.shape[0] != widths[0]:
            raise ValueError(f"C must be [{widths[0]}, M], got {C_mat.shape}")
        self.F, self.M = int(C_mat.shape[0]), int(C_mat.shape[1])
        stats = [_f64(a).reshape(-1) for a in (x_mean, x_std, y_mean, y_std)]
        if [a.size for a in stats] != [self.F, self.F, FFN_OUT, FFN_OUT]:
            raise ValueError(f"x_mean, x_std must be [{self.F}], y_mean, y_std [{FFN_OUT}]")
        h = _vp()
        with ctx._lock:
            _check(load().dh_ffn_create(ctx.handle, n_layers, _ptr(widths, _i32p),
                                        _ptr(w_all, _f32p), _ptr(b_all, _f32p), _ptr(C_mat),
                                        self.M, *(_ptr(a) for a in stats), C.byref(h)))
        self._h = h
        # the context destroys what lives on it: Context.close() closes this object first
        ctx.__dict__.setdefault("_ffns", []).append(weakref.ref(self))

    def close(self):
        if self._h:
            load().dh_ffn_destroy(self._h)
            self._h = None

    def forward(self, market, spots, want_raw=False):
        """dh_ffn_forward: market [B, M], spots [B] -> x0 float64 [B, 13], and the network's
        standardised float32 output [B, 13] with ``want_raw``."""
        market = _f64(market)
        if market.ndim != 2 or market.shape[1] != self.M:
            raise ValueError(f"market must be [B, {self.M}], got {market.shape}")
        B = market.shape[0]
        spots = _f64(spots).reshape(-1)
        if spots.size != B:
            raise ValueError("market and spots differ in length")
        x0 = np.empty((B, FFN_OUT))
        raw = np.empty((B, FFN_OUT), dtype=np.float32) if want_raw else None
        with self.ctx._lock:
            _check(load().dh_ffn_forward(self._h, _addr(market, B), _addr(spots, B), B,
                                         _addr(x0, B), _addr(raw, B)))
        return (x0, raw) if want_raw else x0


class Surface(_Handle):
    """An option set resident in HBM, grouped by maturity into <=256-option tiles (dh_surface)."""

    def __init__(self, ctx: Context, K, T, is_call, mkt=None, strike_mode=STRIKE_ABSOLUTE):
        self.ctx = ctx
        K, T = _f64(K).reshape(-1), _f64(T).reshape(-1)
        M = K.size
        if T.size != M:
            raise ValueError("K and T differ in length")
        ic = _flags(is_call, M)
        mk = None if mkt is None else _f64(mkt).reshape(M)
        h = _vp()
        _check(load().dh_surface_create(ctx.handle, _ptr(K), _ptr(T), _ptr(ic, _i8p),
                                        None if mk is None else _ptr(mk), M, int(strike_mode),
                                        C.byref(h)))
        self._h = h
        self.M = M
        m, nt = C.c_int32(0), C.c_int32(0)
        _check(load().dh_surface_size(h, C.byref(m), C.byref(nt)))
        self.n_tiles = nt.value

    def close(self):
        if self._h:
            load().dh_surface_destroy(self._h)
            self._h = None

    def stage_spot(self, S0):
        """dh_surface_stage_spot: form log(K / S0) and K / S0 of every option once; fused request
        blocks whose record carries exactly this spot then load them (the same bits)."""
        with self.ctx._lock:
            _check(load().dh_surface_stage_spot(self._h, float(S0)))

    def _market_rows(self, mkt):
        """Market rows (prices or vols) as a contiguous float64 [B, M]."""
        return _f64(mkt).reshape(-1, self.M) if self.M else _f64(mkt).reshape(len(mkt), 0)

    def price(self, params, N=128, L=10.0, out=None):
        """Prices [P, M] of every param row (out: a C-contiguous float64 [P, M] to write into)."""
        params = _records(params)
        P = params.shape[0]
        out = _out_array(out, (P, self.M), ValueError,
                         f"out must be a writeable C-contiguous float64 [{P}, {self.M}]")
        with self.ctx._lock:
            _check(load().dh_surface_price(self.ctx.handle, self._h, _ptr(params), P, int(N),
                                           float(L), _ptr(out)))
        return out

    def price_cols(self, params, spots, r, N=128, L=10.0, out=None):
        """dh_surface_price_cols: prices [P, M] from model params [P, 13] and spots [P] (records
        formed on the device; out: a C-contiguous float64 [P, M] to write into)."""
        params = _f64(params).reshape(-1, 13)
        spots = _f64(spots).reshape(-1)
        P = params.shape[0]
        if spots.size != P:
            raise ValueError("params and spots differ in length")
        out = _out_array(out, (P, self.M), ValueError,
                         f"out must be a writeable C-contiguous float64 [{P}, {self.M}]")
        with self.ctx._lock:
            _check(load().dh_surface_price_cols(self.ctx.handle, self._h, _ptr(params),
                                                _ptr(spots), float(r), P, int(N), float(L),
                                                _ptr(out)))
        return out

    def loss_terms(self, params, N=128, L=10.0, want_prices=False):
        """-> (sse[S], n_bad[S], prices[S,M] or None)."""
        params = _records(params)
        S = params.shape[0]
        sse, bad, prices, _, ret = _loss_outputs(S, self.M, want_prices)
        with self.ctx._lock:
            _check(load().dh_surface_loss(self.ctx.handle, self._h, params.ctypes.data, S, int(N),
                                          float(L), sse.ctypes.data, bad.ctypes.data,
                                          None if prices is None else prices.ctypes.data))
        return ret

    def calibrate_lbfgs(self, x0s, S0, r, N=128, L=10.0, *, maxiter=300, maxfun=15000, maxls=20,
                        ftol=1e-9, gtol=1e-6, chunk=8, ctx=None):
        """Device-resident L-BFGS-B for every row of x0s [S, 13] (dh_calibrate_lbfgs).
        ctx: the context (stream and scratch) to run on, default the surface's; a surface may be
        used by several contexts of its device at once.
        -> (list of LbResult, number of loss launches)."""
        x0s = _f64(x0s).reshape(-1, 13)
        S = x0s.shape[0]
        return _lbfgs("dh_calibrate_lbfgs", ctx or self.ctx, self, S,
                      (_ptr(x0s), S, float(S0), float(r), int(N), float(L)),
                      maxiter, maxfun, maxls, chunk, ftol, gtol)

    def loss_terms_rows(self, params, mkt, row, N=128, L=10.0, want_prices=False):
        """dh_surface_loss_rows -> (sse[S], n_bad[S], prices[S,M] or None): the squared relative
        price errors of every param row against row mkt[row[s]] of the market prices mkt [B, M]
        (the surface's option order), and the count of invalid prices."""
        params = _records(params)
        S = params.shape[0]
        mkt = self._market_rows(mkt)
        B = mkt.shape[0]
        row = np.ascontiguousarray(row, dtype=np.int32).reshape(-1)
        if row.size != S:
            raise ValueError("params and row differ in length")
        sse, bad, prices, _, ret = _loss_outputs(S, self.M, want_prices)
        with self.ctx._lock:
            _check(load().dh_surface_loss_rows(self.ctx.handle, self._h, params.ctypes.data,
                                               mkt.ctypes.data, row.ctypes.data, S, B, int(N),
                                               float(L), sse.ctypes.data, bad.ctypes.data,
                                               _addr(prices)))
        return ret

    def loss_rows_dev(self, d_prices: int, d_mkt: int, d_row: int, S: int, d_sse: int, d_bad: int,
                      stream: int = 0):
        """dh_surface_loss_rows_dev: the per-row reduction over [S, M] prices on the device."""
        _check(load().dh_surface_loss_rows_dev(self.ctx.handle, self._h, d_prices, d_mkt, d_row,
                                               int(S), d_sse, d_bad, _addr(stream)))

    def _calibrate_batch(self, symbol, rows_first, mkt, weights, spots, rates, x0s, market_of, N, L,
                         maxiter, maxfun, maxls, chunk, ftol, gtol, ctx):
        """The five calibrate_*_batch* methods: lb_batch_args, and with rows_first iv_rows (mkt
        holds vols and the weight rows follow it in the export's arguments), then _lbfgs."""
        mkt, spots, rates, x0s, mof = lb_batch_args(self.M, mkt, spots, rates, x0s, market_of)
        rows = (_ptr(mkt),)
        if rows_first:
            mkt, w = iv_rows(self.M, mkt, weights)
            rows = (_ptr(mkt), _ptr(w))
        B, S = mkt.shape[0], x0s.shape[0]
        return _lbfgs(symbol, ctx or self.ctx, self, S,
                      (*rows, _ptr(spots), _ptr(rates), B, _ptr(x0s), _ptr(mof, _i32p), S, int(N),
                       float(L)), maxiter, maxfun, maxls, chunk, ftol, gtol)

    def calibrate_lbfgs_batch(self, mkt, spots, rates, x0s, market_of, N=128, L=10.0, *,
                              maxiter=300, maxfun=15000, maxls=20, ftol=1e-9, gtol=1e-6, chunk=8,
                              ctx=None):
        """Device-resident L-BFGS-B over many markets on this surface's option grid
        (dh_calibrate_lbfgs_batch): row i of x0s [S, 13] fits market market_of[i] -- market
        prices mkt[b] of mkt [B, M], spot spots[b], rate rates[b].
        -> (list of LbResult, number of iterations enqueued)."""
        return self._calibrate_batch(
            "dh_calibrate_lbfgs_batch", False, mkt, None, spots, rates, x0s,
            market_of, N, L, maxiter, maxfun, maxls, chunk, ftol, gtol, ctx)

    def loss_terms_iv_rows(self, params, mkt_iv, row, N=128, L=10.0, weights=None,
                           want_prices=False, want_iv=False):
        """dh_surface_loss_iv_rows -> (sse[S], n_bad[S][, prices[S,M]][, iv[S,M]]): the weighted
        squared vol errors of every param row (inverted under its own spot, rate and q) against
        row mkt_iv[row[s]] of the market vols mkt_iv [B, M] under weights [B, M] (None: all 1),
        and the count of weighted options without a vol; iv holds the vols as used."""
        params = _records(params)
        S = params.shape[0]
        mkt_iv = self._market_rows(mkt_iv)
        B = mkt_iv.shape[0]
        w = None
        if weights is not None:
            w = _f64(weights)
            if w.shape != mkt_iv.shape:
                raise ValueError(f"weights must be {mkt_iv.shape}, got {w.shape}")
        row = np.ascontiguousarray(row, dtype=np.int32).reshape(-1)
        if row.size != S:
            raise ValueError("params and row differ in length")
        sse, bad, prices, iv, ret = _loss_outputs(S, self.M, want_prices, bool(want_iv))
        with self.ctx._lock:
            _check(load().dh_surface_loss_iv_rows(
                self.ctx.handle, self._h, params.ctypes.data, mkt_iv.ctypes.data, _addr(w),
                row.ctypes.data, S, B, int(N), float(L), sse.ctypes.data, bad.ctypes.data,
                _addr(prices), _addr(iv)))
        return ret

    def iv_sse_rows_dev(self, d_params: int, d_prices: int, d_mkt_iv: int, d_wgt: int, d_row: int,
                        S: int, d_sse: int, d_bad: int, d_iv: int = 0, stream: int = 0):
        """dh_surface_iv_sse_rows_dev: the per-row vol-space reduction over [S, M] prices on the
        device."""
        _check(load().dh_surface_iv_sse_rows_dev(self.ctx.handle, self._h, d_params, d_prices,
                                                 d_mkt_iv, d_wgt, d_row, int(S), d_sse, d_bad,
                                                 _addr(d_iv), _addr(stream)))

    def calibrate_lbfgs_batch_iv(self, mkt_iv, weights, spots, rates, x0s, market_of, N=128,
                                 L=10.0, *, maxiter=300, maxfun=15000, maxls=20, ftol=1e-9,
                                 gtol=1e-6, chunk=8, ctx=None):
        """calibrate_lbfgs_batch in implied-vol space (dh_calibrate_lbfgs_batch_iv): row i of x0s
        [S, 13] fits the vols mkt_iv[b] of market b = market_of[i] under weights[b] (weights
        [B, M], [M] or None for all 1), spot spots[b], rate rates[b].
        -> (list of LbResult, number of iterations enqueued)."""
        return self._calibrate_batch(
            "dh_calibrate_lbfgs_batch_iv", True, mkt_iv, weights, spots, rates, x0s,
            market_of, N, L, maxiter, maxfun, maxls, chunk, ftol, gtol, ctx)

    def fg(self, X0, S0, r, N=128, L=10.0, model=None):
        """dh_surface_fg: (f [S], g [S, 13], low [S]) of one FD request per row of X0 [S, 13].
        model: [2, S, 13] model params of x0 and x0 + h (dhcos.calibrator.fd_models), or None
        for libm's exp / tanh in the library."""
        X0 = _f64(X0).reshape(-1, 13)
        S = X0.shape[0]
        model = _fd_model(model, S)
        f, g, low = np.empty(S), np.empty((S, 13)), np.empty(S)
        with self.ctx._lock:
            _check(load().dh_surface_fg(self.ctx.handle, self._h, X0.ctypes.data,
                                        None if model is None else model.ctypes.data, S,
                                        float(S0), float(r), int(N), float(L), f.ctypes.data,
                                        g.ctypes.data, low.ctypes.data))
        return f, g, low

    def fg_begin(self, X0, S0, r, N=128, L=10.0, model=None, slot=0):
        """dh_surface_fg_begin: enqueue fg(X0) into a slot (0 .. FG_SLOTS - 1) and return at
        once; the slot keeps the request until fg_end(slot)."""
        X0 = _f64(X0).reshape(-1, 13)
        S = X0.shape[0]
        model = _fd_model(model, S)
        with self.ctx._lock:
            _check(load().dh_surface_fg_begin(self.ctx.handle, self._h, X0.ctypes.data,
                                              None if model is None else model.ctypes.data, S,
                                              float(S0), float(r), int(N), float(L), int(slot)))
            self.ctx._fg_s[int(slot)] = S

    def fg_end(self, slot=0):
        """dh_surface_fg_end: wait for slot's request -> (f [S], g [S, 13], low [S]).  The slot
        must hold a request this surface enqueued (the library checks the surface and S)."""
        with self.ctx._lock:
            S = self.ctx._fg_s[int(slot)] if 0 <= int(slot) < FG_SLOTS else None
            S = 0 if S is None else S          # an idle slot: the library reports the error
            f, g, low = np.empty(S), np.empty((S, 13)), np.empty(S)
            _check(load().dh_surface_fg_end(self.ctx.handle, self._h, int(slot), S, f.ctypes.data,
                                            g.ctypes.data, low.ctypes.data))
            self.ctx._fg_s[int(slot)] = None
        return f, g, low

    def implied_vol(self, params, N=128, L=10.0, want_prices=False):
        """dh_surface_implied_vol: the Black-Scholes vols [P, M] of the model prices of every
        param row (S0, r, q from the row), inverted on the device; with want_prices also the
        prices [P, M] (dh_surface_price's bits) -> iv or (iv, prices)."""
        params = _records(params)
        P = params.shape[0]
        iv = np.empty((P, self.M))
        prices = np.empty((P, self.M)) if want_prices else None
        with self.ctx._lock:
            _check(load().dh_surface_implied_vol(self.ctx.handle, self._h, params.ctypes.data, P,
                                                 int(N), float(L), iv.ctypes.data,
                                                 _addr(prices)))
        return (iv, prices) if want_prices else iv

    def set_iv_market(self, mkt_iv, weight=None):
        """dh_surface_set_iv_market: the market vols [M] (and weights [M], default all 1) of the
        vol-space objective, in the surface's option order; a second call replaces the first."""
        iv = _f64(mkt_iv).reshape(-1)
        w = None if weight is None else _f64(weight).reshape(-1)
        if iv.size != self.M or (w is not None and w.size != self.M):
            raise ValueError(f"mkt_iv and weight must hold {self.M} values")
        with self.ctx._lock:
            _check(load().dh_surface_set_iv_market(self._h, iv.ctypes.data, _addr(w)))

    def loss_terms_iv(self, params, N=128, L=10.0, want_prices=False, want_iv=False):
        """dh_surface_loss_iv -> (sse[S], n_bad[S][, prices[S,M]][, iv[S,M]]): the weighted
        squared vol errors against set_iv_market's vols and the count of weighted options without
        a vol; iv holds the vols as used (0.0 where clamped at the lower bound, NaN where bad)."""
        params = _records(params)
        S = params.shape[0]
        sse, bad, prices, iv, ret = _loss_outputs(S, self.M, want_prices, bool(want_iv))
        with self.ctx._lock:
            _check(load().dh_surface_loss_iv(self.ctx.handle, self._h, params.ctypes.data, S,
                                             int(N), float(L), sse.ctypes.data, bad.ctypes.data,
                                             _addr(prices), _addr(iv)))
        return ret

    def greeks(self, params, N=128, L=10.0):
        """dh_surface_greeks: the planes GREEKS (price, delta, gamma, dual delta, the two v0
        vegas) of every option under every param row -> [6, P, M].  Partial derivatives of the
        COS series at a fixed truncation range and strike (include/dhcos.h)."""
        params = _records(params)
        P = params.shape[0]
        out = np.empty((len(GREEKS), P, self.M))
        with self.ctx._lock:
            _check(load().dh_surface_greeks(self.ctx.handle, self._h, _addr(params, P), P, int(N),
                                            float(L), out.ctypes.data))
        return out

    # device-pointer variants (torch tensors or raw device addresses)
    def greeks_dev(self, d_params: int, P: int, d_out: int, N=128, L=10.0, stream: int = 0):
        """dh_surface_greeks_dev: d_params [P, 16] in, d_out [6, P, M] out, enqueued on stream."""
        _check(load().dh_surface_greeks_dev(self.ctx.handle, self._h, _addr(d_params), int(P),
                                            int(N), float(L), _addr(d_out), _addr(stream)))

    def greeks_full(self, params, N=128, L=10.0):
        """dh_surface_greeks_full: the planes GREEKS_FULL (greeks' six, bit for bit, then
        d price / dT, rho, dual gamma and Dupire's local variance) of every option under every
        param row -> [10, P, M] (include/dhcos.h)."""
        params = _records(params)
        P = params.shape[0]
        out = np.empty((len(GREEKS_FULL), P, self.M))
        with self.ctx._lock:
            _check(load().dh_surface_greeks_full(self.ctx.handle, self._h, _addr(params, P), P,
                                                 int(N), float(L), out.ctypes.data))
        return out

    def greeks_full_dev(self, d_params: int, P: int, d_out: int, N=128, L=10.0, stream: int = 0):
        """dh_surface_greeks_full_dev: d_params [P, 16] in, d_out [10, P, M] out, enqueued on
        stream."""
        _check(load().dh_surface_greeks_full_dev(self.ctx.handle, self._h, _addr(d_params), int(P),
                                                 int(N), float(L), _addr(d_out), _addr(stream)))

    def param_sens(self, params, N=128, L=10.0):
        """dh_surface_param_sens: the planes PARAM_SENS (the price, then its sensitivity to each of
        the thirteen model parameters) of every option under every param row -> [14, P, M].
        Partial derivatives of the COS series at a fixed truncation range (include/dhcos.h)."""
        params = _records(params)
        P = params.shape[0]
        out = np.empty((len(PARAM_SENS), P, self.M))
        with self.ctx._lock:
            _check(load().dh_surface_param_sens(self.ctx.handle, self._h, _addr(params, P), P,
                                                int(N), float(L), out.ctypes.data))
        return out

    def param_sens_dev(self, d_params: int, P: int, d_out: int, N=128, L=10.0, stream: int = 0):
        """dh_surface_param_sens_dev: d_params [P, 16] in, d_out [14, P, M] out, enqueued on
        stream."""
        _check(load().dh_surface_param_sens_dev(self.ctx.handle, self._h, _addr(d_params), int(P),
                                                int(N), float(L), _addr(d_out), _addr(stream)))

    def loss_grad(self, X, S0, r, N=128, L=10.0):
        """dh_surface_loss_grad: the price objective and its analytic gradient in the optimiser's
        unconstrained x, one row of X [S, 13] each -> (f [S], g [S, 13], bad [S]); an invalid set
        (bad > 0) has f = 1e10 and g = 0."""
        X = _f64(X).reshape(-1, 13)
        S = X.shape[0]
        f, g, bad = np.empty(S), np.empty((S, 13)), np.empty(S, dtype=np.int32)
        with self.ctx._lock:
            _check(load().dh_surface_loss_grad(self.ctx.handle, self._h, _addr(X, S), S, float(S0),
                                               float(r), int(N), float(L), f.ctypes.data,
                                               g.ctypes.data, bad.ctypes.data))
        return f, g, bad

    def loss_grad_dev(self, d_x: int, S: int, S0, r, d_f: int, d_g: int, d_bad: int, N=128,
                      L=10.0, stream: int = 0):
        """dh_surface_loss_grad_dev: d_x [S, 13] in, d_f [S], d_g [S, 13], d_bad [S] (int32) out,
        enqueued on stream."""
        _check(load().dh_surface_loss_grad_dev(self.ctx.handle, self._h, _addr(d_x), int(S),
                                               float(S0), float(r), int(N), float(L), _addr(d_f),
                                               _addr(d_g), _addr(d_bad), _addr(stream)))

    def _grad_rows_args(self, X, mkt, spots, rates, row, wgt=None, mkt_name="mkt"):
        """The arguments of the three analytic *_rows methods as contiguous arrays, shapes checked
        -> (X [S, 13], mkt [B, M], spots [B], rates [B], row [S] int32, wgt [B, M] or None, S, B)
        and the outputs every one of them returns: f [S], g [S, 13], bad [S] int32."""
        X = _f64(X).reshape(-1, 13)
        S = X.shape[0]
        mkt = self._market_rows(mkt)
        B = mkt.shape[0]
        w = None
        if wgt is not None:
            w = _f64(wgt)
            if w.shape != mkt.shape:
                raise ValueError(f"wgt must be {mkt.shape}, got {w.shape}")
        spots, rates = _f64(spots).reshape(-1), _f64(rates).reshape(-1)
        if spots.size != B or rates.size != B:
            raise ValueError(f"{mkt_name}, spots and rates differ in length")
        row = np.ascontiguousarray(row, dtype=np.int32).reshape(-1)
        if row.size != S:
            raise ValueError("X and row differ in length")
        return (X, mkt, spots, rates, row, w, S, B,
                np.empty(S), np.empty((S, 13)), np.empty(S, dtype=np.int32))

    def loss_grad_rows(self, X, mkt, spots, rates, row, N=128, L=10.0):
        """dh_surface_loss_grad_rows: loss_grad against a market row per set -- row s of X [S, 13]
        under spots[row[s]] and rates[row[s]] against mkt[row[s]] of mkt [B, M] (the surface's
        option order) -> (f [S], g [S, 13], bad [S]).  The surface needs no market prices."""
        X, mkt, spots, rates, row, _, S, B, f, g, bad = self._grad_rows_args(
            X, mkt, spots, rates, row)
        with self.ctx._lock:
            _check(load().dh_surface_loss_grad_rows(
                self.ctx.handle, self._h, _addr(X, S), _addr(mkt, B), _addr(spots, B),
                _addr(rates, B), _addr(row, S), S, B, int(N), float(L), f.ctypes.data,
                g.ctypes.data, bad.ctypes.data))
        return f, g, bad

    def loss_grad_rows_dev(self, d_x: int, d_mkt: int, d_spot: int, d_rate: int, d_row: int,
                           S: int, d_f: int, d_g: int, d_bad: int, N=128, L=10.0,
                           stream: int = 0):
        """dh_surface_loss_grad_rows_dev: d_x [S, 13], d_mkt [B, M], d_spot [B], d_rate [B], d_row
        [S] (int32) in, d_f [S], d_g [S, 13], d_bad [S] (int32) out, enqueued on stream."""
        _check(load().dh_surface_loss_grad_rows_dev(
            self.ctx.handle, self._h, _addr(d_x), _addr(d_mkt), _addr(d_spot), _addr(d_rate),
            _addr(d_row), int(S), int(N), float(L), _addr(d_f), _addr(d_g), _addr(d_bad),
            _addr(stream)))

    def calibrate_lbfgs_batch_grad(self, mkt, spots, rates, x0s, market_of, N=128, L=10.0, *,
                                   maxiter=300, maxfun=15000, maxls=20, ftol=1e-9, gtol=1e-6,
                                   chunk=8, ctx=None):
        """calibrate_lbfgs_batch with the analytic gradient (dh_calibrate_lbfgs_batch_grad): one
        loss evaluation per request (n_calls == nfev), N <= PARAM_GRAD_MAX_N.
        -> (list of LbResult, number of iterations enqueued)."""
        return self._calibrate_batch(
            "dh_calibrate_lbfgs_batch_grad", False, mkt, None, spots, rates, x0s,
            market_of, N, L, maxiter, maxfun, maxls, chunk, ftol, gtol, ctx)

    def gauss_newton_rows(self, X, mkt, spots, rates, row, N=128, L=10.0):
        """dh_surface_gauss_newton_rows: loss_grad_rows with the Gauss-Newton Hessian of the price
        part of the loss in the optimiser's x -> (f [S], g [S, 13], bad [S], H [S, 13, 13]); f, g
        and bad are loss_grad_rows's bits, H is exactly symmetric, and an invalid set has H = 0."""
        X, mkt, spots, rates, row, _, S, B, f, g, bad = self._grad_rows_args(
            X, mkt, spots, rates, row)
        H = np.empty((S, 13, 13))
        with self.ctx._lock:
            _check(load().dh_surface_gauss_newton_rows(
                self.ctx.handle, self._h, _addr(X, S), _addr(mkt, B), _addr(spots, B),
                _addr(rates, B), _addr(row, S), S, B, int(N), float(L), f.ctypes.data,
                g.ctypes.data, bad.ctypes.data, H.ctypes.data))
        return f, g, bad, H

    def gauss_newton_rows_dev(self, d_x: int, d_mkt: int, d_spot: int, d_rate: int, d_row: int,
                              S: int, d_f: int, d_g: int, d_bad: int, d_H: int, N=128, L=10.0,
                              stream: int = 0):
        """dh_surface_gauss_newton_rows_dev: loss_grad_rows_dev's arguments and d_H [S, 13, 13]
        out, enqueued on stream."""
        _check(load().dh_surface_gauss_newton_rows_dev(
            self.ctx.handle, self._h, _addr(d_x), _addr(d_mkt), _addr(d_spot), _addr(d_rate),
            _addr(d_row), int(S), int(N), float(L), _addr(d_f), _addr(d_g), _addr(d_bad),
            _addr(d_H), _addr(stream)))

    def calibrate_lm_batch(self, mkt, spots, rates, x0s, market_of, N=128, L=10.0, *,
                           maxiter=300, maxfun=15000, ftol=1e-9, gtol=1e-6, chunk=8, ctx=None):
        """calibrate_lbfgs_batch_grad's markets and starts under Levenberg-Marquardt on the
        Gauss-Newton Hessian (dh_calibrate_lm_batch): one request per iteration (n_calls == nfev),
        nit accepted steps, task an LM_* code, N <= PARAM_GRAD_MAX_N.
        -> (list of LbResult, number of iterations enqueued)."""
        return self._calibrate_batch(
            "dh_calibrate_lm_batch", False, mkt, None, spots, rates, x0s,
            market_of, N, L, maxiter, maxfun, 20, chunk, ftol, gtol, ctx)

    def iv_grad_rows_dev(self, d_planes: int, d_params: int, d_pen: int, d_mkt_iv: int, d_wgt: int,
                         d_row: int, d_div: int, S: int, d_f: int, d_g: int, d_bad: int,
                         d_sse: int = 0, d_iv: int = 0, stream: int = 0):
        """dh_surface_iv_grad_rows_dev: the vol objective's loss-and-gradient reduction alone over
        d_planes [14, S, M] (param_sens_dev's), d_params [S, 16], d_pen [S], d_mkt_iv / d_wgt
        [B, M], d_row [S] (int32), d_div [S] in; d_f [S], d_g [S, 13], d_bad [S] (int32) and the
        optional d_sse [S], d_iv [S, M] out, enqueued on stream."""
        _check(load().dh_surface_iv_grad_rows_dev(
            self.ctx.handle, self._h, _addr(d_planes), _addr(d_params), _addr(d_pen),
            _addr(d_mkt_iv), _addr(d_wgt), _addr(d_row), _addr(d_div), int(S), _addr(d_f),
            _addr(d_g), _addr(d_sse), _addr(d_bad), _addr(d_iv), _addr(stream)))

    def loss_iv_grad_rows(self, X, mkt_iv, wgt, spots, rates, row, N=128, L=10.0):
        """dh_surface_loss_iv_grad_rows: the vol objective and its exact gradient (price
        sensitivities over each option's Black-Scholes vega) against a market row per set -- row s
        of X [S, 13] under spots[row[s]] and rates[row[s]] against the vols mkt_iv[row[s]] under
        wgt[row[s]] (mkt_iv [B, M]; wgt [B, M] or None for all 1)
        -> (f [S], g [S, 13], bad [S], iv [S, M] the vols as used)."""
        X, mkt_iv, spots, rates, row, w, S, B, f, g, bad = self._grad_rows_args(
            X, mkt_iv, spots, rates, row, wgt, "mkt_iv")
        iv = np.empty((S, self.M))
        with self.ctx._lock:
            _check(load().dh_surface_loss_iv_grad_rows(
                self.ctx.handle, self._h, _addr(X, S), _addr(mkt_iv, B), _addr(w),
                _addr(spots, B), _addr(rates, B), _addr(row, S), S, B, int(N), float(L),
                f.ctypes.data, g.ctypes.data, bad.ctypes.data, iv.ctypes.data))
        return f, g, bad, iv

    def loss_iv_grad_rows_dev(self, d_x: int, d_mkt_iv: int, d_wgt: int, d_div: int, d_spot: int,
                              d_rate: int, d_row: int, S: int, d_f: int, d_g: int, d_bad: int,
                              d_iv: int = 0, N=128, L=10.0, stream: int = 0):
        """dh_surface_loss_iv_grad_rows_dev: d_x [S, 13], d_mkt_iv / d_wgt [B, M], d_div [S], d_spot
        [B], d_rate [B], d_row [S] (int32) in, d_f [S], d_g [S, 13], d_bad [S] (int32) and the
        optional d_iv [S, M] out, enqueued on stream."""
        _check(load().dh_surface_loss_iv_grad_rows_dev(
            self.ctx.handle, self._h, _addr(d_x), _addr(d_mkt_iv), _addr(d_wgt), _addr(d_div),
            _addr(d_spot), _addr(d_rate), _addr(d_row), int(S), int(N), float(L), _addr(d_f),
            _addr(d_g), _addr(d_bad), _addr(d_iv), _addr(stream)))

    def calibrate_lbfgs_batch_iv_grad(self, mkt_iv, weights, spots, rates, x0s, market_of, N=128,
                                      L=10.0, *, maxiter=300, maxfun=15000, maxls=20, ftol=1e-9,
                                      gtol=1e-6, chunk=8, ctx=None):
        """calibrate_lbfgs_batch_iv with the vol objective's exact gradient
        (dh_calibrate_lbfgs_batch_iv_grad): one loss evaluation per request (n_calls == nfev), N <=
        PARAM_GRAD_MAX_N.  -> (list of LbResult, number of iterations enqueued)."""
        return self._calibrate_batch(
            "dh_calibrate_lbfgs_batch_iv_grad", True, mkt_iv, weights, spots, rates, x0s,
            market_of, N, L, maxiter, maxfun, maxls, chunk, ftol, gtol, ctx)

    def price_dev(self, d_params: int, P: int, d_out: int, N=128, L=10.0, stream: int = 0):
        _check(load().dh_surface_price_dev(self.ctx.handle, self._h, d_params, int(P), int(N),
                                           float(L), d_out, _addr(stream)))

    def loss_dev(self, d_params: int, S: int, d_sse: int, d_bad: int, d_prices: int = 0, N=128,
                 L=10.0, stream: int = 0):
        _check(load().dh_surface_loss_dev(self.ctx.handle, self._h, d_params, int(S), int(N),
                                          float(L), d_sse, d_bad, _addr(d_prices),
                                          _addr(stream)))

    def iv_sse_dev(self, d_params: int, d_prices: int, S: int, d_sse: int, d_bad: int,
                   d_iv: int = 0, stream: int = 0):
        """dh_surface_iv_sse_dev: the vol-space reduction over [S, M] prices on the device."""
        _check(load().dh_surface_iv_sse_dev(self.ctx.handle, self._h, d_params, d_prices, int(S),
                                            d_sse, d_bad, _addr(d_iv), _addr(stream)))

    def loss_iv_dev(self, d_params: int, S: int, d_sse: int, d_bad: int, d_prices: int = 0,
                    d_iv: int = 0, N=128, L=10.0, stream: int = 0):
        """dh_surface_loss_iv_dev: price, then reduce in vol space, on one stream."""
        _check(load().dh_surface_loss_iv_dev(self.ctx.handle, self._h, d_params, int(S), int(N),
                                             float(L), d_sse, d_bad, _addr(d_prices),
                                             _addr(d_iv), _addr(stream)))


class FgChannel:
    """One slot of dh_surface_fg_begin / _end with its arguments prepared once: preallocated
    input (x0, model) and output (f, g, low) buffers whose addresses and the constant scalars are
    ctypes objects built up front, so a request costs two row copies in, one foreign call each
    way and three small copies out (the SciPy driver's per-request host path: the generic
    Surface.fg_begin / fg_end marshal every argument per call, ~10 us each).  The slot protocol
    (Context._fg_s, the context lock) is Surface.fg_begin / fg_end's."""

    def __init__(self, surf: "Surface", slot: int, s_max: int, S0, r, N=128, L=10.0, ctx=None):
        lib = load()
        self.surf, self.slot, self.s_max = surf, int(slot), int(s_max)
        self.ctx = surf.ctx if ctx is None else ctx     # the slot's context (same device)
        if not 0 <= self.slot < FG_SLOTS or self.s_max < 1:
            raise ValueError(f"slot must be 0 .. {FG_SLOTS - 1} and s_max >= 1")
        self._x = np.empty((self.s_max, 13))
        self._m = np.empty(2 * self.s_max * 13)        # [2][S][13] for the request's S
        self._f, self._low = np.empty(self.s_max), np.empty(self.s_max)
        self._g = np.empty((self.s_max, 13))
        self._begin = lib["dh_surface_fg_begin"]        # own function objects: raw arguments
        self._begin.restype, self._begin.argtypes = C.c_int, None
        self._end = lib["dh_surface_fg_end"]
        self._end.restype, self._end.argtypes = C.c_int, None
        ctx = C.c_void_p(self.ctx.handle.value)
        sh = C.c_void_p(surf.handle.value)
        self._S = C.c_int(0)
        self._bargs = (ctx, sh, C.c_void_p(self._x.ctypes.data), C.c_void_p(self._m.ctypes.data),
                       self._S, C.c_double(float(S0)), C.c_double(float(r)), C.c_int(int(N)),
                       C.c_double(float(L)), C.c_int(self.slot))
        self._eargs = (ctx, sh, C.c_int(self.slot), self._S, C.c_void_p(self._f.ctypes.data),
                       C.c_void_p(self._g.ctypes.data), C.c_void_p(self._low.ctypes.data))
        self._lock = self.ctx._lock
        self._fg_s = self.ctx._fg_s
        self._consts = (float(S0), float(r), int(N), float(L))

    def loop_slot(self):
        """The slot's buffers as the native request loop takes them (dhcos._scipy_loop.run):
        x, model, f, g, low, and per request size S the packed exp / tanh columns."""
        ev = [None] + [np.empty(2 * S * 10) for S in range(1, self.s_max + 1)]
        tv = [None] + [np.empty(2 * S * 2) for S in range(1, self.s_max + 1)]
        return (self._x, self._m, self._f, self._g, self._low, ev, tv)

    def loop_device(self):
        """The C-ABI entry points and handles the native request loop calls
        (dh_surface_fg_begin / _end / _cancel on this channel's surface and constants)."""
        lib = load()

        def addr(name):
            return C.cast(lib[name], C.c_void_p).value
        S0, r, N, L = self._consts
        return (addr("dh_surface_fg_begin"), addr("dh_surface_fg_end"),
                addr("dh_surface_fg_cancel"), self.ctx.handle.value, self.surf.handle.value,
                S0, r, N, L)

    def model_out(self, S: int) -> np.ndarray:
        """The [2, S, 13] model buffer of a request of S starts (fd_models(..., out=))."""
        return self._m[:2 * S * 13].reshape(2, S, 13)

    def x_rows(self, S: int) -> np.ndarray:
        """The [S, 13] point buffer of a request of S starts: rows written here need no copy
        in begin()."""
        return self._x[:S]

    def begin(self, X0: np.ndarray, model: np.ndarray = None):
        """Enqueue the request of X0 [S, 13] (x_rows(S) itself, or rows to copy there; model:
        [2, S, 13], default: already written into model_out(S))."""
        S = X0.shape[0]
        if S > self.s_max or S < 1:
            raise ValueError(f"request of {S} starts on a channel of {self.s_max}")
        if not (X0.base is self._x and X0.ctypes.data == self._x.ctypes.data):
            self._x[:S] = X0                            # (x_rows(S) itself needs no copy)
        if model is not None:
            self.model_out(S)[...] = model
        with self._lock:
            self._S.value = S
            _check(self._begin(*self._bargs))
            self._fg_s[self.slot] = S

    def end(self):
        """-> (f [S], g [S, 13], low [S]) of the slot's request (copies: the buffers are reused)."""
        with self._lock:
            S = self._fg_s[self.slot]
            self._S.value = 0 if S is None else S       # an idle slot: the library reports it
            _check(self._end(*self._eargs))             # (on failure the request stays in flight)
            self._fg_s[self.slot] = None
        return self._f[:S].copy(), self._g[:S].copy(), self._low[:S].copy()


def comm_id() -> bytes:
    """dh_comm_id: a fresh RCCL unique id (rank 0), to be shipped to every rank."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().dh_comm_id(C.cast(buf, _vp)))
    return buf.raw


def best_start(records, col_start, col_fun) -> int:
    """dh_best_start: the reference's strict-< best start (lbfgs_calibrator.py:271-275) over
    per-start rows (negative start index = padding); -1 if none."""
    rec = _f64(records)
    rows, width = (rec.shape[0], rec.shape[1]) if rec.ndim == 2 else (0, 1)
    best = C.c_int32(-2)
    _check(load().dh_best_start(_addr(rec, rows), rows, width, int(col_start), int(col_fun),
                                C.byref(best)))
    return best.value


class Comm(_Handle):
    """dh_comm: an RCCL communicator over the ranks' contexts (one per rank, its device and
    stream), for multi-start sharding without torch.distributed.  Collective construction: every
    rank passes rank 0's ``comm_id()`` bytes."""

    def __init__(self, ctx: "Context", uid: bytes, world: int, rank: int):
        if len(uid) != COMM_ID_BYTES:
            raise ValueError(f"comm id must be {COMM_ID_BYTES} bytes")
        self.ctx, self.world, self.rank = ctx, int(world), int(rank)
        self._uid = C.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        h = _vp()
        _check(load().dh_comm_create(ctx.handle, C.cast(self._uid, _vp), self.world, self.rank,
                                     C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            h, self._h = self._h, None
            _check(load().dh_comm_destroy(h))

    def broadcast(self, buf, root: int = 0) -> np.ndarray:
        """root's float64 values on every rank (in place on a contiguous array; returned)."""
        out = _f64(buf)
        _check(load().dh_comm_broadcast(self._h, _addr(out, out.size), out.size, int(root)))
        return out

    def allgather(self, block) -> np.ndarray:
        """block (float64, same size on every rank) -> [world, *block.shape] in rank order."""
        blk = _f64(block)
        out = np.empty((self.world,) + blk.shape)
        _check(load().dh_comm_allgather(self._h, _addr(blk, blk.size), blk.size,
                                        _addr(out, out.size)))
        return out

    def allgather_best(self, records, col_start: int, col_fun: int):
        """records [rows, width] of this rank (same rows on every rank) -> ([world * rows, width]
        in rank order, the strict-< best start or -1)."""
        rec = _f64(records)
        rows, width = rec.shape
        out = np.empty((self.world * rows, width))
        best = C.c_int32(-2)
        _check(load().dh_allgather_best(self._h, _addr(rec, rec.size), rows, width,
                                        int(col_start), int(col_fun), out.ctypes.data,
                                        C.byref(best)))
        return out, best.value


def gen_draw(n_samples, lo, hi, n_opt, alpha, spot0, ret_mu, ret_sigma, noise_sigma):
    """dh_gen_draw on NumPy's global legacy RandomState: draws the generator's samples natively
    and advances np.random's state exactly as the reference's per-sample calls would.
    -> (params [n, 13], spots [n], noise [n, n_opt])."""
    rng = _RngState()
    n = int(n_samples)
    params, spots, noise = np.empty((n, 13)), np.empty(n), np.empty((n, int(n_opt)))
    _check(load().dh_gen_draw(*rng.args(), n, _ptr(_f64(lo)), _ptr(_f64(hi)), int(n_opt),
                              float(alpha), float(spot0), float(ret_mu), float(ret_sigma),
                              float(noise_sigma), _ptr(params), _ptr(spots), _ptr(noise)))
    rng.restore()
    return params, spots, noise


class GenDraw:
    """dh_gen_draw_progress on a worker thread (the ctypes call releases the GIL): the same
    draws as gen_draw, whose finished rows the caller may consume while the rest are drawn.
    ``ready(e)`` blocks until rows < e of params / spots / noise are complete; ``finish()``
    joins the draw, leaves np.random's state where gen_draw leaves it and returns
    (params, spots, noise).  np.random must not be used between the two."""

    def __init__(self, n_samples, lo, hi, n_opt, alpha, spot0, ret_mu, ret_sigma, noise_sigma):
        self._rng = _RngState()
        n = self.n = int(n_samples)
        self.params, self.spots = np.empty((n, 13)), np.empty(n)
        self.noise = np.empty((n, int(n_opt)))
        self._lo, self._hi = _f64(lo), _f64(hi)
        self._args = (int(n_opt), float(alpha), float(spot0), float(ret_mu), float(ret_sigma),
                      float(noise_sigma))
        self._done = C.c_int64(0)
        self._rc = None
        self._finished = False
        lib = load()
        self._thread = threading.Thread(target=self._run, args=(lib,), daemon=True)
        self._thread.start()

    def _run(self, lib):
        self._rc = lib.dh_gen_draw_progress(
            *self._rng.args(), self.n, _ptr(self._lo), _ptr(self._hi), *self._args,
            _ptr(self.params), _ptr(self.spots), _ptr(self.noise), C.byref(self._done))

    def ready(self, e):
        e = min(int(e), self.n)
        while self._done.value < e and self._thread.is_alive():
            self._thread.join(5e-5)
        if self._done.value < e:                      # the draw ended early: its error
            self.finish()
            raise NativeError("dh_gen_draw_progress stopped before the requested rows")

    def finish(self):
        if not self._finished:
            self._thread.join()
            self._finished = True
            _check(self._rc if self._rc is not None else -1)   # None: the thread raised
            self._rng.restore()
        return self.params, self.spots, self.noise


def gen_locate(state, n_samples, n_opt, starts):
    """dh_gen_locate: from an np.random legacy state (``[627]`` float64: key, pos, has_gauss,
    cached gauss) the generator's state at each sample index of ``starts`` of an
    ``n_samples``-sample draw, without drawing the samples -> (loc [len(starts), 627], the state
    the whole draw leaves [627])."""
    st = np.asarray(state, dtype=np.float64).reshape(GEN_LOC_WORDS)
    rng = _RngState(("MT19937", st[:624].astype(np.uint32), st[624], st[625], st[626]))
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    loc = np.empty((starts.size, GEN_LOC_WORDS))
    _check(load().dh_gen_locate(*rng.args(), int(n_samples), int(n_opt),
                                _addr(starts, starts.size), starts.size, _ptr(loc)))
    key, *cells = rng.values()
    return loc, np.concatenate([key.astype(np.float64), cells])


def gen_draw_located(loc, starts, i_end, lo, hi, n_opt, ret_mu, ret_sigma, noise_sigma):
    """dh_gen_draw_located: samples [starts[0], i_end) drawn from located states (chunk j from
    loc[j]) -> (raw params [n, 13], spot returns [n] (row of sample 0 unset), noise [n, n_opt])."""
    loc = _f64(loc).reshape(-1, GEN_LOC_WORDS)
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    if loc.shape[0] != starts.size:
        raise NativeError("gen_draw_located: one state per chunk start")
    n = int(i_end) - int(starts[0]) if starts.size else 0
    if n < 0:
        raise NativeError("gen_draw_located: i_end before the first start")
    params, rets, noise = np.empty((n, 13)), np.empty(n), np.empty((n, int(n_opt)))
    if starts.size:
        _check(load().dh_gen_draw_located(_ptr(loc), starts.ctypes.data, starts.size, int(i_end),
                                          _ptr(_f64(lo)), _ptr(_f64(hi)), int(n_opt),
                                          float(ret_mu), float(ret_sigma), float(noise_sigma),
                                          _ptr(params), _ptr(rets), _ptr(noise)))
    return params, rets, noise


def gen_sweep(params, spots, i0, alpha, spot0, carry):
    """dh_gen_sweep in place on a block of samples [i0, i0 + n): AR(1) blend of the raw params
    and the spot walk from the returns; carry [14] (the previous sample's params and spot) in,
    this block's last row out (returned)."""
    n = params.shape[0]
    for a, shp in ((params, (n, 13)), (spots, (n,))):
        _out_array(a, shp, NativeError,
                   "gen_sweep: params [n, 13] and spots [n] must be C-contiguous float64",
                   writeable=False)
    carry = np.array(carry, dtype=np.float64).reshape(14)
    _check(load().dh_gen_sweep(_ptr(params), _ptr(spots), int(i0), n, float(alpha), float(spot0),
                               _ptr(carry)))
    return carry


def gen_drawn_samples() -> int:
    """dh_gen_drawn_samples: samples this process's draw calls have drawn so far."""
    c = C.c_int64(0)
    _check(load().dh_gen_drawn_samples(C.byref(c)))
    return c.value


def gen_assemble(model, noise, spots, k_rel, out=None):
    """dh_gen_assemble: the generator's market prices, per-sample losses (np.mean's bits) and
    absolute strikes from [n, m] model prices and noise.  -> (market, loss, strikes), written into
    ``out`` (three C-contiguous float64 arrays of those shapes, e.g. row slices) if given."""
    model, noise = _f64(model), _f64(noise)
    spots, k_rel = _f64(spots), _f64(k_rel)
    n, m = model.shape
    if noise.shape != (n, m) or spots.shape != (n,) or k_rel.shape != (m,):
        raise NativeError("gen_assemble: shape mismatch")
    market, loss, strikes = (None, None, None) if out is None else out
    market, loss, strikes = (
        _out_array(a, shp, NativeError, "gen_assemble: out arrays must be writable C-contiguous "
                   "float64 of the input shapes")
        for a, shp in ((market, (n, m)), (loss, (n,)), (strikes, (n, m))))
    _check(load().dh_gen_assemble(_ptr(model), _ptr(noise), _ptr(spots), _ptr(k_rel), n, m,
                                  _ptr(market), _ptr(loss), _ptr(strikes)))
    return market, loss, strikes


def gen_dates(first_day, n):
    """dh_gen_dates: n weekday dates from day first_day (a Monday; days since 1970-01-01) as a
    '<U10' array of 'YYYY-MM-DD', or None past year 9999 (the caller formats those)."""
    out = np.empty(int(n), dtype="U10")
    rc = load().dh_gen_dates(int(first_day), int(n), _addr(out, n))
    if rc != 0:
        return None
    return out


_tls = threading.local()
# the device resolved under each initialised process group (resolve_device): fixed at the group's
# first resolution, so that the library's own CUDA tensors (collectives on the LOCAL_RANK GPU)
# cannot move a later resolution to torch's default device 0
_group_device = {}


def resolve_device(device: int | None = None) -> int:
    """The GPU a call without an explicit ``device=`` runs on, in this order: $DHCOS_DEVICE;
    under torch.distributed (one process per GPU, e.g. torchrun) the device the rank bound --
    the process group's ``device_id``, else torch's current device once the rank has set up its
    CUDA state (``torch.cuda.set_device``, any CUDA tensor: whatever rank-to-GPU map the caller
    used, device 0 included, so this library's GPU is its tensors' and collectives' GPU) -- then
    $LOCAL_RANK modulo the visible devices (a gloo job that never touched CUDA: each rank its own
    GPU, not all on GPU 0); otherwise 0.  ``distributed._comm_device`` puts the collectives'
    tensors on the same GPU."""
    if device is not None:
        return int(device)
    env = os.environ.get("DHCOS_DEVICE")
    if env not in (None, ""):
        return int(env)
    torch = sys.modules.get("torch")
    dist = getattr(torch, "distributed", None) if torch is not None else None
    if dist is not None and dist.is_available() and dist.is_initialized():
        try:
            group = dist.distributed_c10d._get_default_group()
        except Exception:              # noqa: BLE001 -- an older torch without the accessor
            group = None
        key = id(group)
        hit = _group_device.get(key)
        if hit is not None and hit[0] is group:
            return hit[1]
        dev = None
        if torch.cuda.is_available():
            bound = getattr(group, "bound_device_id", None)
            if bound is not None and bound.type == "cuda" and bound.index is not None:
                dev = int(bound.index)
            elif torch.cuda.is_initialized():
                # the rank set up its CUDA state before its first call here: its current device
                dev = int(torch.cuda.current_device())
        if dev is None:
            local = os.environ.get("LOCAL_RANK")
            if local not in (None, ""):
                n = device_count()
                dev = int(local) % n if n > 0 else int(local)
            else:
                dev = 0
        if group is not None:
            _group_device[key] = (group, dev)
        return dev
    return 0


class pinned:
    """Context manager: page-lock the memory of C-contiguous NumPy arrays for its duration
    (dh_host_register), so the library's copies of them run as DMA without staging.  An array
    that cannot be registered (e.g. already registered) is left pageable: the copies then stage
    as usual, with the same results."""

    def __init__(self, *arrays):
        self._arrays = [a for a in arrays if a is not None and a.nbytes and a.flags.c_contiguous]
        self._done = []

    def __enter__(self):
        lib = load()
        for a in self._arrays:
            if lib.dh_host_register(a.ctypes.data, a.nbytes) == 0:
                self._done.append(a)
        return self

    def __exit__(self, *exc):
        lib = load()
        while self._done:
            a = self._done.pop()
            lib.dh_host_unregister(a.ctypes.data)
        return False


class _PinnedBlock:
    """A dh_host_alloc block exposed through the array interface; the block returns to the
    library's page-locked cache when the last array over it is freed."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        ptr = _vp()
        _check(load().dh_host_alloc(self.nbytes, C.byref(ptr)))
        self.ptr = ptr.value
        self.__array_interface__ = {"shape": tuple(int(d) for d in shape), "typestr": dtype.str,
                                    "data": (self.ptr, False), "version": 3}

    def __del__(self):
        lib = _lib
        if lib is not None and getattr(self, "ptr", None):
            lib.dh_host_free(self.ptr)
            self.ptr = None


def pinned_empty(shape, dtype=np.float64) -> np.ndarray:
    """An uninitialised C-contiguous array in page-locked host memory from the library's cache
    (dh_host_alloc): device copies into it run as DMA, and a freed array's block serves the next
    request of its size without a new allocation or page faults."""
    dtype = np.dtype(dtype)
    if isinstance(shape, (int, np.integer)):
        shape = (int(shape),)
    if int(np.prod(shape, dtype=np.int64)) == 0:
        return np.empty(shape, dtype=dtype)
    return np.asarray(_PinnedBlock(shape, dtype))


def host_cache_trim():
    """Release the page-locked blocks the cache holds (dh_host_cache_trim)."""
    _check(load().dh_host_cache_trim())


def gen_log(x, ctx=None) -> np.ndarray:
    """dh_gen_log: the device restatement of glibc's log (the legacy gauss's) over x."""
    x = _f64(x).ravel()
    out = np.empty_like(x)
    ctx = ctx or default_context()
    _check(load().dh_gen_log(ctx.handle, _addr(x, x.size), x.size, _addr(out, x.size)))
    return out


# dh_math_probe's function ids (include/dhcos.h)
MATH_PROBE_FNS = {name: i for i, name in enumerate((
    "dsincos", "dsincos_t", "dexp", "dexp_nonpos", "dexp_t", "dexp_t_nonpos", "dlog", "dlog_t",
    "datan2", "datan2_t", "drcp", "dsqrt_rsqrt", "dsqrt_rsqrt_pos", "csqrt_p", "cdiv",
    "cdiv_rcp"))}
_PROBE_TWO_ARGS = ("datan2", "datan2_t", "csqrt_p", "cdiv", "cdiv_rcp")
_PROBE_TWO_OUT = ("dsincos", "dsincos_t", "dsqrt_rsqrt", "dsqrt_rsqrt_pos", "csqrt_p", "cdiv",
                  "cdiv_rcp")


def math_probe(fn_name, x, y=None, ctx=None):
    """dh_math_probe: one fp64 elementary function of csrc/dh_device.h over arrays (test support).
    x: the argument, atan2's first argument or the real part; y: atan2's second argument or the
    imaginary part.  cdiv / cdiv_rcp take x = [a.re | b.re], y = [a.im | b.im] (two halves of n
    each) and return n quotients.  -> out0, or (out0, out1) for sincos (sin, cos), sqrt_rsqrt
    (sqrt, rsqrt) and the complex helpers (re, im)."""
    if not isinstance(fn_name, str):
        raise TypeError("math_probe: the function is given by name (MATH_PROBE_FNS)")
    fn = MATH_PROBE_FNS.get(fn_name, -1)          # an unknown name: DH_E_ARG from the library
    x = _f64(x).ravel()
    two = fn_name in _PROBE_TWO_ARGS
    if two:
        if y is None:
            raise ValueError(f"math_probe: {fn_name} takes two arrays")
        y = _f64(y).ravel()
        if y.size != x.size:
            raise ValueError("math_probe: x and y differ in size")
    n = x.size
    if fn_name in ("cdiv", "cdiv_rcp"):
        if n % 2:
            raise ValueError("math_probe: cdiv takes two operands (x and y of 2 n entries)")
        n //= 2
    out0, out1 = np.empty(n), np.empty(n)
    ctx = ctx or default_context()
    _check(load().dh_math_probe(ctx.handle, fn, _addr(x, n), _addr(y, two and n), n,
                                _addr(out0, n), _addr(out1, n)))
    return (out0, out1) if fn_name in _PROBE_TWO_OUT else out0


def gen_device(surf, n_samples, lo, hi, alpha, spot0, ret_mu, ret_sigma, noise_sigma, r, k_rel,
               N=128, L=10.0, first_day=None, stats=None):
    """dh_gen_device on NumPy's global legacy RandomState: the generator's samples drawn, blended,
    priced on ``surf`` (its grid, strikes in percent of each sample's spot) and assembled on the
    device; np.random's state advanced exactly as the reference's per-sample calls would.  The
    outputs are page-locked arrays (pinned_empty).  -> dict(params, spots, market, model, loss,
    strikes, dates ('<U10', or None when first_day is None))."""
    rng = _RngState()
    n, m = int(n_samples), int(surf.M)
    k_rel = _f64(k_rel).reshape(-1)
    if k_rel.size != m:
        raise NativeError("gen_device: one strike percentage per option of the grid")
    out = {"params": pinned_empty((n, 13)), "spots": pinned_empty(n),
           "market": pinned_empty((n, m)), "model": pinned_empty((n, m)),
           "loss": pinned_empty(n), "strikes": pinned_empty((n, m)),
           "dates": pinned_empty(n, "U10") if first_day is not None else None}
    st = np.zeros(8) if stats is None else stats
    addr = {k: _addr(v, v is None or v.size) for k, v in out.items()}
    _check(load().dh_gen_device(
        surf.ctx.handle, surf.handle, *rng.args(), n, _ptr(_f64(lo)), _ptr(_f64(hi)),
        float(alpha), float(spot0), float(ret_mu), float(ret_sigma), float(noise_sigma), float(r),
        int(N), float(L), _ptr(k_rel), int(first_day or 0), addr["params"], addr["spots"],
        addr["market"], addr["model"], addr["loss"], addr["strikes"], addr["dates"], _ptr(st)))
    rng.restore()
    return out


def default_context(device: int | None = None) -> Context:
    """Per-thread cached context on ``device`` (default: resolve_device())."""
    device = resolve_device(device)
    cache = getattr(_tls, "ctxs", None)
    if cache is None:
        cache = _tls.ctxs = {}
    ctx = cache.get(device)
    if ctx is None:
        ctx = cache[device] = Context(device)
    return ctx


# every public top-level name, in SIGNATURES' groups: the library, context and surfaces, L-BFGS-B,
# generator, communicator, Monte Carlo, least-squares Monte Carlo, the warm-start network
__all__ = [
    "LIB_PATH", "SIGNATURES", "NativeError", "load", "runtime_shared_with_torch", "device_count",
    "resolve_device", "default_context", "PARAM_STRIDE", "MAX_N", "MAX_N_PER_TERM",
    "STRIKE_ABSOLUTE", "STRIKE_PCT_SPOT", "PATH_AUTO", "PATH_SPLIT", "PATH_FUSED", "PATH_GEN",
    "FG_SLOTS", "STAMPS_PER_BLOCK", "GREEKS", "GREEKS_FULL", "PARAM_SENS", "PARAM_GRAD_MAX_N",
    "LM_MESSAGES", "Context", "Surface", "FgChannel", "pinned", "pinned_empty", "host_cache_trim",
    "LbOptions", "LbResult", "lb_batch_args", "iv_rows",
    "gen_draw", "GenDraw", "GEN_LOC_WORDS", "gen_locate", "gen_draw_located", "gen_sweep",
    "gen_drawn_samples", "gen_dates", "gen_assemble", "gen_device", "gen_log",
    "MATH_PROBE_FNS", "math_probe",
    "COMM_ID_BYTES", "Comm", "comm_id", "best_start",
    "McOption", "MC_KINDS", "MC_MAX_OPTIONS", "MC_POISSON_CAP",
    "MC_VR_ANTITHETIC", "MC_VR_CONTROL", "MC_VR_COS_N", "MC_VR_COS_L", "MC_GREEKS",
    "LsmOption", "LSM_MAX_OPTIONS", "LSM_BASIS", "LSM_MIN_ITM", "LSM_SLOTS", "LSM_MAX_GIB",
    "FFN", "FFN_OUT", "FFN_TM", "FFN_MAX_HIDDEN", "FFN_MAX_WIDTH", "FFN_MAX_IN",
]
