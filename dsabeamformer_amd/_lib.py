"""ctypes loader for libdsabf.so.  Fails loudly: there is no CPU or PyTorch fallback for the hot path."""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# DSABF_LIB_PATH: a measurement build made by tools/build_variant.py (A/B experiments only; never set by tests or bench.py)
LIB_PATH = os.environ.get("DSABF_LIB_PATH") or os.path.join(PKG, "libdsabf.so")

BF_OK = 0
BF_NOT_READY = 1
BF_ERR_INVALID, BF_ERR_DEVICE, BF_ERR_NO_DEVICE, BF_ERR_STATE = -1, -2, -3, -4
BF_DETECT_CANONICAL, BF_DETECT_FAST, BF_DETECT_CONTRACTED = 0, 1, 2
BF_CAL_PHASE, BF_CAL_FULL = 0, 1
BF_NULL_MAX = 4
BF_NULL_SCALED, BF_NULL_CLIP = 0, 1
BF_SK_DEAD, BF_SK_LOW, BF_SK_HIGH = 1, 2, 4   # cell codes of bf_sk_select (include/dsabf.h)
BF_STOKES_MAX_BEAMS = 16


class BfConfig(C.Structure):
    """Mirror of ``bf_config`` (include/dsabf.h)."""

    _fields_ = [(n, C.c_int) for n in ("n_beams", "n_ant", "n_freq", "n_pol", "n_avg", "n_out_per_gemm",
                                       "n_gemms_per_block", "n_blocks_on_gpu", "n_streams", "verbose", "detect_mode")]


class BfhEventOps(C.Structure):
    """Mirror of ``bfh_event_ops`` (include/dsabf_host.h): an event backend as a table of C callbacks."""

    CREATE = C.CFUNCTYPE(C.c_void_p, C.c_void_p)
    DESTROY = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
    RECORD = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
    QUERY = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
    _fields_ = [("user", C.c_void_p), ("create", CREATE), ("destroy", DESTROY), ("record_transfer", RECORD),
                ("record_analysis", RECORD), ("query", QUERY)]


class BfGatherMsg(C.Structure):
    """Mirror of ``bf_gather_msg`` (include/dsabf.h)."""

    _fields_ = [("kind", C.c_int), ("peer", C.c_int), ("local_offset", C.c_size_t), ("full_offset", C.c_size_t),
                ("count", C.c_size_t)]


class BfSpsPeak(C.Structure):
    """Mirror of ``bf_sps_peak`` (include/dsabf.h)."""

    _fields_ = [("value", C.c_float), ("t_end", C.c_int32)]


class BfSpsStat(C.Structure):
    """Mirror of ``bf_sps_stat`` (include/dsabf.h)."""

    _fields_ = [("sum", C.c_double), ("sumsq", C.c_double)]


class BfPsrModel(C.Structure):
    """Mirror of ``bf_psr_model`` (include/dsabf.h)."""
    _fields_ = [("phase0", C.c_uint64), ("dphase", C.c_uint64), ("ddphase", C.c_int64), ("epoch_row", C.c_int64)]


class BfFfaPeak(C.Structure):
    """Mirror of ``bf_ffa_peak`` (include/dsabf.h)."""
    _fields_ = [("value", C.c_float), ("shift", C.c_uint16), ("bin", C.c_uint16)]


class BfFfaStat(C.Structure):
    """Mirror of ``bf_ffa_stat`` (include/dsabf.h)."""
    _fields_ = [("sum", C.c_double), ("sumsq", C.c_double)]


class BfFfaCandidate(C.Structure):
    """Mirror of ``bf_ffa_candidate`` (include/dsabf.h)."""
    _fields_ = [("first_row", C.c_uint64), ("n_rows", C.c_uint64), ("period_rows", C.c_double), ("dm", C.c_int32), ("beam", C.c_int32),
                ("octave", C.c_int32), ("p", C.c_int32), ("shift", C.c_int32), ("bin", C.c_int32), ("width", C.c_int32), ("snr", C.c_double),
                ("value", C.c_float)]


class BfFfaGroup(C.Structure):
    """Mirror of ``bf_ffa_group`` (include/dsabf.h)."""
    _fields_ = [("head", BfFfaCandidate), ("n_members", C.c_int32), ("n_beams", C.c_int32), ("dm_lo", C.c_int32), ("dm_hi", C.c_int32),
                ("n_harmonic", C.c_int32), ("reserved", C.c_int32)]


class BfCondOptions(C.Structure):
    """Mirror of ``bf_cond_options`` (include/dsabf.h)."""
    _fields_ = [("baseline_pushes", C.c_int), ("zero_dm", C.c_int), ("auto_threshold", C.c_double)]


class BfSpsCandidate(C.Structure):
    """Mirror of ``bf_sps_candidate`` (include/dsabf.h)."""

    _fields_ = [("t_start", C.c_uint64), ("dm", C.c_int32), ("beam", C.c_int32), ("width", C.c_int32), ("peak", C.c_float),
                ("snr", C.c_double)]


class BfEvtOptions(C.Structure):
    """Mirror of ``bf_evt_options`` (include/dsabf.h)."""

    _fields_ = [("t_tol", C.c_int32), ("dm_tol", C.c_int32), ("max_width", C.c_int32), ("max_beams", C.c_int32), ("ib_beam", C.c_int32),
                ("ib_ratio", C.c_double)]


class BfEvtEvent(C.Structure):
    """Mirror of ``bf_evt_event`` (include/dsabf.h)."""

    _fields_ = [("best", BfSpsCandidate), ("t_lo", C.c_uint64), ("t_hi", C.c_uint64), ("dm_lo", C.c_int32), ("dm_hi", C.c_int32),
                ("n_members", C.c_int32), ("n_beams", C.c_int32), ("snr_ib", C.c_double), ("flags", C.c_uint32)]


class BfInjTruth(C.Structure):
    """Mirror of ``bf_inj_truth`` (include/dsabf.h)."""

    _fields_ = [("t_lo", C.c_uint64), ("t_hi", C.c_uint64), ("trial", C.c_int32), ("beam", C.c_int32)]


class BfStampRequest(C.Structure):
    """Mirror of ``bf_stamp_request`` (include/dsabf.h)."""

    _fields_ = [("t0", C.c_uint64), ("dm", C.c_int32), ("beam", C.c_int32)]


class BfVcutRequest(C.Structure):
    """Mirror of ``bf_vcut_request`` (include/dsabf.h)."""

    _fields_ = [("t0", C.c_uint64), ("dm", C.c_int32), ("pad", C.c_int32)]


class BfCalOptions(C.Structure):
    """Mirror of ``bf_cal_options`` (include/dsabf.h)."""

    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int), ("ref_ant", C.c_int), ("joint_pol", C.c_int)]


class BfNullOptions(C.Structure):
    """Mirror of ``bf_null_options`` (include/dsabf.h)."""

    _fields_ = [("min_ratio", C.c_double), ("tol", C.c_double), ("n_null", C.c_int), ("max_iter", C.c_int), ("pol", C.c_int)]


class BfSkOptions(C.Structure):
    """Mirror of ``bf_sk_options`` (include/dsabf.h)."""

    _fields_ = [("centre", C.c_double), ("n_sigma", C.c_double), ("max_bad_fraction_ant", C.c_double), ("max_bad_fraction_chan", C.c_double)]


class DsabfError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libdsabf error %d: %s" % (code, msg))
        self.code = code


_lib = None

# name -> (restype, argtypes); every symbol include/dsabf.h declares
SIGNATURES = {
    "bf_last_error": (C.c_char_p, []),
    "bf_version": (C.c_char_p, []),
    "bf_config_default": (C.c_int, [C.POINTER(BfConfig), C.c_int]),
    "bf_n_inputs_per_output": (C.c_int, [C.POINTER(BfConfig)]),
    "bf_n_timesteps_per_gemm": (C.c_int, [C.POINTER(BfConfig)]),
    "bf_bytes_per_gemm": (C.c_size_t, [C.POINTER(BfConfig)]),
    "bf_bytes_per_block": (C.c_size_t, [C.POINTER(BfConfig)]),
    "bf_floats_per_detect": (C.c_size_t, [C.POINTER(BfConfig)]),
    "bf_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "bf_device_name": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "bf_create": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "bf_destroy": (C.c_int, [C.c_void_p]),
    "bf_get_config": (C.c_int, [C.c_void_p, C.POINTER(BfConfig)]),
    "bf_set_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_set_weights_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_alloc_pinned": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "bf_free_pinned": (C.c_int, [C.c_void_p]),
    "bf_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "bf_host_unregister": (C.c_int, [C.c_void_p]),
    "bf_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "bf_event_create_on": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "bf_event_destroy": (C.c_int, [C.c_void_p]),
    "bf_event_query": (C.c_int, [C.c_void_p]),
    "bf_event_synchronize": (C.c_int, [C.c_void_p]),
    "bf_submit_block": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bf_record_transfer_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_enqueue_gemm_unit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "bf_enqueue_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_enqueue_block_dedisperse": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "bf_enqueue_dedisperse": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "bf_record_analysis_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_stream_sync": (C.c_int, [C.c_void_p, C.c_int]),
    "bf_timer_start": (C.c_int, [C.c_void_p]),
    "bf_timer_stop": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "bf_beamform_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_incoherent_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bf_set_incoherent_beam": (C.c_int, [C.c_void_p, C.c_int]),
    "bf_correlate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_corr_entries": (C.c_size_t, [C.POINTER(BfConfig)]),
    "bf_corr_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_corr_destroy": (C.c_int, [C.c_void_p]),
    "bf_corr_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_corr_push_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_corr_dump": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_corr_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bf_corr_pending": (C.c_int, [C.c_void_p]),
    "bf_cal_default_options": (C.c_int, [C.POINTER(BfCalOptions)]),
    "bf_cal_gain_entries": (C.c_size_t, [C.POINTER(BfConfig), C.c_int]),
    "bf_solve_gains_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BfCalOptions), C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "bf_calibrate_weights_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_null_default_options": (C.c_int, [C.POINTER(BfNullOptions)]),
    "bf_null_vec_entries": (C.c_size_t, [C.POINTER(BfConfig), C.c_int]),
    "bf_null_solve_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BfNullOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_null_weights_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "bf_sk_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_sk_entries": (C.c_size_t, [C.POINTER(BfConfig)]),
    "bf_sk_default_options": (C.c_int, [C.POINTER(BfSkOptions)]),
    "bf_sk_select": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(BfSkOptions), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "bf_sk_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_sk_destroy": (C.c_int, [C.c_void_p]),
    "bf_sk_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_sk_push_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_sk_dump": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_sk_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bf_sk_pending": (C.c_int, [C.c_void_p]),
    "bf_stokes_entries": (C.c_size_t, [C.POINTER(BfConfig), C.c_int, C.c_int]),
    "bf_stokes_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_stokes_destroy": (C.c_int, [C.c_void_p]),
    "bf_stokes_set_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "bf_stokes_set_weights_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p]),
    "bf_stokes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_stokes_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_stokes_push_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_stokes_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "bf_stokes_pending": (C.c_int, [C.c_void_p]),
    "bf_expand_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "bf_gemm_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_dedisperse_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_dedisperse_dm_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "bf_dm_stream_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_dm_stream_destroy": (C.c_int, [C.c_void_p]),
    "bf_dm_stream_max_delay": (C.c_int, [C.c_void_p]),
    "bf_dm_stream_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_void_p]),
    "bf_dm_stream_output_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "bf_dm_stream_attach_search": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_sps_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]),
    "bf_sps_destroy": (C.c_int, [C.c_void_p]),
    "bf_sps_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]),
    "bf_sps_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bf_sps_pending": (C.c_int, [C.c_void_p]),
    "bf_sps_last_records": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "bf_sps_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_double,
                                C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bf_cond_default_options": (None, [C.POINTER(BfCondOptions)]),
    "bf_cond_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(BfCondOptions), C.POINTER(C.c_void_p)]),
    "bf_cond_destroy": (C.c_int, [C.c_void_p]),
    "bf_cond_set_mask": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_cond_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_cond_mask_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "bf_dm_stream_attach_conditioner": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_evt_default_options": (None, [C.POINTER(BfEvtOptions)]),
    "bf_evt_create": (C.c_int, [C.POINTER(BfEvtOptions), C.POINTER(C.c_void_p)]),
    "bf_evt_destroy": (C.c_int, [C.c_void_p]),
    "bf_evt_feed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bf_evt_flush": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bf_evt_open": (C.c_int, [C.c_void_p]),
    "bf_dm_stream_create_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_dm_stream_history": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bf_dm_stream_cut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_dm_stream_cut_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_vhist_units_needed": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_vhist_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_vhist_destroy": (C.c_int, [C.c_void_p]),
    "bf_vhist_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_vhist_push_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_vhist_history": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bf_vhist_cut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_vhist_cut_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_stokes_voltage_entries": (C.c_size_t, [C.POINTER(BfConfig), C.c_int]),
    "bf_stokes_voltages_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_cdd_sweep_samples": (C.c_double, [C.c_double, C.c_double, C.c_double]),
    "bf_cdd_edge": (C.c_int, [C.c_double, C.POINTER(C.c_double), C.c_int, C.c_double]),
    "bf_cdd_chirp": (C.c_int, [C.c_double, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]),
    "bf_cdd_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bf_cdd_destroy": (C.c_int, [C.c_void_p]),
    "bf_cdd_set_chirp": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_cdd_voltages_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "bf_cdd_stokes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_rm_lambda2": (C.c_double, [C.c_double]),
    "bf_rm_resolution": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bf_rm_table": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "bf_rm_rmsf": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]),
    "bf_rm_refine": (C.c_int, [C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_double, C.c_void_p]),
    "bf_rm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bf_rm_destroy": (C.c_int, [C.c_void_p]),
    "bf_rm_set_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_rm_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_psr_model_from_spin": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, C.POINTER(BfPsrModel)]),
    "bf_psr_entries": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_psr_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_psr_destroy": (C.c_int, [C.c_void_p]),
    "bf_psr_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_psr_dump": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_psr_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bf_psr_pending": (C.c_int, [C.c_void_p]),
    "bf_psr_beam_snr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_dm_stream_attach_folder": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_ffa_entries": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bf_ffa_rows_of": (C.c_int, [C.c_int, C.c_int]),
    "bf_ffa_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                C.POINTER(C.c_void_p)]),
    "bf_ffa_destroy": (C.c_int, [C.c_void_p]),
    "bf_ffa_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]),
    "bf_ffa_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bf_ffa_pending": (C.c_int, [C.c_void_p]),
    "bf_ffa_last_records": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bf_ffa_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bf_dm_stream_attach_periodicity": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_ffa_set_detrend": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "bf_ffa_detrend": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bf_ffa_sift": (C.c_int, [C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bf_inj_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_inj_destroy": (C.c_int, [C.c_void_p]),
    "bf_inj_add_burst": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bf_inj_add_train": (C.c_int, [C.c_void_p, C.POINTER(BfPsrModel), C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_uint64)]),
    "bf_inj_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bf_inj_next_row": (C.c_uint64, [C.c_void_p]),
    "bf_inj_launches": (C.c_uint64, [C.c_void_p]),
    "bf_inj_burst_profile": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_inj_nearest_trial": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "bf_inj_match": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64, C.c_int32, C.c_void_p]),
    "bf_dm_stream_attach_injector": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bf_comm_unique_id": (C.c_int, [C.c_void_p]),
    "bf_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_comm_destroy": (C.c_int, [C.c_void_p]),
    "bf_comm_rank": (C.c_int, [C.c_void_p]),
    "bf_comm_world": (C.c_int, [C.c_void_p]),
    "bf_comm_library_info": (C.c_int, [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "bf_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "bf_gather_detected": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_gather_detected_staged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bf_gather_offset": (C.c_size_t, [C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_size_t]),
    "bf_gather_rows_held": (C.c_size_t, [C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "bf_gather_plan": (C.c_size_t, [C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(BfGatherMsg),
                                    C.c_size_t]),
    "bf_block_output_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_queue_stream": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_block_gather_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_block_gather_stage_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bf_enqueue_d2h": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "bf_dedisperse_band_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bf_dedisperse_dm_band_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p]),
    "bf_gather_relayout_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_void_p]),
    "bf_set_switch": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "bf_get_counter": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]),
    "bf_rtw_plan": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bf_kernel_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_int)]),
    "bf_kernel_name": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "bf_mfma_peak_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double),
                                    C.c_void_p]),
    "bf_launch_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                               C.c_char_p, C.c_size_t]),
    "bf_enqueue_block_to": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bf_dm_stream_reserve": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "bf_variant_key": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "bf_handle_variant_key": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]),
    "bf_stage_launches": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int]),
    # ---- include/dsabf_host.h ----
    "bfh_default_positions": (C.c_int, [C.c_int, C.c_void_p]),
    "bfh_default_directions": (C.c_int, [C.c_int, C.c_void_p]),
    "bfh_read_positions": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p]),
    "bfh_read_directions": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p]),
    "bfh_count_entries": (C.c_int, [C.c_char_p]),
    "bfh_write_python_file": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p]),
    "bfh_channel_frequency": (C.c_float, [C.c_int, C.c_int, C.c_int]),
    "bfh_make_weights": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bfh_gen_create": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bfh_gen_destroy": (C.c_int, [C.c_void_p]),
    "bfh_gen_read_sources": (C.c_int, [C.c_void_p, C.c_char_p]),
    "bfh_gen_set_sources": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "bfh_gen_generate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "bfh_gen_data": (C.c_void_p, [C.c_void_p]),
    "bfh_gen_size": (C.c_size_t, [C.c_void_p]),
    "bfh_gen_n_pt_sources": (C.c_int, [C.c_void_p]),
    "bfh_gen_need_more": (C.c_int, [C.c_void_p, C.c_int]),
    "bfh_gen_ready": (C.c_int, [C.c_void_p, C.c_int]),
    "bfh_obs_create": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(BfConfig), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "bfh_obs_destroy": (C.c_int, [C.c_void_p]),
    "bfh_obs_generate_transfer_event": (C.c_int, [C.c_void_p]),
    "bfh_obs_generate_analysis_event": (C.c_int, [C.c_void_p]),
    "bfh_obs_check_transfer_events": (C.c_int, [C.c_void_p]),
    "bfh_obs_check_analysis_events": (C.c_int, [C.c_void_p]),
    "bfh_obs_counters": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint64)] * 4),
    "bfh_obs_check_ready_for_transfer": (C.c_int, [C.c_void_p]),
    "bfh_obs_check_ready_for_analysis": (C.c_int, [C.c_void_p]),
    "bfh_obs_check_ready_for_dh2_transfer": (C.c_int, [C.c_void_p, C.c_int]),
    "bfh_obs_check_observations_complete": (C.c_int, [C.c_void_p]),
    "bfh_obs_check_transfers_complete": (C.c_int, [C.c_void_p]),
    "bfh_obs_set_transfers_complete": (C.c_int, [C.c_void_p, C.c_int]),
    "bfh_obs_set_n_pt_sources": (C.c_int, [C.c_void_p, C.c_int]),
    "bfh_obs_get_current_analysis_gemm": (C.c_uint64, [C.c_void_p, C.c_int]),
    "bfh_obs_get_current_transfer_gemm": (C.c_uint64, [C.c_void_p]),
    "bfh_obs_get_next_gpu_analysis_block": (C.c_uint64, [C.c_void_p]),
    "bfh_obs_get_next_gpu_transfer_block": (C.c_uint64, [C.c_void_p]),
    "bfh_obs_describe": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "bfh_obs_create_custom": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(BfConfig), C.POINTER(BfhEventOps), C.c_int,
                                        C.POINTER(C.c_void_p)]),
    "bfh_obs_status": (C.c_int, [C.c_void_p]),
    "bfh_run_observation_junk": (C.c_int, [C.POINTER(BfConfig), C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "bfh_run_observation_junk_to_file": (C.c_int, [C.POINTER(BfConfig), C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_int,
                                                   C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_float),
                                                   C.POINTER(C.c_uint64), C.c_void_p]),
    "bfh_run_observation_junk_dm": (C.c_int, [C.POINTER(BfConfig), C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_float),
                                              C.POINTER(C.c_uint64), C.c_void_p]),
    "bfh_run_observation_junk_sharded": (C.c_int, [C.POINTER(BfConfig), C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                                   C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.c_void_p]),
    "bfh_run_observation_junk_to_ring": (C.c_int, [C.POINTER(BfConfig), C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_int,
                                                   C.c_char_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint64),
                                                   C.c_void_p]),
    "bfh_file_sink_create": (C.c_int, [C.POINTER(BfConfig), C.c_char_p, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "bfh_sink_acquire": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.POINTER(C.c_float))]),
    "bfh_sink_commit": (C.c_int, [C.c_void_p, C.c_uint64]),
    "bfh_sink_close": (C.c_int, [C.c_void_p]),
    "bfh_sink_destroy": (C.c_int, [C.c_void_p]),
    "bfh_dm_trials": (C.c_int, [C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                C.c_double, C.POINTER(C.c_double), C.c_int]),
    "bfh_dm_delays": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_float), C.c_int, C.c_double, C.c_double,
                                C.POINTER(C.c_int32)]),
    "bfh_dm_sink_create": (C.c_int, [C.POINTER(BfConfig), C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bfh_dm_sink_deliver": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "bfh_dm_sink_destroy": (C.c_int, [C.c_void_p]),
    "bfh_event_sink_create": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "bfh_event_sink_deliver": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "bfh_event_sink_destroy": (C.c_int, [C.c_void_p]),
    "bfh_stamp_sink_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bfh_stamp_sink_deliver": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int]),
    "bfh_stamp_sink_destroy": (C.c_int, [C.c_void_p]),
    "bfh_voltage_sink_create": (C.c_int, [C.c_char_p, C.POINTER(BfConfig), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bfh_voltage_sink_deliver": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_size_t]),
    "bfh_voltage_sink_destroy": (C.c_int, [C.c_void_p]),
    "bfh_psr_sink_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "bfh_psr_sink_deliver": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "bfh_psr_sink_destroy": (C.c_int, [C.c_void_p]),
    "bfh_ffa_sink_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]),
    "bfh_ffa_sink_create_detrend": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                              C.POINTER(C.c_void_p)]),
    "bfh_ffa_sink_deliver": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "bfh_ffa_sink_destroy": (C.c_int, [C.c_void_p]),
    "bfh_dm_trial_share": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bfh_junk_fill": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_uint64, C.c_void_p]),
    "bfh_shm_ring_create": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(C.c_void_p)]),
    "bfh_shm_ring_attach": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "bfh_shm_ring_detach": (C.c_int, [C.c_void_p]),
    "bfh_shm_ring_unlink": (C.c_int, [C.c_char_p]),
    "bfh_shm_ring_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "bfh_shm_ring_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "bfh_shm_ring_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bfh_run_observation_shm_dm": (C.c_int, [C.POINTER(BfConfig), C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p,
                                             C.c_int, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_int)]),
    "bfh_run_observation_shm": (C.c_int, [C.POINTER(BfConfig), C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                          C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "bfh_run_debug_observation": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                            C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                            C.POINTER(C.c_float)]),
    "bfh_run_debug_observation2": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                             C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                             C.POINTER(C.c_float), C.c_int]),
    "bfh_run_debug_observation3": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                             C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                             C.POINTER(C.c_float), C.c_int, C.c_char_p, C.c_void_p]),
    "bfh_run_debug_observation4": (C.c_int, [C.POINTER(BfConfig), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                             C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                             C.POINTER(C.c_float), C.c_int, C.c_char_p, C.c_char_p, C.c_void_p]),
}


_hip = None
_rccl_path = None


def _preload_hip_runtime():
    """libdsabf.so carries no DT_NEEDED for the HIP runtime (see build.py): make exactly ONE libamdhip64 visible
    process-wide before loading it -- torch's bundled copy when torch is installed (so that torch streams, events
    and allocations belong to the same runtime as our launches), else the system ROCm one."""
    global _hip
    if _hip is not None:
        return _hip
    cands = []
    try:
        import torch  # noqa: F401  (plumbing only: device memory, streams, torch.distributed)

        cands.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except ImportError:
        pass
    cands += [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"), "libamdhip64.so"]
    errs = []
    for c in cands:
        if os.path.sep in c and not os.path.exists(c):
            continue
        try:
            _hip = C.CDLL(c, mode=C.RTLD_GLOBAL)
            # RCCL must come from the same place as the HIP runtime (bf_comm.cpp binds it with dlopen at first use):
            # torch's bundled librccl.so next to torch's libamdhip64.so, ROCm's next to ROCm's.
            global _rccl_path
            for r in ("librccl.so", "librccl.so.1"):
                rp = os.path.join(os.path.dirname(c), r) if os.path.sep in c else r
                if os.path.sep in rp and os.path.exists(rp):
                    # only a file that exists: a bare soname would turn bf_comm.cpp's soft resolution order (a copy
                    # already in the process, librccl.so.1, librccl.so) into its hard-fail DSABF_RCCL_LIB branch
                    _rccl_path = rp
                    os.environ.setdefault("DSABF_RCCL_LIB", rp)
                    break
            return _hip
        except OSError as e:  # pragma: no cover
            errs.append("%s: %s" % (c, e))
    raise ImportError("no HIP runtime (libamdhip64.so) could be loaded: %s" % "; ".join(errs))


def load() -> C.CDLL:
    """Load libdsabf.so (built by ``dsabeamformer_amd.build.build()`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -m dsabeamformer_amd.build` (hipcc, gfx950). "
                "There is no CPU fallback for the beamformer hot path." % LIB_PATH)
        _preload_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
            except AttributeError:
                if os.environ.get("DSABF_LIB_PATH"):   # a measurement build of another round beside the product (tools/ab_libs.py):
                    continue                           # it may predate an export; calling that one fails, the rest works
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise DsabfError(rc, load().bf_last_error().decode(errors="replace"))
    return rc
