"""Object wrapper over the C-ABI (include/dsabf.h) for Python callers that own device memory through torch.

Names follow the reference: a *gemm-unit* is the work of one cublasGemmStridedBatchedEx call
(src/beamformer.cu:470-477), a *block* is a PSRDADA block of ``n_gemms_per_block`` gemm-units, a *beam-block* is
one detected ``[n_freq][n_beams]`` float32 output.
"""
from __future__ import annotations

import ctypes as C

from ._lib import BF_CAL_FULL, BF_CAL_PHASE, BF_NULL_CLIP, BF_NULL_SCALED, BfCalOptions, BfNullOptions, BfCondOptions, BfConfig, BfFfaCandidate, BfFfaGroup, BfFfaPeak, BfFfaStat, BfInjTruth, BfPsrModel, BfEvtEvent, BfEvtOptions, BfSkOptions, BfStampRequest, BfVcutRequest, DsabfError, BfSpsCandidate, BfSpsPeak, BfSpsStat, check, load


def debug_config(**over) -> BfConfig:
    """The reference's ``make debug`` geometry (N_AVERAGING = 1, src/beamformer.hh:55-57)."""
    cfg = BfConfig()
    check(load().bf_config_default(C.byref(cfg), 1))
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def production_config(**over) -> BfConfig:
    """The reference's production geometry (N_AVERAGING = 16, src/beamformer.hh:59)."""
    cfg = BfConfig()
    check(load().bf_config_default(C.byref(cfg), 0))
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def launch_plan(cfg: BfConfig, paired: bool, n_units: int = 1, n_cus: int = 256) -> dict:
    """Which fused kernel and launch shape ``cfg`` would run (bf_launch_plan: host arithmetic, no device needed)."""
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    name = C.create_string_buffer(200)
    check(load().bf_launch_plan(C.byref(cfg), int(paired), n_units, n_cus, C.byref(g), C.byref(b), C.byref(l), name, 200))
    return {"kernel": name.value.decode(), "grid": g.value, "block": b.value, "lds_bytes": l.value}


def variant_key(cfg: BfConfig, paired: bool, write_c: bool = False) -> str:
    """The compiled kernel instantiation ``cfg`` selects, as its demangled symbol spells the template arguments
    (bf_variant_key: host arithmetic; the census of tests/test_census_cpu.py)."""
    buf = C.create_string_buffer(120)
    check(load().bf_variant_key(C.byref(cfg), int(paired), int(write_c), buf, 120))
    return buf.value.decode()


def stage_launches(clear: bool = False) -> list[str]:
    """The stage kernels the calling thread launched most recently (at most 32, oldest first), as their demangled symbols spell
    them -- "cdd_kernel<9, true>", "corr_kernel" (bf_stage_launches: the launchers' own record); ``clear`` empties the record."""
    buf = C.create_string_buffer(32 * 64 + 1)
    check(load().bf_stage_launches(buf, len(buf), int(clear)))
    return buf.value.decode().split("\n")[:-1]


def _ptr(x) -> C.c_void_p:
    """Accept ints, ctypes pointers, numpy arrays (host) and torch tensors (device or host)."""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if hasattr(x, "ctypes"):
        return C.c_void_p(x.ctypes.data)
    return x


class _Owner:
    """Owns one pointer of the C-ABI: the attribute named ``_ptr_attr`` (``_h``, ``_s`` or ``_c``), destroyed once by the library
    function named ``_destroy``."""
    _ptr_attr = _destroy = ""

    def close(self) -> None:
        if getattr(self, self._ptr_attr, None):
            getattr(self._lib, self._destroy)(getattr(self, self._ptr_attr))
            setattr(self, self._ptr_attr, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Beamformer(_Owner):
    """One handle = one GPU = one frequency shard (the reference runs one process per GPU, README.md:168)."""
    _ptr_attr, _destroy = "_h", "bf_destroy"

    def __init__(self, cfg: BfConfig, device: int = 0):
        self._lib = load()
        self._h = C.c_void_p()
        self.cfg = cfg
        check(self._lib.bf_create(C.byref(cfg), device, C.byref(self._h)))

    # -- geometry -----------------------------------------------------------------------------------------
    @property
    def n_ipo(self) -> int:
        return self._lib.bf_n_inputs_per_output(C.byref(self.cfg))

    @property
    def n_time(self) -> int:
        return self._lib.bf_n_timesteps_per_gemm(C.byref(self.cfg))

    @property
    def bytes_per_gemm(self) -> int:
        return self._lib.bf_bytes_per_gemm(C.byref(self.cfg))

    @property
    def bytes_per_block(self) -> int:
        return self._lib.bf_bytes_per_block(C.byref(self.cfg))

    @property
    def floats_per_detect(self) -> int:
        return self._lib.bf_floats_per_detect(C.byref(self.cfg))

    # -- setup --------------------------------------------------------------------------------------------
    def set_weights(self, w_host) -> None:
        """``w_host``: int8 host array [freq][ant][beam][2] (reference layout)."""
        check(self._lib.bf_set_weights(self._h, _ptr(w_host)))

    def set_weights_device(self, d_w, stream: int = 0) -> None:
        check(self._lib.bf_set_weights_device(self._h, _ptr(d_w), C.c_void_p(stream)))

    # -- device-pointer entry points -------------------------------------------------------------------------
    def beamform(self, d_packed, n_units: int, d_out, stream: int = 0) -> None:
        check(self._lib.bf_beamform_device(self._h, _ptr(d_packed), int(n_units), _ptr(d_out), C.c_void_p(stream)))

    def incoherent(self, d_packed, n_units: int, d_out, stride: int = 1, stream: int = 0) -> None:
        """bf_incoherent_device: the incoherent beam of n_units gemm-units, one float per (unit, output, freq) ``stride`` floats apart."""
        check(self._lib.bf_incoherent_device(self._h, _ptr(d_packed), int(n_units), _ptr(d_out), int(stride), C.c_void_p(stream)))

    def set_incoherent_beam(self, beam: int) -> None:
        """bf_set_incoherent_beam: every detect launch from now on overwrites beam column ``beam`` with the incoherent beam (-1: off)."""
        check(self._lib.bf_set_incoherent_beam(self._h, int(beam)))

    def correlate(self, d_packed, n_units: int, d_vis, accumulate: bool = False, stream: int = 0) -> None:
        """bf_correlate_device: the visibilities of n_units gemm-units into d_vis, int64 [freq][pol][a1 (a1 + 1) / 2 + a2]{re, im}
        (``corr_entries`` entries), overwritten or -- ``accumulate`` -- added to.  Needs no weights."""
        check(self._lib.bf_correlate_device(self._h, _ptr(d_packed), int(n_units), _ptr(d_vis), int(bool(accumulate)), C.c_void_p(stream)))

    @property
    def corr_entries(self) -> int:
        """bf_corr_entries: n_freq * n_pol * n_ant (n_ant + 1) / 2 complex entries (two int64 each)."""
        return self._lib.bf_corr_entries(C.byref(self.cfg))

    def voltage_moments(self, d_packed, n_units: int, d_moments, accumulate: bool = False, stream: int = 0) -> None:
        """bf_sk_device (docs/SPECTRAL_KURTOSIS.md): the power moments of n_units gemm-units into d_moments, int64 [freq][pol][ant]{m1, m2}
        (``sk_entries`` cells), overwritten or -- ``accumulate`` -- added to.  Needs no weights."""
        check(self._lib.bf_sk_device(self._h, _ptr(d_packed), int(n_units), _ptr(d_moments), int(bool(accumulate)), C.c_void_p(stream)))

    @property
    def sk_entries(self) -> int:
        """bf_sk_entries: n_freq * n_pol * n_ant cells (two int64 each)."""
        return self._lib.bf_sk_entries(C.byref(self.cfg))

    def solve_gains(self, d_vis, d_gains, d_info, model=None, flags=None, tol: float = 1e-10, max_iter: int = 200, ref_ant: int = -1,
                    joint_pol: bool = False, stream: int = 0) -> None:
        """bf_solve_gains_device (docs/CALIBRATION.md): the visibilities d_vis (as ``correlate`` leaves them) -> d_gains, float64
        [pol_out][freq][ant]{re, im} (``gain_entries(joint_pol)`` complex entries), and d_info, int32 [pol_out][freq]{iterations,
        status}.  ``model``: float64 [freq][ant]{re, im} on the device or None (all ones); ``flags``: uint8 [ant] on the device or None."""
        opt = BfCalOptions(float(tol), int(max_iter), int(ref_ant), int(bool(joint_pol)))
        check(self._lib.bf_solve_gains_device(self._h, _ptr(d_vis), _ptr(model), _ptr(flags), C.byref(opt), _ptr(d_gains), _ptr(d_info),
                                              C.c_void_p(stream)))

    def calibrate_weights(self, d_w_in, d_gains_layer, d_w_out, flags=None, mode: str = "phase", stream: int = 0) -> None:
        """bf_calibrate_weights_device: d_w_out = d_w_in times conj(g) / |g| (``mode`` "phase"), times k_f / |g| as well ("full"),
        rounded half to even and clipped to +-127; int8 [freq][ant][beam]{re, im}, the array ``set_weights_device`` takes."""
        modes = {"phase": BF_CAL_PHASE, "full": BF_CAL_FULL}
        if mode not in modes:
            raise ValueError("mode must be 'phase' or 'full', not %r" % (mode,))
        check(self._lib.bf_calibrate_weights_device(self._h, _ptr(d_w_in), _ptr(d_gains_layer), _ptr(flags), modes[mode], _ptr(d_w_out),
                                                    C.c_void_p(stream)))

    def gain_entries(self, joint_pol: bool = False) -> int:
        """bf_cal_gain_entries: (joint_pol ? 1 : n_pol) * n_freq * n_ant complex entries (two float64 each)."""
        return self._lib.bf_cal_gain_entries(C.byref(self.cfg), int(bool(joint_pol)))

    def null_solve(self, d_vis, d_vecs, d_eig, d_info, flags=None, n_null: int = 1, min_ratio: float = 4.0, tol: float = 1e-6,
                   max_iter: int = 200, pol: int = -1, stream: int = 0) -> None:
        """bf_null_solve_device (docs/NULLING.md): the visibilities d_vis (as ``correlate`` leaves them) -> d_vecs, float64
        [freq][n_null][ant]{re, im} (``null_vec_entries(n_null)`` complex entries; exact zeros where unused), d_eig, float64
        [freq][n_null + 1] (the lambdas, then the trace), and d_info, int32 [freq][1 + 2 n_null] (n_used, then {iterations, status} per
        vector).  ``flags``: uint8 [ant] on the device or None; ``pol`` -1: the polarisations are added first."""
        opt = BfNullOptions(float(min_ratio), float(tol), int(n_null), int(max_iter), int(pol))
        check(self._lib.bf_null_solve_device(self._h, _ptr(d_vis), _ptr(flags), C.byref(opt), _ptr(d_vecs), _ptr(d_eig), _ptr(d_info),
                                             C.c_void_p(stream)))

    def null_weights(self, d_w_in, d_vecs, d_info, d_w_out, n_null: int, flags=None, mode: str = "scaled", scale=None, stream: int = 0) -> None:
        """bf_null_weights_device: d_w_out = d_w_in with the used vectors of every channel projected out, w' = w - sum_j conj(u_j) (u_j^T w),
        times k_f = min(1, 127 / max |part|) (``mode`` "scaled") or 1 ("clip"), rounded half to even and clipped to +-127; int8
        [freq][ant][beam]{re, im}, the array ``set_weights_device`` takes.  ``scale``: float64 [freq] on the device or None, receives k_f."""
        modes = {"scaled": BF_NULL_SCALED, "clip": BF_NULL_CLIP}
        if mode not in modes:
            raise ValueError("mode must be 'scaled' or 'clip', not %r" % (mode,))
        check(self._lib.bf_null_weights_device(self._h, _ptr(d_w_in), _ptr(d_vecs), _ptr(d_info), int(n_null), _ptr(flags), modes[mode],
                                               _ptr(d_w_out), _ptr(scale), C.c_void_p(stream)))

    def null_vec_entries(self, n_null: int = 1) -> int:
        """bf_null_vec_entries: n_freq * n_null * n_ant complex entries (two float64 each); 0 for an n_null outside 1 ... 4."""
        return self._lib.bf_null_vec_entries(C.byref(self.cfg), int(n_null))

    def expand(self, d_in, nbytes: int, d_out, stream: int = 0) -> None:
        check(self._lib.bf_expand_device(self._h, _ptr(d_in), int(nbytes), _ptr(d_out), C.c_void_p(stream)))

    def gemm(self, d_packed_unit, d_c, stream: int = 0) -> None:
        check(self._lib.bf_gemm_device(self._h, _ptr(d_packed_unit), _ptr(d_c), C.c_void_p(stream)))

    def dedisperse(self, d_out_unit, d_ded, stream: int = 0) -> None:
        check(self._lib.bf_dedisperse_device(self._h, _ptr(d_out_unit), _ptr(d_ded), C.c_void_p(stream)))

    def dedisperse_dm(self, d_series, n_t: int, d_delays, n_dm: int, n_t_out: int, d_out, stream: int = 0) -> None:
        """d_series float32 [n_t][freq][beam], d_delays int32 [n_dm][freq] -> d_out float32 [n_dm][n_t_out][beam]."""
        check(self._lib.bf_dedisperse_dm_device(self._h, _ptr(d_series), int(n_t), _ptr(d_delays), int(n_dm),
                                                int(n_t_out), _ptr(d_out), C.c_void_p(stream)))

    def dedisperse_band(self, d_out_unit, n_freq_total: int, d_ded, stream: int = 0) -> None:
        check(self._lib.bf_dedisperse_band_device(self._h, _ptr(d_out_unit), n_freq_total, _ptr(d_ded), C.c_void_p(stream)))

    def dedisperse_dm_band(self, d_series, n_t: int, n_freq_total: int, d_delays, n_dm: int, n_t_out: int, d_out,
                           stream: int = 0) -> None:
        check(self._lib.bf_dedisperse_dm_band_device(self._h, _ptr(d_series), n_t, n_freq_total, _ptr(d_delays), n_dm, n_t_out,
                                                     _ptr(d_out), C.c_void_p(stream)))

    # -- streaming entry points (the reference's observation loop) ---------------------------------------------
    def submit_block(self, slot: int, host, nbytes: int, event=None) -> None:
        check(self._lib.bf_submit_block(self._h, slot, _ptr(host), nbytes, _ptr(event)))

    def enqueue_gemm_unit(self, stream_idx: int, slot: int, time_slice: int, host_out=None) -> None:
        check(self._lib.bf_enqueue_gemm_unit(self._h, stream_idx, slot, time_slice, _ptr(host_out)))

    def enqueue_block(self, stream_idx: int, slot: int, first_unit: int, n_units: int, host_outs=None) -> None:
        """One launch over n_units consecutive gemm-units of a ring slot; host_outs: n_units host pointers (or None)."""
        arr = None
        if host_outs is not None:
            arr = (C.c_void_p * n_units)(*[_ptr(p).value for p in host_outs])
        check(self._lib.bf_enqueue_block(self._h, stream_idx, slot, first_unit, n_units, arr))

    def enqueue_block_to(self, stream_idx: int, slot: int, first_unit: int, n_units: int, d_dst, host_outs=None) -> None:
        """enqueue_block with the powers written to the device address d_dst ([unit][o][f][b]) instead of the queue's buffer."""
        arr = None
        if host_outs is not None:
            arr = (C.c_void_p * n_units)(*[_ptr(p).value for p in host_outs])
        check(self._lib.bf_enqueue_block_to(self._h, stream_idx, slot, first_unit, n_units, _ptr(d_dst), arr))

    def enqueue_block_dedisperse(self, stream_idx: int, first_unit: int, n_units: int, host_rows=None) -> None:
        check(self._lib.bf_enqueue_block_dedisperse(self._h, stream_idx, first_unit, n_units, _ptr(host_rows)))

    def enqueue_dedisperse(self, stream_idx: int, host_out_row=None) -> None:
        check(self._lib.bf_enqueue_dedisperse(self._h, stream_idx, _ptr(host_out_row)))

    def queue_stream(self, stream_idx: int) -> int:
        """bf_queue_stream: the hipStream_t of compute queue stream_idx (launches what is still only queued first)."""
        p = C.c_void_p()
        check(self._lib.bf_queue_stream(self._h, stream_idx, C.byref(p)))
        return p.value or 0

    def block_output_device(self, stream_idx: int) -> int:
        """bf_block_output_device: device pointer of the queue's block buffer [n_gemms_per_block][output][freq][beam]."""
        p = C.c_void_p()
        check(self._lib.bf_block_output_device(self._h, stream_idx, C.byref(p)))
        return p.value or 0

    def enqueue_d2h(self, stream_idx: int, d_src, host_dst, n_floats: int) -> None:
        check(self._lib.bf_enqueue_d2h(self._h, stream_idx, _ptr(d_src), _ptr(host_dst), n_floats))

    def record_analysis_event(self, event) -> None:
        check(self._lib.bf_record_analysis_event(self._h, _ptr(event)))

    def sync(self, stream_idx: int = -1) -> None:
        check(self._lib.bf_stream_sync(self._h, stream_idx))

    def timer_start(self) -> None:
        check(self._lib.bf_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float()
        check(self._lib.bf_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def mfma_peak(self, d_operands, operand_bytes: int, d_scratch, scratch_bytes: int, iters: int, stream) -> float:
        """One launch of back-to-back v_mfma_i32_16x16x64_i8 on the caller's operand bytes; returns the int8 ops it executes."""
        ops = C.c_double()
        check(self._lib.bf_mfma_peak_device(self._h, _ptr(d_operands), operand_bytes, _ptr(d_scratch), scratch_bytes, iters,
                                            C.byref(ops), C.c_void_p(stream)))
        return ops.value

    def gather_relayout(self, d_stage, d_full, rows_held: int, world: int, row_floats: int, skip_rank: int, stream: int = 0) -> None:
        """bf_gather_relayout_device (dsabf_bench.h): the staged transport's device pass by itself."""
        check(self._lib.bf_gather_relayout_device(self._h, _ptr(d_stage), _ptr(d_full), rows_held, world, row_floats, skip_rank,
                                                  C.c_void_p(stream)))

    def set_switch(self, name: str, value: int) -> None:
        """bf_set_switch: a measurement / test switch of this handle ("tsplit", "lds_pad", "dm_wide", "paired", "fold")."""
        check(self._lib.bf_set_switch(self._h, name.encode(), int(value)))

    def counter(self, name: str) -> int:
        """bf_get_counter: "fused_launches", "queued_units", "dm_ring_stages", "fold_stream"; "dm_wide_groups" / "dm_wide_mask": the
        trial groups the shared-window DM kernel took in the most recent DM launch (these two wait for that launch's stream)."""
        v = C.c_uint64()
        check(self._lib.bf_get_counter(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def kernel_info(self, n_units: int = 1) -> dict:
        g, b, l, v = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self._lib.bf_kernel_info(self._h, n_units, C.byref(g), C.byref(b), C.byref(l), C.byref(v)))
        name = C.create_string_buffer(160)
        check(self._lib.bf_kernel_name(self._h, name, 160))
        # "launch": the kernel template the fused launch instantiates; variant_key() and "kernel" name the antenna-fold FAMILY, whose
        # launches of whole chunk spans are fused16_fold_stream_kernel
        key = self.variant_key()
        launch = key.split("<")[0]
        if launch == "fused16_fold_kernel":
            v64 = C.c_uint64()   # (an A/B library of an earlier build, DSABF_LIB_PATH, has neither the counter nor the streamed kernel)
            if self._lib.bf_get_counter(self._h, b"fold_stream", C.byref(v64)) == 0 and v64.value:
                launch = "fused16_fold_stream_kernel"
        return {"kernel": name.value.decode(), "grid": g.value, "block": b.value, "lds_bytes": l.value,
                "vgprs": v.value, "launch": launch}

    def variant_key(self, write_c: bool = False) -> str:
        """The instantiation this handle launches (after set_weights decided general / conjugate-pair)."""
        buf = C.create_string_buffer(120)
        check(self._lib.bf_handle_variant_key(self._h, int(write_c), buf, 120))
        return buf.value.decode()


class DmStream(_Owner):
    """bf_dm_stream: DM-trial dedispersion of the detected stream, block by block, with the delay window carried over on the
    device (include/dsabf.h).  delays: int32 host array [n_dm][n_freq_total]."""
    _ptr_attr, _destroy = "_s", "bf_dm_stream_destroy"

    def __init__(self, bf: Beamformer, delays, n_freq_total: int, max_rows_per_push: int, history_rows: int = 0):
        import numpy as np

        self._lib = load()
        self._s = C.c_void_p()
        d = np.ascontiguousarray(delays, np.int32)
        assert d.ndim == 2 and d.shape[1] == n_freq_total
        self.n_dm, self.n_beams, self._bf = d.shape[0], bf.cfg.n_beams, bf
        # history_rows: rows kept for cut(), beyond what the pushes in flight need.  0 goes through bf_dm_stream_create (the same
        # stage): a measurement build of an earlier round beside the product (DSABF_LIB_PATH) has only that export.
        if history_rows:
            check(self._lib.bf_dm_stream_create_history(bf._h, _ptr(d), d.shape[0], n_freq_total, max_rows_per_push, history_rows, C.byref(self._s)))
        else:
            check(self._lib.bf_dm_stream_create(bf._h, _ptr(d), d.shape[0], n_freq_total, max_rows_per_push, C.byref(self._s)))

    @property
    def max_delay(self) -> int:
        return self._lib.bf_dm_stream_max_delay(self._s)

    def push(self, d_rows, n_rows: int, host_out=None, stream: int = 0):
        """Returns (first_t, n_t_out) of the chunk this push emits ([n_dm][n_t_out][beam] into host_out, asynchronously)."""
        first, n = C.c_uint64(), C.c_int()
        check(self._lib.bf_dm_stream_push(self._s, _ptr(d_rows), n_rows, _ptr(host_out), C.byref(first), C.byref(n), C.c_void_p(stream)))
        return int(first.value), int(n.value)

    def reserve(self, n_rows: int, stream: int = 0) -> int:
        """Device address of the next n_rows rows' place inside the stage's buffer (bf_dm_stream_reserve): write them there on
        ``stream``, then push(that address, n_rows) -- no copy."""
        p = C.c_void_p()
        check(self._lib.bf_dm_stream_reserve(self._s, n_rows, C.byref(p), C.c_void_p(stream)))
        return p.value or 0

    def output_device(self) -> int:
        p = C.c_void_p()
        check(self._lib.bf_dm_stream_output_device(self._s, C.byref(p)))
        return p.value or 0

    def attach_search(self, sps) -> None:
        """bf_dm_stream_attach_search: every chunk a push emits from now on also goes into ``sps`` (a SinglePulseSearch; None
        detaches), on the push's queue."""
        check(self._lib.bf_dm_stream_attach_search(self._s, sps._s if sps is not None else None))

    def attach_conditioner(self, cond) -> None:
        """bf_dm_stream_attach_conditioner: every push from now on conditions its new rows in the stage's buffer (``cond``: a
        Conditioner; None detaches) before they are dedispersed."""
        check(self._lib.bf_dm_stream_attach_conditioner(self._s, cond._c if cond is not None else None))

    def attach_folder(self, folder) -> None:
        """bf_dm_stream_attach_folder: every push from now on also folds its new rows where they lie in the stage's buffer
        (``folder``: a PulsarFolder; None detaches), behind an attached conditioner."""
        check(self._lib.bf_dm_stream_attach_folder(self._s, folder._c if folder is not None else None))

    def attach_periodicity(self, ffa) -> None:
        """bf_dm_stream_attach_periodicity: every chunk a push emits from now on also goes into ``ffa`` (a PeriodicitySearch; None
        detaches), behind an attached search stage."""
        check(self._lib.bf_dm_stream_attach_periodicity(self._s, ffa._s if ffa is not None else None))

    def attach_injector(self, inj) -> None:
        """bf_dm_stream_attach_injector: every push from now on adds the live pulses of ``inj`` (an Injector; None detaches) to its new
        rows where they lie in the stage's buffer, in front of an attached conditioner."""
        check(self._lib.bf_dm_stream_attach_injector(self._s, inj._c if inj is not None else None))

    def history(self):
        """bf_dm_stream_history: (oldest_row, next_row, cap_rows) -- rows [oldest_row, next_row) of the series can be cut."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.bf_dm_stream_history(self._s, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def cut(self, requests, n_tau: int, tbin: int, fbin: int, d_out, stream: int = 0):
        """bf_dm_stream_cut: dedispersed stamps [request][n_freq_total / fbin][n_tau] (fp32, device memory ``d_out``) of the
        requests -- an iterable of (t0, local trial, beam), or a structured array with fields t0, dm, beam -- asynchronously on
        ``stream``.  Returns the int32 status of every request: 0 cut, 1 too old, 2 not pushed yet (its cells stay untouched)."""
        import numpy as np

        reqs = np.zeros(len(requests), stamp_request_dtype())
        if len(requests):
            r = np.asarray(requests)
            if r.dtype.names:
                for k in ("t0", "dm", "beam"):
                    reqs[k] = r[k]
            else:
                reqs["t0"], reqs["dm"], reqs["beam"] = [[int(q[k]) for q in requests] for k in range(3)]
        status = np.full(len(reqs), -1, np.int32)
        check(self._lib.bf_dm_stream_cut(self._s, _ptr(reqs), len(reqs), n_tau, tbin, fbin, _ptr(d_out), _ptr(status), C.c_void_p(stream)))
        return status


def stamp_request_dtype():
    import numpy as np

    dt = np.dtype([("t0", np.uint64), ("dm", np.int32), ("beam", np.int32)], align=True)
    assert dt.itemsize == C.sizeof(BfStampRequest)
    return dt


def vcut_request_dtype():
    import numpy as np

    dt = np.dtype([("t0", np.uint64), ("dm", np.int32), ("pad", np.int32)], align=True)
    assert dt.itemsize == C.sizeof(BfVcutRequest)
    return dt


def vhist_units_needed(cfg: BfConfig, max_delay_rows: int, dm_rows: int, n_buf: int, t_tol: int, max_width: int, cut_units: int) -> int:
    """bf_vhist_units_needed: the history (whole gemm-units) with which a consumer that cuts ``cut_units`` units around an event when it
    closes misses nothing (docs/VOLTAGE_CUTS.md section 3); 0 where undefined.  Host arithmetic, no device."""
    return int(load().bf_vhist_units_needed(C.byref(cfg), max_delay_rows, dm_rows, n_buf, t_tol, max_width, cut_units))


class VoltageHistory(_Owner):
    """bf_vhist: a device ring of the last ``history_units`` whole gemm-units of packed voltages, and dedispersed cuts of it in the input
    layout [unit][freq][time][ant] (include/dsabf.h, docs/VOLTAGE_CUTS.md).  delays: int32 host array [n_dm][n_freq], in samples."""
    _ptr_attr, _destroy = "_c", "bf_vhist_destroy"

    def __init__(self, bf: Beamformer, delays, history_units: int):
        import numpy as np

        self._lib = load()
        self._c = C.c_void_p()
        d = np.ascontiguousarray(delays, np.int32)
        assert d.ndim == 2 and d.shape[1] == bf.cfg.n_freq
        self.n_dm, self._bf = d.shape[0], bf
        check(self._lib.bf_vhist_create(bf._h, _ptr(d), d.shape[0], int(history_units), C.byref(self._c)))

    def push(self, d_packed, n_units: int, stream: int = 0) -> None:
        """bf_vhist_push: ``n_units`` units at ``d_packed`` (device) take the next unit positions, asynchronously on ``stream``."""
        check(self._lib.bf_vhist_push(self._c, _ptr(d_packed), int(n_units), C.c_void_p(stream)))

    def push_block(self, stream_idx: int, slot: int, first_unit: int, n_units: int) -> None:
        """bf_vhist_push_block: the resident units [first_unit, first_unit + n_units) of the handle's ring slot, on compute queue stream_idx."""
        check(self._lib.bf_vhist_push_block(self._c, int(stream_idx), int(slot), int(first_unit), int(n_units)))

    def history(self):
        """bf_vhist_history: (oldest_unit, next_unit, cap_units) -- units [oldest_unit, next_unit) of the series can be cut."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.bf_vhist_history(self._c, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    @staticmethod
    def _requests(requests):
        import numpy as np

        reqs = np.zeros(len(requests), vcut_request_dtype())
        if len(requests):
            r = np.asarray(requests)
            if r.dtype.names:
                for k in ("t0", "dm"):
                    reqs[k] = r[k]
            else:
                reqs["t0"], reqs["dm"] = [[int(q[k]) for q in requests] for k in range(2)]
        return reqs

    def cut(self, requests, n_units_out: int, d_out, stream: int = 0):
        """bf_vhist_cut: dedispersed units [request][n_units_out][freq][S][n_pol][ant] (packed bytes, device memory ``d_out``) of the
        requests -- an iterable of (t0 in samples, row of the delay table), or a structured array with fields t0, dm -- asynchronously
        on ``stream``.  Returns the int32 status of every request: 0 cut, 1 too old, 2 not pushed yet (its cells stay untouched)."""
        import numpy as np

        reqs = self._requests(requests)
        status = np.full(len(reqs), -1, np.int32)
        check(self._lib.bf_vhist_cut(self._c, _ptr(reqs), len(reqs), int(n_units_out), _ptr(d_out), _ptr(status), C.c_void_p(stream)))
        return status

    def cut_host(self, requests, n_units_out: int, host_out):
        """bf_vhist_cut_host: the same cut on a queue of the stage's own, copied to ``host_out`` (host memory, pinned for an asynchronous
        copy) and waited for there.  Returns the status array."""
        import numpy as np

        reqs = self._requests(requests)
        status = np.full(len(reqs), -1, np.int32)
        check(self._lib.bf_vhist_cut_host(self._c, _ptr(reqs), len(reqs), int(n_units_out), _ptr(host_out), _ptr(status)))
        return status


def event_dtype():
    """numpy mirror of ``bf_evt_event``: best (a candidate record), t_lo, t_hi, dm_lo, dm_hi, n_members, n_beams, snr_ib, flags."""
    import numpy as np

    dt = np.dtype([("best", _candidate_dtype()), ("t_lo", np.uint64), ("t_hi", np.uint64), ("dm_lo", np.int32), ("dm_hi", np.int32),
                   ("n_members", np.int32), ("n_beams", np.int32), ("snr_ib", np.float64), ("flags", np.uint32)], align=True)
    assert dt.itemsize == C.sizeof(BfEvtEvent)
    return dt


EVT_IB_ONLY, EVT_WIDE, EVT_INCOHERENT = 1, 2, 4


class EventBuilder(_Owner):
    """bf_evt: the search's candidates grouped into events (include/dsabf.h, docs/EVENTS.md) -- friends of friends in time and
    trial, streaming, on the host.  Options as in ``bf_evt_options``: t_tol, dm_tol, max_width, max_beams, ib_beam, ib_ratio."""
    _ptr_attr, _destroy = "_e", "bf_evt_destroy"

    def __init__(self, **options):
        self._lib = load()
        self._e = C.c_void_p()
        opt = BfEvtOptions()
        self._lib.bf_evt_default_options(C.byref(opt))
        for k, v in options.items():
            if k not in dict(BfEvtOptions._fields_):
                raise TypeError("EventBuilder: unknown option %r" % k)
            setattr(opt, k, v)
        self.options = opt
        check(self._lib.bf_evt_create(C.byref(opt), C.byref(self._e)))

    @property
    def open(self) -> int:
        return self._lib.bf_evt_open(self._e)

    def _events(self, call, n_new: int):
        import numpy as np

        out = np.zeros(self.open + n_new, event_dtype())
        n_out = C.c_size_t()
        check(call(_ptr(out), out.size, C.byref(n_out)))
        return out[:n_out.value].copy()

    def feed(self, cands, next_t: int):
        """The candidates of one collected push (a structured array as SinglePulseSearch.collect returns) and that push's
        first_t + n_t; returns the events that close, a structured array of ``event_dtype()``."""
        import numpy as np

        c = np.ascontiguousarray(cands, _candidate_dtype())
        return self._events(lambda out, n, n_out: self._lib.bf_evt_feed(self._e, _ptr(c), c.size, next_t, out, n, n_out), c.size)

    def flush(self):
        """Closes every open cluster and returns the events."""
        return self._events(lambda out, n, n_out: self._lib.bf_evt_flush(self._e, out, n, n_out), 0)


def _candidate_dtype():
    import numpy as np

    return np.dtype([("t_start", np.uint64), ("dm", np.int32), ("beam", np.int32), ("width", np.int32), ("peak", np.float32),
                     ("snr", np.float64)], align=True)


def sps_select(peaks, totals, n: int, n_beams: int, first_t: int = 0, dm_first: int = 0, min_samples: int = 64, threshold: float = 8.0):
    """bf_sps_select, the candidate selection as a pure host function (no GPU).  peaks: a pair (value [K][n_dm][n_beams] float32,
    t_end int32) or a structured array of bf_sps_peak; totals: (sum, sumsq) [n_dm][n_beams] float64 over the baseline window of
    ``n`` samples.  Returns the candidates as a numpy structured array."""
    import numpy as np

    if isinstance(peaks, tuple):
        value, t_end = peaks
        pk = np.empty(np.shape(value), np.dtype([("value", np.float32), ("t_end", np.int32)]))
        pk["value"], pk["t_end"] = value, t_end
    else:
        pk = np.ascontiguousarray(peaks)
    n_widths, n_dm = pk.shape[0], pk.shape[1]
    assert pk.shape == (n_widths, n_dm, n_beams) and pk.dtype.itemsize == C.sizeof(BfSpsPeak)
    tot = np.empty((n_dm, n_beams), np.dtype([("sum", np.float64), ("sumsq", np.float64)]))
    tot["sum"], tot["sumsq"] = totals
    out = np.zeros(n_dm * n_beams, _candidate_dtype())
    assert out.dtype.itemsize == C.sizeof(BfSpsCandidate)
    n_out = C.c_size_t()
    check(load().bf_sps_select(_ptr(pk), _ptr(tot), n, n_widths, n_dm, n_beams, first_t, dm_first, min_samples, threshold, _ptr(out),
                               out.size, C.byref(n_out)))
    return out[:n_out.value].copy()


class SinglePulseSearch(_Owner):
    """bf_sps: boxcar single-pulse search over the chunks [n_dm][n_t][beam] of a DmStream, on the device (include/dsabf.h,
    docs/SINGLE_PULSE.md).  Attach it with ``DmStream.attach_search`` or push chunks yourself."""
    _ptr_attr, _destroy = "_s", "bf_sps_destroy"

    def __init__(self, bf: Beamformer, n_dm: int, n_widths: int, max_t_per_push: int, dm_first: int = 0, max_in_flight: int = 4,
                 baseline_pushes: int = 8, min_samples: int = 64, threshold: float = 8.0):
        self._lib = load()
        self._s = C.c_void_p()
        self.n_dm, self.n_widths, self.n_beams, self._bf = n_dm, n_widths, bf.cfg.n_beams, bf
        check(self._lib.bf_sps_create(bf._h, n_dm, dm_first, n_widths, max_t_per_push, max_in_flight, baseline_pushes, min_samples,
                                      threshold, C.byref(self._s)))

    def push(self, d_chunk, n_t: int, first_t: int, stream: int = 0) -> None:
        check(self._lib.bf_sps_push(self._s, _ptr(d_chunk), n_t, first_t, C.c_void_p(stream)))

    @property
    def pending(self) -> int:
        return self._lib.bf_sps_pending(self._s)

    def collect(self):
        """Waits for the oldest uncollected push and returns its candidates (numpy structured array: t_start, dm, beam, width,
        peak, snr)."""
        import numpy as np

        out = np.zeros(self.n_dm * self.n_beams, _candidate_dtype())
        n_out = C.c_size_t()
        check(self._lib.bf_sps_collect(self._s, _ptr(out), out.size, C.byref(n_out)))
        return out[:n_out.value].copy()

    def last_records(self) -> dict:
        """The raw records of the push just collected (copies): value / t_end [K][n_dm][n_beams], sum / sumsq [n_dm][n_beams],
        first_t, n_t."""
        import numpy as np

        pk, st, first, n_t = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_int()
        check(self._lib.bf_sps_last_records(self._s, C.byref(pk), C.byref(st), C.byref(first), C.byref(n_t)))
        n_db = self.n_dm * self.n_beams
        peaks = np.ctypeslib.as_array(C.cast(pk, C.POINTER(BfSpsPeak)), (self.n_widths * n_db,)).reshape(self.n_widths, self.n_dm, self.n_beams)
        stats = np.ctypeslib.as_array(C.cast(st, C.POINTER(BfSpsStat)), (n_db,)).reshape(self.n_dm, self.n_beams)
        return {"value": peaks["value"].copy(), "t_end": peaks["t_end"].copy(), "sum": stats["sum"].copy(), "sumsq": stats["sumsq"].copy(),
                "first_t": int(first.value), "n_t": int(n_t.value)}


def _ffa_candidate_dtype():
    import numpy as np

    return np.dtype([("first_row", np.uint64), ("n_rows", np.uint64), ("period_rows", np.float64), ("dm", np.int32), ("beam", np.int32),
                     ("octave", np.int32), ("p", np.int32), ("shift", np.int32), ("bin", np.int32), ("width", np.int32), ("snr", np.float64),
                     ("value", np.float32)], align=True)


def _ffa_group_dtype():
    import numpy as np

    return np.dtype([("head", _ffa_candidate_dtype()), ("n_members", np.int32), ("n_beams", np.int32), ("dm_lo", np.int32), ("dm_hi", np.int32),
                     ("n_harmonic", np.int32), ("reserved", np.int32)], align=True)


class PeriodicitySearch(_Owner):
    """bf_ffa: a blind periodicity search (Fast Folding Algorithm) over the chunks [n_dm][n_t][beam] of a DmStream, on the device
    (include/dsabf.h, docs/PERIODICITY.md): the series of every (trial, beam) decimated by ``tdec``, cut into segments of ``n_seg``
    samples, folded at every base period p_lo <= p < p_hi of ``n_oct`` octaves, boxcar-filtered at ``n_widths`` widths.  Attach it
    with ``DmStream.attach_periodicity`` or push chunks yourself.  ``detrend=(blk, win)`` (bf_ffa_set_detrend) removes a running
    median over ``win`` means of ``blk`` decimated samples from every segment in front of the fold; None leaves it off."""
    _ptr_attr, _destroy = "_s", "bf_ffa_destroy"

    def __init__(self, bf: Beamformer, n_dm: int, tdec: int, n_seg: int, n_oct: int, p_lo: int, p_hi: int, n_widths: int, max_t_per_push: int,
                 dm_first: int = 0, max_in_flight: int = 2, threshold: float = 8.0, detrend: "tuple[int, int] | None" = None):
        self._lib = load()
        self._s = C.c_void_p()
        self.n_dm, self.n_beams, self._bf = n_dm, bf.cfg.n_beams, bf
        self.tdec, self.n_seg, self.n_oct, self.p_lo, self.p_hi, self.n_widths, self.dm_first = tdec, n_seg, n_oct, p_lo, p_hi, n_widths, dm_first
        check(self._lib.bf_ffa_create(bf._h, n_dm, dm_first, tdec, n_seg, n_oct, p_lo, p_hi, n_widths, max_t_per_push, max_in_flight, threshold,
                                      C.byref(self._s)))
        if detrend is not None:
            try:
                self.set_detrend(*detrend)
            except Exception:
                self.close()
                raise

    def set_detrend(self, blk: int, win: int) -> None:
        """bf_ffa_set_detrend: before the first push only; blk 0 switches the detrend off."""
        check(self._lib.bf_ffa_set_detrend(self._s, int(blk), int(win)))

    @property
    def detrend(self):
        """bf_ffa_detrend: (blk, win), or None while the detrend is off."""
        blk, win = C.c_int(), C.c_int()
        check(self._lib.bf_ffa_detrend(self._s, C.byref(blk), C.byref(win)))
        return (blk.value, win.value) if blk.value else None

    @staticmethod
    def sift(cands, tol: float = 0.002, max_harm: int = 4, dm_tol: int = 2):
        """bf_ffa_sift, the harmonic sift as a pure host function (no GPU): ``cands`` a candidate array as ``collect`` returns it (of
        any number of segments, concatenated).  Returns a numpy structured array of groups (head, n_members, n_beams, dm_lo, dm_hi,
        n_harmonic), in the order the groups were created."""
        import numpy as np

        cands = np.ascontiguousarray(cands, _ffa_candidate_dtype())
        out = np.zeros(max(len(cands), 1), _ffa_group_dtype())
        assert out.dtype.itemsize == C.sizeof(BfFfaGroup)
        n_out = C.c_size_t()
        check(load().bf_ffa_sift(_ptr(cands) if len(cands) else None, len(cands), tol, max_harm, dm_tol, _ptr(out), len(cands), C.byref(n_out)))
        return out[:n_out.value].copy()

    @staticmethod
    def rows_of(length: int, p: int) -> int:
        """bf_ffa_rows_of: the rows M of the fold of ``length`` samples at base period p (host, no GPU)."""
        return load().bf_ffa_rows_of(int(length), int(p))

    @staticmethod
    def select(peaks, stats, tdec: int, n_seg: int, p_lo: int, first_row: int = 0, dm_first: int = 0, threshold: float = 8.0):
        """bf_ffa_select, the candidate selection as a pure host function (no GPU).  peaks: (value float32, shift, bin)
        [n_oct][n_p][K][n_dm][n_beams]; stats: (sum, sumsq) [n_dm][n_beams] float64 of the segment.  Returns a numpy structured array."""
        import numpy as np

        value, shift, bin_ = peaks
        n_oct, n_p, n_widths, n_dm, n_beams = np.shape(value)
        pk = np.empty(np.shape(value), np.dtype([("value", np.float32), ("shift", np.uint16), ("bin", np.uint16)]))
        pk["value"], pk["shift"], pk["bin"] = value, shift, bin_
        st = np.empty((n_dm, n_beams), np.dtype([("sum", np.float64), ("sumsq", np.float64)]))
        st["sum"], st["sumsq"] = stats
        assert pk.dtype.itemsize == C.sizeof(BfFfaPeak) and st.dtype.itemsize == C.sizeof(BfFfaStat)
        out = np.zeros(n_dm * n_beams, _ffa_candidate_dtype())
        assert out.dtype.itemsize == C.sizeof(BfFfaCandidate)
        n_out = C.c_size_t()
        check(load().bf_ffa_select(_ptr(pk), _ptr(st), tdec, n_seg, n_oct, p_lo, p_lo + n_p, n_widths, n_dm, n_beams, first_row, n_seg * tdec,
                                   dm_first, threshold, _ptr(out), out.size, C.byref(n_out)))
        return out[:n_out.value].copy()

    def push(self, d_chunk, n_t: int, first_t: int, stream: int = 0) -> None:
        check(self._lib.bf_ffa_push(self._s, _ptr(d_chunk), n_t, first_t, C.c_void_p(stream)))

    @property
    def pending(self) -> int:
        return self._lib.bf_ffa_pending(self._s)

    def collect(self):
        """Waits for the oldest uncollected segment and returns its candidates (numpy structured array, one per (trial, beam) at most)."""
        import numpy as np

        out = np.zeros(self.n_dm * self.n_beams, _ffa_candidate_dtype())
        n_out = C.c_size_t()
        check(self._lib.bf_ffa_collect(self._s, _ptr(out), out.size, C.byref(n_out)))
        return out[:n_out.value].copy()

    def last_records(self) -> dict:
        """The raw records of the segment just collected (copies): value / shift / bin [n_oct][n_p][K][n_dm][n_beams], sum / sumsq
        [n_dm][n_beams], first_row, n_rows."""
        import numpy as np

        pk, st, first, n_rows = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(self._lib.bf_ffa_last_records(self._s, C.byref(pk), C.byref(st), C.byref(first), C.byref(n_rows)))
        n_db = self.n_dm * self.n_beams
        shape = (self.n_oct, self.p_hi - self.p_lo, self.n_widths, self.n_dm, self.n_beams)
        peaks = np.ctypeslib.as_array(C.cast(pk, C.POINTER(BfFfaPeak)), (int(np.prod(shape)),)).reshape(shape)
        stats = np.ctypeslib.as_array(C.cast(st, C.POINTER(BfFfaStat)), (n_db,)).reshape(self.n_dm, self.n_beams)
        return {"value": peaks["value"].copy(), "shift": peaks["shift"].copy(), "bin": peaks["bin"].copy(), "sum": stats["sum"].copy(),
                "sumsq": stats["sumsq"].copy(), "first_row": int(first.value), "n_rows": int(n_rows.value)}


class Conditioner(_Owner):
    """bf_cond: the detected rows [t][f][b] rewritten in place on the device -- normalised per (channel, beam) against the last
    ``baseline_pushes`` pushes, bad channels masked, the per-(time, beam) mean over the channels removed (include/dsabf.h,
    docs/CONDITIONING.md).  Attach it with ``DmStream.attach_conditioner`` or push rows yourself."""
    _ptr_attr, _destroy = "_c", "bf_cond_destroy"

    def __init__(self, bf: Beamformer, n_freq_total: int, max_rows: int, baseline_pushes: int = 8, zero_dm: bool = True,
                 auto_threshold: float = 0.0, mask=None):
        self._lib = load()
        self._c = C.c_void_p()
        self.n_freq_total, self.n_beams, self._bf = n_freq_total, bf.cfg.n_beams, bf
        opt = BfCondOptions(baseline_pushes, int(bool(zero_dm)), auto_threshold)
        check(self._lib.bf_cond_create(bf._h, n_freq_total, max_rows, C.byref(opt), C.byref(self._c)))
        if mask is not None:
            self.set_mask(mask)

    def push(self, d_rows, n_rows: int, stream: int = 0) -> None:
        check(self._lib.bf_cond_push(self._c, _ptr(d_rows), n_rows, C.c_void_p(stream)))

    def set_mask(self, mask) -> None:
        """The static mask (nonzero = masked), one entry per channel: holds from the next push on."""
        import numpy as np

        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        assert m.shape == (self.n_freq_total,)
        check(self._lib.bf_cond_set_mask(self._c, _ptr(m)))

    def mask(self):
        """mask[f] of the most recent push (uint8 host copy, after a device synchronisation)."""
        import numpy as np

        from ._lib import _preload_hip_runtime

        p = C.c_void_p()
        check(self._lib.bf_cond_mask_device(self._c, C.byref(p)))
        out = np.zeros(self.n_freq_total, np.uint8)
        hip = _preload_hip_runtime()
        if hip.hipDeviceSynchronize() != 0 or hip.hipMemcpy(_ptr(out), p, C.c_size_t(out.size), 2) != 0:
            raise DsabfError(-3, "Conditioner.mask: the copy from the device failed")
        return out


class PulsarFolder(_Owner):
    """bf_psr: the detected rows [t][f][b] folded at known spin models into fp64 profiles [pulsar][freq][bin][beam] and uint64 hits
    [pulsar][freq][bin], every cell summed in row order (include/dsabf.h, docs/PULSAR_FOLDING.md).  ``models``: BfPsrModel objects or
    (phase0, dphase, ddphase, epoch_row) tuples; ``delays``: int32 host array [n_psr][n_freq_total].  Attach it with
    ``DmStream.attach_folder`` or push rows yourself."""
    _ptr_attr, _destroy = "_c", "bf_psr_destroy"

    def __init__(self, bf: Beamformer, n_freq_total: int, max_rows: int, n_bins: int, models, delays, max_in_flight: int = 2):
        import numpy as np

        self._lib = load()
        self._c = C.c_void_p()
        self._bf = bf
        ms = (BfPsrModel * max(len(models), 1))()
        for i, m in enumerate(models):
            ms[i] = m if isinstance(m, BfPsrModel) else BfPsrModel(*[int(v) for v in m])
        d = np.ascontiguousarray(delays, np.int32)
        assert d.ndim == 2 and d.shape == (len(models), n_freq_total)
        self.n_psr, self.n_freq_total, self.n_bins, self.n_beams = len(models), n_freq_total, n_bins, bf.cfg.n_beams
        check(self._lib.bf_psr_create(bf._h, n_freq_total, max_rows, n_bins, C.cast(ms, C.c_void_p), _ptr(d), len(models), int(max_in_flight),
                                      C.byref(self._c)))

    @staticmethod
    def model_from_spin(f0_hz: float, f1_hz_s: float = 0.0, phase0_turns: float = 0.0, row_seconds: float = 1.0, epoch_row: int = 0) -> BfPsrModel:
        """bf_psr_model_from_spin: the fixed-point oscillator of a spin frequency and its derivative (host, no GPU)."""
        m = BfPsrModel()
        check(load().bf_psr_model_from_spin(f0_hz, f1_hz_s, phase0_turns, row_seconds, int(epoch_row), C.byref(m)))
        return m

    @staticmethod
    def beam_snr(profile_k, hits_k, chan_mask=None):
        """bf_psr_beam_snr: (snr float64 [n_beams], peak_bin int32 [n_beams]) of one pulsar's profile [f][bin][beam] and hits [f][bin]
        (host, no GPU); chan_mask: nonzero = channel left out."""
        import numpy as np

        p = np.ascontiguousarray(profile_k, np.float64)
        h = np.ascontiguousarray(hits_k, np.uint64)
        assert p.ndim == 3 and h.shape == p.shape[:2]
        m = None if chan_mask is None else np.ascontiguousarray(np.asarray(chan_mask) != 0, np.uint8)
        assert m is None or m.shape == (p.shape[0],)
        snr, peak = np.zeros(p.shape[2], np.float64), np.zeros(p.shape[2], np.int32)
        check(load().bf_psr_beam_snr(_ptr(p), _ptr(h), p.shape[0], p.shape[1], p.shape[2], _ptr(m), _ptr(snr), _ptr(peak)))
        return snr, peak

    def push(self, d_rows, n_rows: int, stream: int = 0) -> None:
        check(self._lib.bf_psr_push(self._c, _ptr(d_rows), int(n_rows), C.c_void_p(stream)))

    def dump(self, stream: int = 0) -> None:
        """Snapshot profile and hits to pinned host memory, then zero them (BF_ERR_STATE beyond max_in_flight uncollected dumps)."""
        check(self._lib.bf_psr_dump(self._c, C.c_void_p(stream)))

    @property
    def pending(self) -> int:
        return self._lib.bf_psr_pending(self._c)

    def collect(self):
        """Waits for the oldest uncollected dump; returns (profile float64 [n_psr][freq][bin][beam], hits uint64 [n_psr][freq][bin],
        first_row, n_rows) of that integration."""
        import numpy as np

        prof = np.empty((self.n_psr, self.n_freq_total, self.n_bins, self.n_beams), np.float64)
        hits = np.empty((self.n_psr, self.n_freq_total, self.n_bins), np.uint64)
        first, n = C.c_uint64(), C.c_uint64()
        check(self._lib.bf_psr_collect(self._c, _ptr(prof), _ptr(hits), C.byref(first), C.byref(n)))
        return prof, hits, int(first.value), int(n.value)


def _truth_dtype():
    import numpy as np

    return np.dtype([("t_lo", np.uint64), ("t_hi", np.uint64), ("trial", np.int32), ("beam", np.int32)], align=True)


class Injector(_Owner):
    """bf_inj: synthetic bursts and pulse trains added in place to the detected rows [t][f][b], bit-equal to
    tests/support/inj_oracle.py (include/dsabf.h, docs/INJECTION.md).  Tables are host arrays: ``delay`` int32 [n_freq_total],
    ``profile`` float32 [n_freq_total][W or n_bins], ``response`` float32 [n_beams].  Attach it with ``DmStream.attach_injector`` or
    apply it to rows yourself."""
    _ptr_attr, _destroy = "_c", "bf_inj_destroy"

    def __init__(self, bf: Beamformer, n_freq_total: int, max_rows: int, max_pulses: int = 64, max_width: int = 256):
        self._lib = load()
        self._c = C.c_void_p()
        self.n_freq_total, self.n_beams, self._bf = n_freq_total, bf.cfg.n_beams, bf
        check(self._lib.bf_inj_create(bf._h, n_freq_total, max_rows, max_pulses, max_width, C.byref(self._c)))

    def _tables(self, width: int, delay, profile, response):
        import numpy as np

        d = np.ascontiguousarray(delay, np.int32)
        p = np.ascontiguousarray(profile, np.float32)
        r = np.ascontiguousarray(response, np.float32)
        assert d.shape == (self.n_freq_total,) and p.shape == (self.n_freq_total, width) and r.shape == (self.n_beams,)
        return d, p, r

    def add_burst(self, t0: int, delay, profile, response) -> int:
        """bf_inj_add_burst (W = profile.shape[1]); returns the pulse's id."""
        import numpy as np

        W = int(np.shape(profile)[1])
        d, p, r = self._tables(W, delay, profile, response)
        pid = C.c_uint64()
        check(self._lib.bf_inj_add_burst(self._c, int(t0), W, _ptr(d), _ptr(p), _ptr(r), C.byref(pid)))
        return int(pid.value)

    def add_train(self, model, delay, profile, response, first_row: int = 0, n_rows: int | None = None) -> int:
        """bf_inj_add_train (n_bins = profile.shape[1]; n_rows None: until the end); ``model``: a BfPsrModel or a (phase0, dphase,
        ddphase, epoch_row) tuple.  Returns the pulse's id."""
        import numpy as np

        n_bins = int(np.shape(profile)[1])
        d, p, r = self._tables(n_bins, delay, profile, response)
        m = model if isinstance(model, BfPsrModel) else BfPsrModel(*[int(v) for v in model])
        pid = C.c_uint64()
        check(self._lib.bf_inj_add_train(self._c, C.byref(m), int(first_row), (1 << 64) - 1 if n_rows is None else int(n_rows), n_bins, _ptr(d),
                                         _ptr(p), _ptr(r), C.byref(pid)))
        return int(pid.value)

    def apply(self, d_rows, n_rows: int, stream: int = 0) -> None:
        check(self._lib.bf_inj_apply(self._c, _ptr(d_rows), int(n_rows), C.c_void_p(stream)))

    @property
    def next_row(self) -> int:
        return int(self._lib.bf_inj_next_row(self._c))

    @property
    def launches(self) -> int:
        return int(self._lib.bf_inj_launches(self._c))

    @staticmethod
    def burst_profile(n_freq_total: int, W: int, centre: float, sigma: float, fluence, smear=None):
        """bf_inj_burst_profile: float32 [n_freq_total][W], a Gaussian of ``sigma`` rows around ``centre``, box-smeared over smear[f] rows,
        each channel summing to fluence[f] (a scalar: every channel) (host, no GPU)."""
        import numpy as np

        fl = np.ascontiguousarray(np.broadcast_to(np.asarray(fluence, np.float64), (n_freq_total,)))
        sm = None if smear is None else np.ascontiguousarray(np.broadcast_to(np.asarray(smear, np.int32), (n_freq_total,)))
        out = np.zeros((n_freq_total, W), np.float32)
        check(load().bf_inj_burst_profile(n_freq_total, W, float(centre), float(sigma), _ptr(sm), _ptr(fl), _ptr(out)))
        return out

    @staticmethod
    def nearest_trial(ladder, delay) -> int:
        """bf_inj_nearest_trial: the trial of ``ladder`` int32 [n_dm][n_freq_total] closest to ``delay`` in summed |difference| (host, no GPU)."""
        import numpy as np

        lad = np.ascontiguousarray(ladder, np.int32)
        d = np.ascontiguousarray(delay, np.int32)
        assert lad.ndim == 2 and d.shape == (lad.shape[1],)
        trial = C.c_int(-1)
        check(load().bf_inj_nearest_trial(_ptr(lad), lad.shape[0], lad.shape[1], _ptr(d), C.byref(trial)))
        return int(trial.value)

    @staticmethod
    def match(truth, cands, t_tol: int = 0, dm_tol: int = 0):
        """bf_inj_match: int32 [len(truth)], per truth record (t_lo, t_hi, trial, beam) the index of the matching candidate with the
        largest snr, -1 if none (host, no GPU).  ``cands``: a structured array as ``SinglePulseSearch.collect`` returns."""
        import numpy as np

        tr = np.zeros(len(truth), _truth_dtype())
        for i, t in enumerate(truth):
            tr[i] = tuple(int(v) for v in t)
        cd = np.ascontiguousarray(cands, _candidate_dtype())
        assert tr.dtype.itemsize == C.sizeof(BfInjTruth) and cd.dtype.itemsize == C.sizeof(BfSpsCandidate)
        best = np.full(len(tr), -1, np.int32)
        check(load().bf_inj_match(_ptr(tr), len(tr), _ptr(cd), len(cd), int(t_tol), int(dm_tol), _ptr(best)))
        return best


class _AccumStage(_Owner):
    """What ``Correlator`` and ``SpectralKurtosis`` share: the bf_<_abi>_* entry points of an accumulator stage, whose results have
    the shape ``_shape(cfg)``."""
    _ptr_attr = "_c"
    _abi = None

    def __init__(self, bf: Beamformer, max_in_flight: int = 2):
        self._lib = load()
        self._c = C.c_void_p()
        self._bf = bf
        self.shape = self._shape(bf.cfg)
        check(self._call("create")(bf._h, int(max_in_flight), C.byref(self._c)))

    def _call(self, name: str):
        return getattr(self._lib, "bf_%s_%s" % (self._abi, name))

    def push(self, d_packed, n_units: int, stream: int = 0) -> None:
        check(self._call("push")(self._c, _ptr(d_packed), int(n_units), C.c_void_p(stream)))

    def push_block(self, stream_idx: int, slot: int, first_unit: int, n_units: int) -> None:
        """The gemm-units [first_unit, first_unit + n_units) of ring slot ``slot`` (what enqueue_block reads), on compute queue stream_idx."""
        check(self._call("push_block")(self._c, int(stream_idx), int(slot), int(first_unit), int(n_units)))

    def dump(self, stream: int = 0) -> None:
        """Snapshot the accumulator to pinned host memory, then zero it (BF_ERR_STATE beyond max_in_flight uncollected dumps)."""
        check(self._call("dump")(self._c, C.c_void_p(stream)))

    @property
    def pending(self) -> int:
        return self._call("pending")(self._c)

    def collect(self):
        import numpy as np

        out = np.empty(self.shape, np.int64)
        n = C.c_uint64()
        check(self._call("collect")(self._c, _ptr(out), C.byref(n)))
        return out, int(n.value)


class Correlator(_AccumStage):
    """bf_corr: the correlator as a stage (include/dsabf.h, docs/CORRELATOR.md): one int64 accumulator on the device that pushes add
    to and a dump snapshots and zeroes; the stage orders its pushes and dumps itself, whatever queues they are issued on."""
    _abi, _destroy = "corr", "bf_corr_destroy"

    @staticmethod
    def _shape(cfg):
        return (cfg.n_freq, cfg.n_pol, cfg.n_ant * (cfg.n_ant + 1) // 2, 2)

    def collect(self):
        """Waits for the oldest uncollected dump; returns (int64 array [freq][pol][baseline][2], columns per polarisation)."""
        return super().collect()


class SpectralKurtosis(_AccumStage):
    """bf_sk: the voltage moments as a stage (include/dsabf.h, docs/SPECTRAL_KURTOSIS.md), a twin of ``Correlator``: one int64
    accumulator on the device that pushes add to and a dump snapshots and zeroes; the stage orders its pushes and dumps itself."""
    _abi, _destroy = "sk", "bf_sk_destroy"

    @staticmethod
    def _shape(cfg):
        return (cfg.n_freq, cfg.n_pol, cfg.n_ant, 2)

    def collect(self):
        """Waits for the oldest uncollected dump; returns (int64 array [freq][pol][ant][2] = {m1, m2}, columns per polarisation)."""
        return super().collect()


class StokesBeams(_Owner):
    """bf_stokes: full-Stokes follow-up beams as a stage (include/dsabf.h, docs/STOKES.md).  For up to 16 beams picked from a weight
    array in the layout of ``set_weights`` it forms I, Q, U, V as exact int64 over windows of ``n_int`` samples (None: n_avg, the
    detected stream's resolution; 1: the voltages' own) from the packed voltages the beamformer reads."""
    _ptr_attr, _destroy = "_c", "bf_stokes_destroy"

    def __init__(self, bf: Beamformer, n_int: int | None = None, max_in_flight: int = 2):
        self._lib = load()
        self._c = C.c_void_p()
        self._bf = bf
        self.cfg = bf.cfg
        self.n_int = int(bf.cfg.n_avg if n_int is None else n_int)
        self.n_sel = 0
        self._pushed = []   # beams selected at each uncollected push, oldest first
        check(self._lib.bf_stokes_create(bf._h, self.n_int, int(max_in_flight), C.byref(self._c)))

    def set_weights(self, w, beams, stream: int = 0) -> None:
        """w: int8 [freq][ant][beam][2] as a host numpy array (bf_stokes_set_weights, returns when the copy has run) or a device tensor
        (bf_stokes_set_weights_device, asynchronous on ``stream``); beams: the indices to follow, in the order of the output."""
        sel = [int(b) for b in beams]
        arr = (C.c_int * max(len(sel), 1))(*sel)
        if hasattr(w, "data_ptr") and getattr(w, "is_cuda", False):
            check(self._lib.bf_stokes_set_weights_device(self._c, _ptr(w), arr, len(sel), C.c_void_p(stream)))
        else:
            check(self._lib.bf_stokes_set_weights(self._c, _ptr(w), arr, len(sel)))
        self.n_sel = len(sel)

    @property
    def entries(self) -> int:
        """bf_stokes_entries at the beams now selected: T * n_freq * K cells (four int64 each) per gemm-unit; 0 before set_weights."""
        return self._lib.bf_stokes_entries(C.byref(self.cfg), self.n_sel, self.n_int)

    def compute(self, d_packed, n_units: int, d_out, stream: int = 0) -> None:
        """bf_stokes_device: the kernel alone into d_out (device int64, n_units * entries * 4), asynchronously on ``stream``."""
        check(self._lib.bf_stokes_device(self._c, _ptr(d_packed), int(n_units), _ptr(d_out), C.c_void_p(stream)))

    def voltages(self, d_packed, n_units: int, d_out, stream: int = 0) -> None:
        """bf_stokes_voltages_device: the beam samples themselves into d_out (device complex64 [freq][k][pol][n_units * S], the exact
        integers as float32), asynchronously on ``stream`` and ordered as ``compute`` is (docs/COHERENT_DEDISPERSION.md section 1)."""
        check(self._lib.bf_stokes_voltages_device(self._c, _ptr(d_packed), int(n_units), _ptr(d_out), C.c_void_p(stream)))

    def push(self, d_packed, n_units: int, stream: int = 0) -> None:
        check(self._lib.bf_stokes_push(self._c, _ptr(d_packed), int(n_units), C.c_void_p(stream)))
        self._pushed.append(self.n_sel)

    def push_block(self, stream_idx: int, slot: int, first_unit: int, n_units: int) -> None:
        """The gemm-units [first_unit, first_unit + n_units) of ring slot ``slot`` (what enqueue_block reads), on compute queue stream_idx."""
        check(self._lib.bf_stokes_push_block(self._c, int(stream_idx), int(slot), int(first_unit), int(n_units)))
        self._pushed.append(self.n_sel)

    @property
    def pending(self) -> int:
        return self._lib.bf_stokes_pending(self._c)

    def collect(self):
        """Waits for the oldest uncollected push; returns its int64 array [unit][t][freq][k][4] = {I, Q, U, V}."""
        import numpy as np

        if not self._pushed:
            check(self._lib.bf_stokes_collect(self._c, _ptr(np.empty(4, np.int64)), None))   # (raises BF_ERR_STATE: nothing pending)
        k = self._pushed[0]
        cfg = self.cfg
        T = cfg.n_out_per_gemm * cfg.n_avg // self.n_int
        out = np.empty((cfg.n_gemms_per_block, T, cfg.n_freq, k, 4), np.int64)
        n = C.c_int()
        check(self._lib.bf_stokes_collect(self._c, _ptr(out), C.byref(n)))
        self._pushed.pop(0)
        return out[:n.value].copy()


def _freqs(freq_ghz):
    import numpy as np

    f = np.ascontiguousarray(np.atleast_1d(freq_ghz), np.float64)
    return f, f.ctypes.data_as(C.POINTER(C.c_double))


def cdd_sweep_samples(dm: float, f_ghz: float, bw_mhz: float) -> float:
    """bf_cdd_sweep_samples: the dispersion sweep across one channel of width bw_mhz centred on f_ghz, in samples of 1 / bw_mhz us."""
    return load().bf_cdd_sweep_samples(float(dm), float(f_ghz), float(bw_mhz))


def cdd_edge(dm: float, freq_ghz, bw_mhz: float) -> int:
    """bf_cdd_edge: the largest ceil(sweep) over the channels -- the samples a segment gives up on each side."""
    f, p = _freqs(freq_ghz)
    return check(load().bf_cdd_edge(float(dm), p, len(f), float(bw_mhz)))


def cdd_chirp(dm: float, freq_ghz, bw_mhz: float, sideband: int, n_fft: int):
    """bf_cdd_chirp: the table complex64 [n_chan][n_fft] of a CoherentDedisperser (the 1 / n_fft of the inverse transform included)."""
    import numpy as np

    f, p = _freqs(freq_ghz)
    out = np.empty((len(f), max(int(n_fft), 0)), np.complex64)
    check(load().bf_cdd_chirp(float(dm), p, len(f), float(bw_mhz), int(sideband), int(n_fft), _ptr(out)))
    return out


class CoherentDedisperser(_Owner):
    """bf_cdd: coherent dedispersion of beam voltages by overlap-save FFT segments (include/dsabf.h, docs/COHERENT_DEDISPERSION.md).
    ``chirp`` is complex64 [n_chan][n_fft] (cdd_chirp, or any table); the input of ``voltages`` and ``stokes`` is a device complex64
    array [n_chan][K][2][n_time], what StokesBeams.voltages writes."""
    _ptr_attr, _destroy = "_c", "bf_cdd_destroy"

    def __init__(self, bf: Beamformer, n_chan: int, n_fft: int, n_edge: int, chirp):
        self._lib = load()
        self._c = C.c_void_p()
        self._bf = bf
        self.n_chan, self.n_fft, self.n_edge = int(n_chan), int(n_fft), int(n_edge)
        check(self._lib.bf_cdd_create(bf._h, self.n_chan, self.n_fft, self.n_edge, _ptr(self._table(chirp)), C.byref(self._c)))

    def _table(self, chirp):
        import numpy as np

        if chirp is None:
            return None
        table = np.ascontiguousarray(chirp, np.complex64)
        if self.n_chan * self.n_fft > 0 and table.size != self.n_chan * self.n_fft:   # (a shape the library refuses: left to it)
            raise ValueError("the chirp table has %d entries, not n_chan * n_fft = %d" % (table.size, self.n_chan * self.n_fft))
        return table

    @property
    def n_valid(self) -> int:
        """V = n_fft - 2 n_edge: the output samples of one segment."""
        return self.n_fft - 2 * self.n_edge

    def set_chirp(self, chirp) -> None:
        """bf_cdd_set_chirp: waits for the stage's kernels in flight, uploads, returns when the table is in place."""
        check(self._lib.bf_cdd_set_chirp(self._c, _ptr(self._table(chirp))))

    def voltages(self, d_in, K: int, n_time: int, d_out, stream: int = 0) -> None:
        """bf_cdd_voltages_device: the dedispersed series in the input's shape, asynchronously on ``stream``."""
        check(self._lib.bf_cdd_voltages_device(self._c, _ptr(d_in), int(K), int(n_time), _ptr(d_out), C.c_void_p(stream)))

    def stokes(self, d_in, K: int, n_time: int, n_int: int, d_out, stream: int = 0) -> None:
        """bf_cdd_stokes_device: float32 [n_time / n_int][n_chan][K]{I, Q, U, V}; n_int divides n_valid and n_time."""
        check(self._lib.bf_cdd_stokes_device(self._c, _ptr(d_in), int(K), int(n_time), int(n_int), _ptr(d_out), C.c_void_p(stream)))


def rm_peak_dtype():
    """bf_rm_peak: the 32-byte record FaradaySynthesis.run writes per (row, beam)."""
    import numpy as np

    dt = np.dtype([("p", np.int32), ("pow_lo", np.float32), ("pow_pk", np.float32), ("pow_hi", np.float32), ("re", np.float32),
                   ("im", np.float32), ("isum", np.float32), ("zero", np.int32)])
    assert dt.itemsize == 32
    return dt


def rm_fit_dtype():
    """bf_rm_fit: what rm_refine makes of a record."""
    import numpy as np

    return np.dtype([("rm", np.float64), ("pa", np.float64), ("lin", np.float64), ("frac", np.float64)])


def _channels(freq_ghz, w):
    import numpy as np

    f, fp = _freqs(freq_ghz)
    wt = np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if w is None else w, np.float64), f.shape))
    return f, fp, wt, wt.ctypes.data_as(C.POINTER(C.c_double))


def rm_lambda2(f_ghz: float) -> float:
    """bf_rm_lambda2: (0.299792458 / f_ghz)^2 in m^2."""
    return load().bf_rm_lambda2(float(f_ghz))


def rm_resolution(freq_ghz, w=None):
    """bf_rm_resolution: (fwhm, phi_max) in rad / m^2 of the unmasked channels (w None: all ones)."""
    f, fp, wt, wp = _channels(freq_ghz, w)
    fwhm, phi_max = C.c_double(), C.c_double()
    check(load().bf_rm_resolution(fp, wp, len(f), C.byref(fwhm), C.byref(phi_max)))
    return fwhm.value, phi_max.value


def rm_table(freq_ghz, w, phi0: float, dphi: float, n_phi: int):
    """bf_rm_table: (rot complex64 [n_phi][n_chan] = r + i s, wn float32 [n_chan], lambda0_2) of a FaradaySynthesis."""
    import numpy as np

    f, fp, wt, wp = _channels(freq_ghz, w)
    rot, wn, l0 = np.empty((max(int(n_phi), 0), len(f)), np.complex64), np.empty(len(f), np.float32), C.c_double()
    check(load().bf_rm_table(fp, wp, len(f), float(phi0), float(dphi), int(n_phi), _ptr(rot), _ptr(wn), C.byref(l0)))
    return rot, wn, l0.value


def rm_rmsf(freq_ghz, w, phi0: float, dphi: float, n_phi: int):
    """bf_rm_rmsf: the rotation measure spread function on the grid, complex128 [n_phi]."""
    import numpy as np

    f, fp, wt, wp = _channels(freq_ghz, w)
    out = np.empty(max(int(n_phi), 0), np.complex128)
    check(load().bf_rm_rmsf(fp, wp, len(f), float(phi0), float(dphi), int(n_phi), _ptr(out)))
    return out


def rm_refine(peaks, phi0: float, dphi: float, n_phi: int, lambda0_2: float):
    """bf_rm_refine: the parabola through the three powers of every record -> a structured array of rm_fit_dtype in ``peaks``'s shape."""
    import numpy as np

    pk = np.ascontiguousarray(peaks, rm_peak_dtype())
    fits = np.empty(pk.shape, rm_fit_dtype())
    check(load().bf_rm_refine(_ptr(pk), pk.size, float(phi0), float(dphi), int(n_phi), float(lambda0_2), _ptr(fits)))
    return fits


class FaradaySynthesis(_Owner):
    """bf_rm: rotation-measure synthesis of Stokes beams on the f32 matrix instructions (include/dsabf.h, docs/FARADAY.md).  ``rot`` is
    complex64 [n_phi][n_chan] and ``wn`` float32 [n_chan] (rm_table, or any table); the input of ``run`` is a device float32 array
    [n_rows][n_chan][K][4], what CoherentDedisperser.stokes writes."""
    _ptr_attr, _destroy = "_c", "bf_rm_destroy"

    def __init__(self, bf: Beamformer, n_chan: int, n_phi: int, rot, wn):
        self._lib = load()
        self._c = C.c_void_p()
        self._bf = bf
        self.n_chan, self.n_phi = int(n_chan), int(n_phi)
        r, n = self._tables(rot, wn)
        check(self._lib.bf_rm_create(bf._h, self.n_chan, self.n_phi, _ptr(r), _ptr(n), C.byref(self._c)))

    def _tables(self, rot, wn):
        import numpy as np

        r = None if rot is None else np.ascontiguousarray(rot, np.complex64)
        n = None if wn is None else np.ascontiguousarray(wn, np.float32)
        if self.n_chan * self.n_phi > 0:   # (a shape the library refuses: left to it)
            if r is not None and r.size != self.n_chan * self.n_phi:
                raise ValueError("the table has %d entries, not n_phi * n_chan = %d" % (r.size, self.n_chan * self.n_phi))
            if n is not None and n.size != self.n_chan:
                raise ValueError("wn has %d entries, not n_chan = %d" % (n.size, self.n_chan))
        return r, n

    def set_table(self, rot, wn) -> None:
        """bf_rm_set_table: waits for the stage's kernels in flight, uploads, returns when the table is in place."""
        r, n = self._tables(rot, wn)
        check(self._lib.bf_rm_set_table(self._c, _ptr(r), _ptr(n)))

    def run(self, d_stokes, K: int, n_rows: int, base=None, spec=None, peaks=None, stream: int = 0) -> None:
        """bf_rm_device: spec complex64 [n_rows][K][n_phi] and / or peaks [n_rows][K] records of rm_peak_dtype (32 bytes each), device
        arrays, asynchronously on ``stream``; base: an optional device float32 [n_chan][K][4] subtracted from every row."""
        check(self._lib.bf_rm_device(self._c, _ptr(d_stokes), int(K), int(n_rows), _ptr(base), _ptr(spec), _ptr(peaks), C.c_void_p(stream)))


def sk_select(moments, M: int, centre: float | None = None, n_sigma: float | None = None, max_bad_fraction_ant: float | None = None,
              max_bad_fraction_chan: float | None = None):
    """bf_sk_select (host only): moments int64 [freq][pol][ant][2] over ``M`` columns per polarisation -> (sk float64 [freq][pol][ant],
    cell uint8 [freq][pol][ant], ant_flags uint8 [ant], chan_flags uint8 [freq]).  Options left None keep bf_sk_default_options."""
    import numpy as np

    lib = load()
    mom = np.ascontiguousarray(moments, np.int64)
    if mom.ndim != 4 or mom.shape[3] != 2:
        raise ValueError("moments must be [freq][pol][ant][2], not %r" % (mom.shape,))
    n_freq, n_pol, n_ant = mom.shape[:3]
    opt = BfSkOptions()
    check(lib.bf_sk_default_options(C.byref(opt)))
    for name, v in (("centre", centre), ("n_sigma", n_sigma), ("max_bad_fraction_ant", max_bad_fraction_ant),
                    ("max_bad_fraction_chan", max_bad_fraction_chan)):
        if v is not None:
            setattr(opt, name, float(v))
    sk = np.empty((n_freq, n_pol, n_ant), np.float64)
    cell = np.empty((n_freq, n_pol, n_ant), np.uint8)
    ant_flags, chan_flags = np.empty(n_ant, np.uint8), np.empty(n_freq, np.uint8)
    check(lib.bf_sk_select(_ptr(mom), int(M), n_freq, n_pol, n_ant, C.byref(opt), _ptr(sk), _ptr(cell), _ptr(ant_flags), _ptr(chan_flags)))
    return sk, cell, ant_flags, chan_flags


def vis_to_square(tri, n_ant: int):
    """The packed lower triangle [...][a1 (a1 + 1) / 2 + a2][2] (re, im) as the full Hermitian complex128 array [...][a1][a2]:
    V[a2][a1] = conj(V[a1][a2])."""
    import numpy as np

    tri = np.asarray(tri)
    assert tri.shape[-1] == 2 and tri.shape[-2] == n_ant * (n_ant + 1) // 2
    a1, a2 = np.tril_indices(n_ant)          # row-major over the lower triangle: exactly bl = a1 (a1 + 1) / 2 + a2
    z = tri[..., 0].astype(np.float64) + 1j * tri[..., 1].astype(np.float64)
    sq = np.zeros(tri.shape[:-2] + (n_ant, n_ant), np.complex128)
    sq[..., a2, a1] = np.conj(z)
    sq[..., a1, a2] = z
    return sq


# events / pinned memory as free functions (they are not tied to a handle in the C-ABI)
GATHER_FREQ_MAJOR, GATHER_RANK_MAJOR = 0, 1
GATHER_ROOT_ALL, GATHER_ROOT_DISTRIBUTED = -1, -2


def comm_unique_id() -> bytes:
    """Rank 0: the 128-byte RCCL unique id to hand to the other ranks (bf_comm_unique_id)."""
    buf = C.create_string_buffer(128)
    check(load().bf_comm_unique_id(buf))
    return buf.raw


def comm_library_info() -> dict:
    """Which librccl bf_comm_create would bind, and its version -- before any communicator exists (bf_comm_library_info)."""
    v, path = C.c_int(), C.create_string_buffer(512)
    check(load().bf_comm_library_info(C.byref(v), path, 512))
    return {"version": v.value, "lib": path.value.decode(errors="replace")}


class Comm(_Owner):
    """bf_comm: this rank's place in the frequency partition + the RCCL communicator behind bf_gather_detected."""
    _ptr_attr, _destroy = "_c", "bf_comm_destroy"

    def __init__(self, rank: int, world: int, unique_id: bytes | None = None, device: int = 0):
        self._lib = load()
        self._c = C.c_void_p()
        idbuf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        check(self._lib.bf_comm_create(rank, world, idbuf, device, C.byref(self._c)))
        self.rank, self.world = rank, world

    def info(self) -> dict:
        """{"ranks": what the library reports (ncclCommCount), "version": ncclGetVersion, "lib": file it was loaded from}."""
        n, v, path = C.c_int(), C.c_int(), C.create_string_buffer(512)
        check(self._lib.bf_comm_info(self._c, C.byref(n), C.byref(v), path, 512))
        return {"ranks": n.value, "version": v.value, "lib": path.value.decode(errors="replace")}

    def rows_held(self, n_rows: int, root: int) -> int:
        return self._lib.bf_gather_rows_held(n_rows, self.world, self.rank, root)

    def gather(self, d_local, n_rows: int, row_floats: int, root: int, layout: int, d_full, stream: int = 0) -> None:
        check(self._lib.bf_gather_detected(self._c, _ptr(d_local), n_rows, row_floats, root, layout, _ptr(d_full),
                                           C.c_void_p(stream)))

    def gather_staged(self, d_local, n_rows: int, row_floats: int, root: int, d_full, d_stage, stream: int = 0) -> None:
        """bf_gather_detected_staged: freq-major result, rank-major on the wire + one device re-layout pass."""
        check(self._lib.bf_gather_detected_staged(self._c, _ptr(d_local), n_rows, row_floats, root, _ptr(d_full), _ptr(d_stage),
                                                  C.c_void_p(stream)))


def event_create(bf=None) -> C.c_void_p:
    """An event on the caller's current device, or -- given a Beamformer -- on that handle's device (bf_event_create_on)."""
    ev = C.c_void_p()
    if bf is not None:
        check(load().bf_event_create_on(bf._h, C.byref(ev)))
    else:
        check(load().bf_event_create(C.byref(ev)))
    return ev


def event_query(ev) -> int:
    return check(load().bf_event_query(ev))


def event_destroy(ev) -> None:
    check(load().bf_event_destroy(ev))


def alloc_pinned(nbytes: int) -> int:
    p = C.c_void_p()
    check(load().bf_alloc_pinned(C.byref(p), nbytes))
    return p.value


def free_pinned(ptr: int) -> None:
    check(load().bf_free_pinned(C.c_void_p(ptr)))
