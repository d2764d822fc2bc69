/* dsabf.h -- C-ABI of libdsabf.so, the MI355X-native (gfx950) DSA beamformer hot path.
 *
 * The reference (devincody/DSAbeamformer) has no plugin/FFI layer: its device code is inlined into main()
 * of one CUDA translation unit.  This header is the drop-in boundary for that implicit interface -- one entry
 * point per cluster of CUDA/cuBLAS calls made by main(), observation_loop_state and test_data_generator
 * (SURVEY.md section 8b).  Every entry point cites the reference call sites it replaces (file:line under
 * the reference repository).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - every function returns int: 0 = BF_OK, negative = error; bf_last_error() gives the message of the
 *     calling thread's most recent failure.  The library never calls exit() (the reference's gpuErrchk does,
 *     src/beamformer.cuh:19-29; a driver may keep that policy on top of the return codes).
 *   - one host thread drives one handle (as in the reference, src/beamformer.cu:364-534); the library is
 *     re-entrant per handle but a handle is not thread-safe.
 *   - "gemm-unit": the work of one cublasGemmStridedBatchedEx call in the reference = n_freq batches of
 *     [n_beams x n_ant] . [n_ant x n_time], n_time = n_out_per_gemm * n_pol * n_avg, producing n_out_per_gemm
 *     detected [n_freq][n_beams] float32 "beam-blocks".
 *
 * Data layouts (identical to the reference's)
 *   packed voltages  uint8  [unit][freq][time][ant]      one byte per complex sample, high nibble = real,
 *                                                         low nibble = imaginary, two's complement 4-bit
 *   weights          int8   [freq][ant][beam]{re,im}     src/beamformer.cu:230-241
 *   detected power   float  [unit][output][freq][beam]   src/beamformer.cuh:147
 */
#ifndef DSABF_H
#define DSABF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BF_OK 0
#define BF_NOT_READY 1          /* bf_event_query: work still in flight (cudaErrorNotReady) */
#define BF_ERR_INVALID (-1)     /* bad argument / unsupported geometry */
#define BF_ERR_DEVICE (-2)      /* HIP runtime error (message in bf_last_error) */
#define BF_ERR_NO_DEVICE (-3)   /* no gfx950 device visible */
#define BF_ERR_STATE (-4)       /* call out of order (e.g. beamform before bf_set_weights) */

/* Geometry.  The reference fixes these at compile time (src/beamformer.hh:45-152); they are runtime here
 * because BASELINE config 5 needs 100 ant / 512 beams / 1024 freq.  bf_config_default fills the reference's
 * values (debug != 0: `make debug`, n_avg = 1; debug == 0: production, n_avg = 16). */
typedef struct bf_config {
    int n_beams;           /* N_BEAMS            src/beamformer.hh:47   multiple of 4 (:155) */
    int n_ant;             /* N_ANTENNAS         src/beamformer.hh:48   multiple of 4 (:156), at most 2048 */
    int n_freq;            /* N_FREQUENCIES      src/beamformer.hh:49   frequencies owned by THIS handle/GPU */
    int n_pol;             /* N_POL              src/beamformer.hh:52 */
    int n_avg;             /* N_AVERAGING        src/beamformer.hh:55-60  any; n_pol*n_avg in {2,...,64} powers of 2: specialised kernels */
    int n_out_per_gemm;    /* N_OUTPUTS_PER_GEMM src/beamformer.hh:111 */
    int n_gemms_per_block; /* N_GEMMS_PER_BLOCK  src/beamformer.hh:114 */
    int n_blocks_on_gpu;   /* N_BLOCKS_ON_GPU    src/beamformer.hh:124 */
    int n_streams;         /* N_STREAMS          src/beamformer.hh:83 */
    int verbose;           /* -DVERBOSE as a runtime flag */
    int detect_mode;       /* BF_DETECT_CANONICAL (0, default), BF_DETECT_CONTRACTED or BF_DETECT_FAST */
} bf_config;

/* detect_mode: how the power term of detect_sum, `acc += x*x + y*y` (src/beamformer.cuh:150-152), is evaluated.  x, y are
 * the float32 real / imaginary parts fl(n * (float)(1/127)) of one beam sample, n the exact integer dot product.
 *   BF_DETECT_CANONICAL   xx = x*x; yy = y*y; p = xx + yy; acc = acc + p -- two multiplies, an add and the accumulate add,
 *                         ascending time order: what the reference's source says when no contraction happens (g++ on
 *                         x86-64, the CPU restatement in oracle/).  Bit-identical to that restatement for every geometry.
 *   BF_DETECT_CONTRACTED  yy = y*y; p = fma(x, x, yy); acc = acc + p -- what nvcc makes of the same source with its
 *                         default -fmad=true (the reference's makefile:13-16 never turns it off), i.e. most likely the
 *                         bits the reference's GPU build produces.  5 instead of 6 VALU ops per sample.  Bit-identical to
 *                         the restatement's ORC_CONTRACT_NVCC reading.
 *   BF_DETECT_FAST        (n_pol*n_avg >= 16; canonical elsewhere) d = 16 n exactly; acc = fma(d, d, acc) for re then im;
 *                         one (alpha/16)^2 scale per output: 4 VALU ops per sample.
 * Which of the first two the reference's device code really computes cannot be decided without NVIDIA hardware; the
 * stated tolerance covers all three: with E = alpha^2 * sum over the n_ipo samples of |n|^2 evaluated exactly,
 *   |canonical - E|, |contracted - E| <= (n_ipo + 4) * 2^-24 * E        |fast - E| <= (n_ipo + 1) * 2^-23 * E
 * (at most 4 roundings per term -- x, x^2 or the fma, y^2, the pair sum -- plus n_ipo - 1 accumulate roundings of
 * non-negative terms; fast: 2 n_ipo fma roundings, the scale and its constant).  tests/test_oracle.py and
 * tests/test_gpu_parity.py hold all modes to these bounds; measured errors are a few units of 2^-24. */
#define BF_DETECT_CANONICAL 0
#define BF_DETECT_FAST 1
#define BF_DETECT_CONTRACTED 2

typedef struct bf_handle bf_handle; /* owns device memory, 1 transfer queue + n_streams compute queues */
typedef struct bf_event bf_event;

/* Replace gpuErrchk / gpuBLASchk, src/beamformer.cuh:19-36 (print `GPUassert: <msg> <file> <line>` and exit): the message of
 * the calling thread's most recent failure, and the library's identification string. */
const char *bf_last_error(void);
const char *bf_version(void);

/* The reference's compile-time geometry as a value, src/beamformer.hh:45-152 (debug != 0: N_AVERAGING 1, :55-57). */
int bf_config_default(bf_config *cfg, int debug);
/* Derived sizes (src/beamformer.hh:117,120,144,147,137): */
int bf_n_inputs_per_output(const bf_config *cfg);  /* N_INPUTS_PER_OUTPUT */
int bf_n_timesteps_per_gemm(const bf_config *cfg); /* N_TIMESTEPS_PER_GEMM */
size_t bf_bytes_per_gemm(const bf_config *cfg);    /* N_BYTES_PRE_EXPANSION_PER_GEMM */
size_t bf_bytes_per_block(const bf_config *cfg);   /* N_BYTES_PRE_EXPANSION_PER_BLOCK */
size_t bf_floats_per_detect(const bf_config *cfg); /* N_F_PER_DETECT */

/* Device selection.  Replaces CUDA_select_GPU (src/beamformer.cuh:171-192): device index instead of a name
 * match; bf_device_name reports what was found. */
int bf_device_count(int *count);
int bf_device_name(int device, char *buf, size_t buflen);

/* Replaces: allocations src/beamformer.cu:249-266, memsets :291-298, streams/handles :305-320 and the
 * teardown :560-605.  d_B and d_C of the reference do not exist here (expand, GEMM and detect are fused).
 * bf_destroy drains the handle's queues first, as the reference's teardown does (cudaStreamSynchronize of every stream,
 * src/beamformer.cu:560-562): gemm-units that bf_enqueue_gemm_unit accepted and nothing has launched yet are launched, and their
 * host copies land -- so the host_out / host_out_row buffers of every enqueued unit must stay valid until bf_destroy has
 * returned (free pinned memory AFTER the handle, as the reference frees beam_out after its streams, :605,613). */
int bf_create(const bf_config *cfg, int device, bf_handle **out);
int bf_destroy(bf_handle *h);
int bf_get_config(const bf_handle *h, bf_config *cfg); /* the geometry the handle was built for (the #defines of src/beamformer.hh:45-152) */

/* Replaces the weight upload src/beamformer.cu:251,272.  `w` is a HOST array in the reference layout
 * [freq][ant][beam]{re,im} int8; the library re-lays it out once for the MFMA operand fragments.
 * Imaginary parts must be >= -127 (the reference's round(127*sin) never produces -128).
 * If W[f][a][n_beams-1-b] == conj(W[f][a][b]) for every f, a, b -- any beam set symmetric about the boresight, e.g. the
 * reference's -- the library notices (checked on the device, exactly) and runs a kernel that forms each such beam pair
 * from shared products: half the matrix-core work, identical results.  Nothing to configure.
 * If W[f][n_ant-1-a][b] == conj(W[f][a][b]) for every f, a, b -- an array that is point-symmetric about its phase centre: any
 * regular line or grid with the reference's steering weights -- and the geometry is 64 antennas with an accumulation window of
 * 16, 32 or 64 samples, the library notices that too and folds each mirror pair of antennas into one matrix-core operand (sums and
 * differences of the two voltages): the same halved matrix-core work for ANY beam set, fewer vector instructions per sample,
 * identical results.  A calibrated array (per-antenna gains and phases) has neither symmetry and runs the general kernel. */
int bf_set_weights(bf_handle *h, const int8_t *w);
/* Same (the cudaMemcpy of src/beamformer.cu:272 becomes a device-side read), from a DEVICE array: caller-owned HBM, e.g.
 * weights computed on the GPU or a sharded slice. */
int bf_set_weights_device(bf_handle *h, const int8_t *d_w, void *hip_stream);

/* Replaces cudaHostAlloc/cudaFreeHost in src/test_data_generator.hh:35,40 and src/beamformer.cu:212,249,
 * 605,613 (pinned input batch, beam_out, dedispersed_out). */
int bf_alloc_pinned(void **ptr, size_t nbytes);
int bf_free_pinned(void *ptr);
/* Replace cudaHostRegister / cudaHostUnregister on the PSRDADA data blocks (dada_cuda_dbregister /
 * dada_cuda_dbunregister, src/dada_handler.hh:127-177): page-lock caller-owned host memory for DMA. */
int bf_host_register(void *ptr, size_t nbytes);
int bf_host_unregister(void *ptr);

/* Events.  Replace the cudaEvent ring of observation_loop_state (src/observation_loop.hh:58-61,65-68,73,
 * 79,86,95-96,105,112-113).  bf_event_query returns BF_OK (done), BF_NOT_READY, or a negative error. */
int bf_event_create(bf_event **ev);                    /* on the caller's current device (as cudaEventCreate) */
int bf_event_create_on(bf_handle *h, bf_event **ev);   /* on the handle's device: use this for events that bf_submit_block /
                                                        * bf_record_*_event of `h` will record when h's device may not be
                                                        * the caller's current one (`beam -D i`, one thread driving several GPUs) */
int bf_event_destroy(bf_event *ev);
int bf_event_query(bf_event *ev);
int bf_event_synchronize(bf_event *ev);

/* Replaces cudaMemcpyAsync H2D of one PSRDADA block + generate_transfer_event, src/beamformer.cu:389-396,
 * 425-431 and src/observation_loop.hh:71-75.  Copies `nbytes` (<= bf_bytes_per_block) from host memory into
 * ring slot `slot` (0 .. n_blocks_on_gpu-1) on the transfer queue and records `ev` (may be NULL) behind it.
 * The host buffer must stay valid until the event fires. */
int bf_submit_block(bf_handle *h, int slot, const void *host, size_t nbytes, bf_event *ev);

/* Replaces generate_transfer_event's cudaEventRecord(..., HtoDstream), src/observation_loop.hh:73, when the
 * copy and the event are issued separately (bf_submit_block with ev == NULL, then this). */
int bf_record_transfer_event(bf_handle *h, bf_event *ev);

/* Replaces K1-K4 for one gemm-unit, src/beamformer.cu:464-488: expand_input, cublasGemmStridedBatchedEx,
 * detect_sum and the D2H copy of the detected powers.  Reads gemm-unit `time_slice` (0 .. n_gemms_per_block-1)
 * of ring slot `slot`, produces [n_out_per_gemm][n_freq][n_beams] float32 on the device and, if host_out != NULL,
 * copies it there asynchronously (host_out should be pinned).
 * The caller keeps the reference's loop -- one call per gemm-unit, round-robin over the N_STREAMS queues,
 * src/beamformer.cu:454-519 -- but the calls are COALESCED: units are queued and, per run of consecutive time slices of
 * one slot (the reference's loop enqueues 0, 1, 2, ... of a block: one run), launched as ONE kernel, with one DM-0 launch for
 * the units that bf_enqueue_dedisperse was called for and the host copies behind it -- every unit's, in call order, so a
 * host buffer written by several units ends up holding the last one, as on the reference's per-queue streams.  One-unit
 * launches cannot fill the chip (0.28 of the int8 peak alone, 0.385 with 8 in flight; a block launch 0.49); same results.
 * The queued work is launched when a block's worth (n_gemms_per_block units) is queued and at every call that orders or
 * observes device work: bf_record_analysis_event (the reference calls it after each block, :525), bf_stream_sync,
 * bf_enqueue_block*, bf_enqueue_d2h, bf_queue_stream, bf_timer_stop, bf_destroy.  Ordering contract -- the literal pattern's:
 * once launched, a unit's kernel and host copy are ORDERED ON QUEUE stream_idx (that queue waits for the coalesced launch
 * wherever it ran), so anything the caller puts on that queue afterwards -- bf_enqueue_d2h, a hipStreamSynchronize or an event
 * of its own on the hipStream_t from bf_queue_stream, RCCL chained on it -- sees the unit complete; and a unit's results are
 * complete when an event of bf_record_analysis_event recorded after the call fires, or after bf_stream_sync.  What is NOT the
 * literal pattern: a hipStream_t obtained earlier says nothing about units that are still only queued (nothing has been
 * launched for them yet) -- one of the calls above launches them.  DSABF_COALESCE=0 at bf_create (or the "coalesce" switch of
 * dsabf_bench.h): the literal pattern itself, one launch per call on queue stream_idx. */
int bf_enqueue_gemm_unit(bf_handle *h, int stream_idx, int slot, int time_slice, float *host_out);

/* Block-granular form of the same: ONE kernel launch over the n_units consecutive gemm-units [first_unit, first_unit +
 * n_units) of ring slot `slot` on compute queue `stream_idx` (the reference launches K1-K3 once per gemm-unit,
 * src/beamformer.cu:454-519; a whole PSRDADA block of 32 units keeps the chip filled where one unit cannot).  The detected
 * powers land in a per-queue device buffer of n_gemms_per_block units; host_out, if not NULL, is an array of n_units host
 * pointers (pinned; NULL entries are skipped): unit first_unit + i is copied to host_out[i] asynchronously, behind the
 * launch, on the same queue.  Results are identical to n_units calls of bf_enqueue_gemm_unit.
 * The per-queue buffer is allocated when a queue is first used: a caller that rotates over queues reserves them BEFORE its loop
 * with bf_block_output_device(h, q, &p) for every queue it will use (a hipMalloc in the middle of a stream of blocks stalls the
 * device: 9.4 -> 10.9 us per beam-block measured; run_observation and examples/ do).
 * bf_enqueue_block_to: the same launch with the powers written to d_dst (device, room for n_units * bf_floats_per_detect floats,
 * [unit][o][f][b]) instead of the queue's buffer -- for a consumer that owns the place the rows belong in (bf_dm_stream_reserve:
 * the frequency collapse directly behind detect, src/beamformer.cu:481,492-511, with no copy in between). */
int bf_enqueue_block(bf_handle *h, int stream_idx, int slot, int first_unit, int n_units, float *const *host_out);
int bf_enqueue_block_to(bf_handle *h, int stream_idx, int slot, int first_unit, int n_units, float *d_dst, float *const *host_out);

/* Replaces K5, the DEBUG dedisperse, src/beamformer.cu:498-510: sums output 0 of the unit last enqueued on
 * `stream_idx` over frequency (ascending f, fp32) and copies the n_beams floats to host_out_row. */
int bf_enqueue_dedisperse(bf_handle *h, int stream_idx, float *host_out_row);
/* The same K5 (src/beamformer.cu:498-510) for the gemm-units [first_unit, first_unit + n_units) of the block bf_enqueue_block last put on
 * `stream_idx`, in ONE launch (units x beams threads; every beam's sum still runs over ascending f in one thread, so the
 * bits are those of n_units bf_enqueue_dedisperse calls).  host_rows, if not NULL, receives [n_units][n_beams] floats. */
int bf_enqueue_block_dedisperse(bf_handle *h, int stream_idx, int first_unit, int n_units, float *host_rows);

/* Replaces generate_analysis_event, src/beamformer.cu:525 / src/observation_loop.hh:77-81.  The reference
 * records on stream[N_STREAMS-1] only (a latent race); this records `ev` behind ALL
 * compute queues. */
int bf_record_analysis_event(bf_handle *h, bf_event *ev);

/* Replaces cudaStreamSynchronize x N_STREAMS, src/beamformer.cu:560-562 (stream_idx < 0: all queues incl.
 * the transfer queue). */
int bf_stream_sync(bf_handle *h, int stream_idx);

/* Replaces START_TIMER / STOP_RECORD_TIMER, src/beamformer.cuh:43-58 (events on the default queue order). */
int bf_timer_start(bf_handle *h);
int bf_timer_stop(bf_handle *h, float *ms);

/* ---- Device-pointer entry points: operands already resident in HBM (caller-owned memory and queue). ----
 * These are what bench.py and the multi-GPU path call; `hip_stream` is a hipStream_t (NULL = default). */

/* K1-K3 of src/beamformer.cu:464-481 (expand_input, cublasGemmStridedBatchedEx, detect_sum) without the copies around them.
 * Fused a1+a2+a3 over n_units gemm-units: d_packed [n_units][freq][time][ant] -> d_out
 * [n_units][output][freq][beam].  One kernel launch.  Both pointers must be 16-byte aligned (16-byte loads; groups of
 * four beams are stored with one 16-byte store).  Like every entry point, the call leaves the caller's current HIP
 * device as it found it. */
int bf_beamform_device(bf_handle *h, const void *d_packed, int n_units, float *d_out, void *hip_stream);

/* The incoherent beam (docs/INCOHERENT_BEAM.md): what detect_sum, src/beamformer.cuh:139-154, computes for a tied beam -- the sum
 * of |.|^2 over the n_pol * n_avg samples of an output window -- taken of the antenna voltages themselves, summed over the
 * antennas, with no weights: per gemm-unit u, output o and channel f
 *   S = sum over the n_pol * n_avg * n_ant packed bytes of the window of re^2 + im^2        out = (float)S
 * S is an exact integer, summed in integer arithmetic, so the result is the same for every launch path and bit-equal to a
 * restatement in any order.  Defined where 128 * n_ant * n_pol * n_avg <= 2^24 (a sample contributes at most 128: the
 * conversion to float is then exact); beyond that both calls return BF_ERR_INVALID.  With steering weights of modulus ~127 and
 * detect's 1/127^2 a tied beam on noise has expectation ~S: the two are in the same units.
 * bf_incoherent_device: d_packed [n_units][freq][time][ant] as for bf_beamform_device (16-byte aligned) ->
 *   d_out[((u * n_out_per_gemm + o) * n_freq + f) * stride], one float each: stride 1 gives the compact [unit][o][f] array,
 *   stride n_beams with d_out advanced by b the column of beam b in a detected array.  One kernel launch; needs no weights.
 * bf_set_incoherent_beam(h, b): from now on EVERY detect launch of the handle -- the loop's K1-K3 of src/beamformer.cu:464-488
 *   behind bf_enqueue_gemm_unit (coalesced or not), bf_enqueue_block, bf_enqueue_block_to, and bf_beamform_device -- is followed on
 *   the same queue by that launch into column b of the same output, in front of everything that reads it there (the host copies,
 *   the DM-0 collapse, the DM stage): for every consumer "beam b" IS the incoherent beam, at the price of one tied beam.  -1: off
 *   (the default).  Gemm-units that are still only queued are launched first and keep the old setting.  The weights are
 *   untouched and the tied beam b is still computed, then overwritten: which fused kernel runs does not change, and a caller who
 *   wants the conjugate-pair kernel keeps that column's weights symmetric like the rest.  bf_gemm_device is no detect launch. */
int bf_incoherent_device(bf_handle *h, const void *d_packed, int n_units, float *d_out, size_t stride, void *hip_stream);
int bf_set_incoherent_beam(bf_handle *h, int beam);

/* ---- The correlator (docs/CORRELATOR.md) ---------------------------------------------------------------------------------
 * The reference uploads steering weights only (src/beamformer.cu:230-241); a real array multiplies them by per-(frequency, antenna)
 * gains, and those are solved from VISIBILITIES: per channel the cross-products of the antenna voltages, taken on a calibrator.
 * The voltages are the packed bytes the beamformer reads ([unit][freq][time][ant], time = n_out_per_gemm * n_pol * n_avg).
 * POLARISATION ORDER -- the one place the library reads it: the reference never tells polarisation from time inside a window; its
 * README documents the order Time x Polarization x Antenna, polarisation fastest, and the correlator takes that order: column c of
 * a gemm-unit belongs to polarisation c % n_pol.  Per channel f and polarisation p
 *   V[f][p][a1][a2] = sum over the units and over the columns c = p (mod n_pol) of v[u][f][c][a1] * conj(v[u][f][c][a2]),   a2 <= a1
 * stored as the packed lower triangle [freq][pol][bl]{re, im}, bl = a1 * (a1 + 1) / 2 + a2: n_ant * (n_ant + 1) / 2 entries per
 * (f, p), two int64 each; the diagonal is the autocorrelation (im == 0).  Every sum is an exact integer (int8 MFMA with time as the
 * K axis, int32 within a launch, int64 in memory): the result is the same for every launch path and bit-equal to a restatement in
 * any order (tests/support/corr_oracle.py).  Known answer: bytes 0xD7 (-3+7i) at antenna 1 and 0x25 (2+5i) at antenna 0 in one
 * column give V[1][0] = (29, 29), V[1][1] = (58, 0), V[0][0] = (29, 0).
 * Bounds: a column contributes at most 128 to either part; with N = n_units * n_out_per_gemm * n_avg columns per polarisation in
 * one call, the call is defined for 128 * N <= 2^31 - 1, i.e. N < 2^24, and for n_ant <= 256 (any multiple of 4; the output grows
 * as n_ant^2).  Beyond either every call below returns BF_ERR_INVALID and launches nothing.
 * bf_correlate_device: d_packed as for bf_beamform_device (16-byte aligned) -> d_vis (device, bf_corr_entries(cfg) * 2 int64),
 *   overwritten (accumulate == 0) or added to (accumulate != 0).  One kernel launch; needs no weights: callable before
 *   bf_set_weights.  bf_corr_entries: n_freq * n_pol * n_ant * (n_ant + 1) / 2 complex entries (two int64 each).
 * A bf_corr is the correlator as a STAGE: it owns one int64 accumulator on the device, a column count and max_in_flight pinned
 *   result sets.  bf_corr_push adds n_units gemm-units at d_packed, asynchronously on hip_stream; bf_corr_push_block the units
 *   [first_unit, first_unit + n_units) of ring slot `slot` -- the resident block bf_enqueue_block reads -- on compute queue
 *   stream_idx, behind whatever that queue holds.  bf_corr_dump snapshots the accumulator into the next pinned set and zeroes it
 *   (on a copy queue of the stage; hip_stream is not held).  Pushes and dumps of one stage share the accumulator, so the stage
 *   orders them itself, whichever queues they are issued on: each waits for the kernel or copy of the one before it, and a push
 *   holds the caller's queue for its kernel only.  A dump beyond max_in_flight uncollected ones returns BF_ERR_STATE before it
 *   queues anything.  bf_corr_collect waits for the OLDEST uncollected dump and copies its entries to `out` (host, bf_corr_entries
 *   * 2 int64) and the columns per polarisation it integrated to *n_columns_per_pol (may be NULL); nothing pending: BF_ERR_STATE.
 *   bf_corr_pending: dumps not yet collected.  Lifetime as for a bf_sps: a handle that goes first releases the device memory, the
 *   stage then answers BF_ERR_STATE and can still be destroyed. */
int bf_correlate_device(bf_handle *h, const void *d_packed, int n_units, int64_t *d_vis, int accumulate, void *hip_stream);
size_t bf_corr_entries(const bf_config *cfg);
typedef struct bf_corr bf_corr;
int bf_corr_create(bf_handle *h, int max_in_flight, bf_corr **out);
int bf_corr_destroy(bf_corr *c);
int bf_corr_push(bf_corr *c, const void *d_packed, int n_units, void *hip_stream);
int bf_corr_push_block(bf_corr *c, int stream_idx, int slot, int first_unit, int n_units);
int bf_corr_dump(bf_corr *c, void *hip_stream);
int bf_corr_collect(bf_corr *c, int64_t *out, uint64_t *n_columns_per_pol);
int bf_corr_pending(const bf_corr *c);

/* ---- The gain solver and calibrated weights (docs/CALIBRATION.md) ------------------------------------------------------------
 * Extends the weight upload, src/beamformer.cu:230-241 (the steering weights), :251, :272 (their allocation and copy): between
 * the visibilities of a calibrator (bf_correlate_device) and the weights a calibrated array uploads (bf_set_weights_device) sit the
 * per-(channel, polarisation, antenna) complex gains g with V[a1][a2] ~ g[a1] conj(g[a2]) M[a1][a2], M[p][q] = s_p conj(s_q) the
 * model of one point source.  bf_solve_gains_device solves them with StEFCal (Salvini & Wijnholds 2014) on the device, one
 * workgroup per (channel, polarisation layer); bf_calibrate_weights_device multiplies a weight array by conj(g) / |g|.
 * The arithmetic is fp64, one rounding per operation (no fused multiply-add), every sum in ONE fixed order (OSUM, docs/CALIBRATION.md
 * section 2), so the result is bit-equal to a numpy restatement (tests/support/cal_oracle.py) whatever path the kernel takes.
 * bf_solve_gains_device: d_vis as bf_correlate_device leaves it ([freq][pol][bl]{re, im} int64), d_model NULL (all ones: the source
 *   at the phase centre) or fp64 [freq][ant]{re, im} (the calibrator's steering phasors s), d_flags NULL or uint8 [ant] (non-zero:
 *   the antenna is left out and its gain is exactly (0, 0)).  opt: tol (stop when |g - g_prev| <= tol |g|, tested on even
 *   iterations), max_iter >= 1, ref_ant (the antenna whose gain gets zero phase; -1: the first unflagged one), joint_pol (non-zero:
 *   the polarisations' integers are added first and ONE layer is solved -- the beamformer has one weight per (f, a, b) for both).
 *   d_gains: fp64 [pol_out][freq][ant]{re, im}, pol_out = joint_pol ? 1 : n_pol (bf_cal_gain_entries complex entries; one layer is
 *   contiguous); d_info: int32 [pol_out][freq]{iterations, status}, status 1 = converged, 0 = max_iter ran out.  A dead antenna
 *   (a zero row) stays at (0, 0); no NaN is produced.  d_vis, d_model, d_gains 16-byte aligned.
 * bf_calibrate_weights_device: d_w_in / d_w_out int8 [freq][ant][beam]{re, im} as for bf_set_weights_device (4-byte aligned; they
 *   may be the same array), d_gains_layer ONE layer [freq][ant]{re, im}.  Per (f, a) with m = |g|: BF_CAL_PHASE c = conj(g) / m;
 *   BF_CAL_FULL c = conj(g) / m * (k_f / m), k_f the smallest non-zero m among the channel's unflagged antennas (|c| <= 1); a flagged
 *   or zero-gain antenna gets c = 0.  Each part of w * c is rounded half to even and clipped to [-127, 127].
 * Both calls are asynchronous on hip_stream, need no weights set, leave the caller's current device as found and keep NO state or
 *   scratch in the handle (the solver reads d_vis in place), so calls issued on different queues without synchronisation are
 *   independent.  One exception to "asynchronous": with ref_ant >= 0 AND d_flags given, the solver reads that one flag byte back
 *   behind hip_stream (it waits for the queue) to refuse a flagged reference.  Defined for n_ant a multiple of 4 up to 256; beyond
 *   that, and for max_iter < 1, tol < 0, ref_ant out of range or flagged, a mode that is neither, or a NULL pointer, they return
 *   BF_ERR_INVALID and launch nothing.  bf_cal_default_options: tol 1e-10, max_iter 200, ref_ant -1, joint_pol 0. */
typedef struct {
    double tol;
    int max_iter;
    int ref_ant;
    int joint_pol;
} bf_cal_options;
#define BF_CAL_PHASE 0
#define BF_CAL_FULL 1
int bf_cal_default_options(bf_cal_options *o);
size_t bf_cal_gain_entries(const bf_config *cfg, int joint_pol);
int bf_solve_gains_device(bf_handle *h, const int64_t *d_vis, const double *d_model, const uint8_t *d_flags, const bf_cal_options *opt,
                          double *d_gains, int32_t *d_info, void *hip_stream);
int bf_calibrate_weights_device(bf_handle *h, const int8_t *d_w_in, const double *d_gains_layer, const uint8_t *d_flags, int mode,
                                int8_t *d_w_out, void *hip_stream);

/* ---- The spatial null: interferer vectors from visibilities, projected weights (docs/NULLING.md) ------------------------------
 * Extends the weight upload as the gain solver does, src/beamformer.cu:230-241 (the steering weights), :251, :272 (their allocation
 * and copy): an interferer that is strong in every antenna occupies ONE direction of antenna space per channel, the dominant
 * eigenvector of the visibility matrix V[a1][a2] = sum v[a1] conj(v[a2]) that bf_correlate_device measures.  bf_null_solve_device finds
 * the n_null dominant eigenvectors u_j per channel by power iteration with deflation, one workgroup per channel;
 * bf_null_weights_device removes them from every beam: w' = w - sum_j conj(u_j) (u_j^T w), so that u_j^T w' = 0 -- the beam sample is
 * sum_a v_a w_a, and v ~ s u for the interferer.  The fused kernels run unchanged with other weight bytes.
 * The arithmetic is fp64, one rounding per operation (no fused multiply-add), every sum over antennas in the OSUM order of
 * docs/CALIBRATION.md section 2, so the result is bit-equal to a numpy restatement (tests/support/null_oracle.py) on every path.
 * bf_null_solve_device: d_vis as bf_correlate_device leaves it, d_flags NULL or uint8 [ant] (non-zero: the antenna's row and column
 *   are zero, and so are its vector entries).  opt: n_null 1 ... BF_NULL_MAX vectors per channel; min_ratio: vector j is used only if
 *   lambda_j >= min_ratio * max(rest_j, 0), rest_j = (trace - lambda_0 - ... - lambda_j) / (m - j - 1) the mean of what is left over the
 *   m unflagged antennas (0: always), and only if every earlier vector is used, m > j + 1 and lambda_j > 0; tol: stop when
 *   |u - u_prev| <= tol; max_iter >= 1 multiplications per vector; pol -1: the polarisations' integers are added first (the
 *   beamformer has one weight per (f, a, b) for both), 0 ... n_pol - 1: that polarisation alone.
 *   d_vecs: fp64 [freq][n_null][ant]{re, im} (bf_null_vec_entries complex entries), unit vectors, exact zeros where unused;
 *   d_eig: fp64 [freq][n_null + 1], the lambdas and then the trace; d_info: int32 [freq][1 + 2 n_null], n_used and then
 *   {iterations, status} per vector: status 1 = converged, 0 = max_iter ran out (the vector is used all the same: it lies in the
 *   dominant subspace), 2 = nothing was left (this vector and all later ones are zero).  No NaN is produced.  d_vis and d_vecs
 *   16-byte aligned.
 * bf_null_weights_device: d_w_in / d_w_out int8 [freq][ant][beam]{re, im} as for bf_set_weights_device (4-byte aligned; they may be
 *   the same array); d_vecs, d_info and n_null as the solver left them; d_flags as given to the solver.  Channels with n_used > 0:
 *   each part of k_f w' is rounded half to even and clipped to [-127, 127]; BF_NULL_SCALED k_f = min(1, 127 / M_f) with M_f the
 *   largest |part| of w' in the channel, BF_NULL_CLIP k_f = 1.  Channels with n_used == 0 are copied byte for byte, k_f = 1.  Flagged
 *   antennas get (0, 0) in both.  d_scale NULL or fp64 [freq]: k_f (the channel's power gain is k_f^2).
 * Both calls are asynchronous on hip_stream, need no weights set, leave the caller's current device as found and keep NO state or
 *   scratch in the handle, so calls issued on different queues without synchronisation are independent.  Defined for n_ant a multiple
 *   of 4 up to 256; beyond that, and for n_null outside 1 ... BF_NULL_MAX, max_iter < 1, tol or min_ratio negative or NaN, pol out of
 *   range, a mode that is neither, or a NULL or misaligned pointer, they return BF_ERR_INVALID and launch nothing.
 *   bf_null_default_options: min_ratio 4.0, tol 1e-6, n_null 1, max_iter 200, pol -1. */
typedef struct {
    double min_ratio;
    double tol;
    int n_null;
    int max_iter;
    int pol;
} bf_null_options;
#define BF_NULL_MAX 4
#define BF_NULL_SCALED 0
#define BF_NULL_CLIP 1
int bf_null_default_options(bf_null_options *o);
size_t bf_null_vec_entries(const bf_config *cfg, int n_null);
int bf_null_solve_device(bf_handle *h, const int64_t *d_vis, const uint8_t *d_flags, const bf_null_options *opt, double *d_vecs,
                         double *d_eig, int32_t *d_info, void *hip_stream);
int bf_null_weights_device(bf_handle *h, const int8_t *d_w_in, const double *d_vecs, const int32_t *d_info, int n_null,
                           const uint8_t *d_flags, int mode, int8_t *d_w_out, double *d_scale, void *hip_stream);

/* ---- Voltage moments and spectral kurtosis (docs/SPECTRAL_KURTOSIS.md) --------------------------------------------------------
 * Reads what the loop's kernels read, src/beamformer.cu:454-488 (the packed voltages of the resident gemm-units), and produces what
 * the calibration path above takes and nothing else here makes: antenna flags.  Per (antenna, channel, polarisation) cell two power
 * moments of the voltages, S1 = sum |v|^2 and S2 = sum |v|^4, give the spectral-kurtosis estimator: ~1 for Gaussian noise, ~0 for a
 * constant-envelope carrier, > 1 for intermittent interference; S1 == 0 is a dead input.
 * Input: packed [unit][freq][time][ant], one byte per complex sample, re in the high nibble and im in the low nibble, both two's
 * complement, time = n_out_per_gemm * n_pol * n_avg; polarisation order as for the correlator: column c of a unit belongs to
 * polarisation c % n_pol.  With p = re^2 + im^2 (0 ... 128)
 *   M1[f][pol][a] = sum over the units and the columns c = pol (mod n_pol) of p          M2[f][pol][a] = the same sum of p^2
 * stored as [freq][pol][ant]{m1, m2}, two int64 per cell; bf_sk_entries(cfg) = n_freq * n_pol * n_ant cells.  The sums are exact
 * integers, so their order is free and the result is bit-equal to a numpy restatement (tests/support/sk_oracle.py) for every
 * geometry and launch path.  Known answer: the bytes 0xD7 0x25 0xA8 0x70 as four columns of one antenna with n_pol = 1 give
 * M1 = 58 + 29 + 100 + 49 = 236 and M2 = 58^2 + 29^2 + 100^2 + 49^2 = 16606.
 * Bounds: a call is defined for N < 2^24 columns per polarisation, N = n_units * n_out_per_gemm * n_avg (the correlator's bound:
 * M1 <= 128 * N fits int32; p^2 <= 2^14, so the kernel widens its int32 partials of M2 before 2^17 columns), for any n_ant % 4 == 0
 * up to 2048 (the output is linear in n_ant: the correlator's 256 do not apply) and n_pol <= 64.  Beyond them every entry point
 * below returns BF_ERR_INVALID with a message and launches nothing.
 * bf_sk_device: d_packed as for bf_beamform_device (16-byte aligned) -> d_moments (device, bf_sk_entries(cfg) * 2 int64, 8-byte
 *   aligned), overwritten (accumulate == 0) or added to (accumulate != 0).  Asynchronous on hip_stream; needs no weights; leaves
 *   the caller's current device as found.
 * bf_sk_select: a pure host function in fp64, one rounding per operation in exactly this order (it touches no device).  For M =
 *   n_columns_per_pol >= 2 and per cell with moments m1, m2:
 *     m1 == 0 -> sk = 0.0, cell code BF_SK_DEAD
 *     else       r = ((double)M * (double)m2) / ((double)m1 * (double)m1)        sk = ((double)(M + 1) / (double)(M - 1)) * (r - 1.0)
 *                half_width = n_sigma * 2.0 / sqrt((double)M)
 *                code |= BF_SK_LOW if sk < centre - half_width                   code |= BF_SK_HIGH if sk > centre + half_width
 *   Antenna a is flagged when (double)bad_a > max_bad_fraction_ant * (double)(n_freq * n_pol), bad_a its cells with a non-zero code;
 *   channel f when the bad cells of the UNFLAGGED antennas at f satisfy (double)bad_f > max_bad_fraction_chan * (double)(n_good_ant *
 *   n_pol), and always when no antenna is unflagged.  Outputs, each may be NULL: sk double [freq][pol][ant], cell uint8
 *   [freq][pol][ant], ant_flags uint8 [ant] (what bf_solve_gains_device and bf_calibrate_weights_device take as d_flags),
 *   chan_flags uint8 [freq] (what bf_cond_set_mask takes).  opt NULL: the defaults.  M < 2 or moments NULL: BF_ERR_INVALID.
 *   bf_sk_default_options: centre 1.0, n_sigma 5.0, both fractions 0.5 -- conventions, not measurements: 4-bit quantisation moves
 *   the centre (docs/SPECTRAL_KURTOSIS.md), an operator takes it from a clean moments file of their own levels.
 * A bf_sk is the measurement as a STAGE, a twin of bf_corr: one int64 accumulator on the device, a column count and max_in_flight
 *   pinned result sets.  bf_sk_push adds n_units gemm-units at d_packed, asynchronously on hip_stream; bf_sk_push_block the units
 *   [first_unit, first_unit + n_units) of ring slot `slot` on compute queue stream_idx, behind whatever that queue holds.
 *   bf_sk_dump snapshots the accumulator into the next pinned set and zeroes it, on a copy queue of the stage (hip_stream is not
 *   held).  The stage orders its pushes and dumps itself, whichever queues they are issued on.  A dump beyond max_in_flight
 *   uncollected ones returns BF_ERR_STATE before it queues anything.  bf_sk_collect waits for the OLDEST uncollected dump and copies
 *   its moments to `out` (host, bf_sk_entries * 2 int64) and the columns per polarisation it integrated to *n_columns_per_pol (may
 *   be NULL); nothing pending: BF_ERR_STATE.  bf_sk_pending: dumps not yet collected.  A handle that goes first releases the device
 *   memory; the stage then answers BF_ERR_STATE and can still be destroyed. */
typedef struct {
    double centre;
    double n_sigma;
    double max_bad_fraction_ant;
    double max_bad_fraction_chan;
} bf_sk_options;
#define BF_SK_DEAD 1
#define BF_SK_LOW 2
#define BF_SK_HIGH 4
int bf_sk_device(bf_handle *h, const void *d_packed, int n_units, int64_t *d_moments, int accumulate, void *hip_stream);
size_t bf_sk_entries(const bf_config *cfg);
int bf_sk_default_options(bf_sk_options *o);
int bf_sk_select(const int64_t *moments, uint64_t n_columns_per_pol, int n_freq, int n_pol, int n_ant, const bf_sk_options *opt, double *sk,
                 uint8_t *cell, uint8_t *ant_flags, uint8_t *chan_flags);
typedef struct bf_sk bf_sk;
int bf_sk_create(bf_handle *h, int max_in_flight, bf_sk **out);
int bf_sk_destroy(bf_sk *c);
int bf_sk_push(bf_sk *c, const void *d_packed, int n_units, void *hip_stream);
int bf_sk_push_block(bf_sk *c, int stream_idx, int slot, int first_unit, int n_units);
int bf_sk_dump(bf_sk *c, void *hip_stream);
int bf_sk_collect(bf_sk *c, int64_t *out, uint64_t *n_columns_per_pol);
int bf_sk_pending(const bf_sk *c);

/* ---- Full-Stokes follow-up beams (docs/STOKES.md) --------------------------------------------------------------------------------
 * The detect of the loop adds |X|^2 + |Y|^2 of the two polarisation columns into one float (src/beamformer.hh:116, BF_DETECT_* above)
 * and integrates N_AVERAGING samples (src/beamformer.hh:52); the phase between the feeds -- Stokes Q, U, V -- and every time scale
 * below the window are gone.  A bf_stokes reads the same resident packed voltages the loop's GEMM reads (src/beamformer.cu:179) and
 * forms, for a FEW selected beams, all four Stokes parameters at a window of its own.
 * Input: packed [unit][freq][time][ant], one byte per complex sample, re in the high nibble and im in the low nibble, both two's
 * complement; time = n_out_per_gemm * n_pol * n_avg; column c belongs to polarisation c % n_pol (README.md:53, the correlator's order).
 * n_pol must be 2: sample j of a unit is the column pair (2j, 2j + 1) = (X, Y); a unit has S = n_out_per_gemm * n_avg samples.
 * Weights: K beams of the stage's own, 1 <= K <= BF_STOKES_MAX_BEAMS, picked by the index list `beams` (any order, any of [0, n_beams))
 * from an array in the layout of bf_set_weights, [freq][ant][beam]{re, im} int8, every value legal (-128 included), on the host
 * (bf_stokes_set_weights) or the device (bf_stokes_set_weights_device: what bf_calibrate_weights_device writes).  The handle's own
 * operand copy is not read: the stage gathers a compact copy.
 * Beam sample (exact integers, no conjugation):  n[u][f][c][k] = sum over a of v[u][f][c][a] * w[f][a][beam_k].
 * Stokes, with X = n[...][2j], Y = n[...][2j + 1] and a window n_int >= 1 that divides S (T = S / n_int outputs per unit), summed over
 * j in [t n_int, (t + 1) n_int), all exact int64:
 *   I = sum Xr^2 + Xi^2 + Yr^2 + Yi^2        Q = sum Xr^2 + Xi^2 - Yr^2 - Yi^2
 *   U = sum 2 (Xr Yr + Xi Yi) = 2 Re(X conj Y)      V = sum 2 (Xi Yr - Xr Yi) = 2 Im(X conj Y)
 * Layout [unit][t][freq][k]{I, Q, U, V}, four int64 per cell; bf_stokes_entries(cfg, K, n_int) = T * n_freq * K cells per unit (0 if
 * undefined).  n_int = n_avg is the detected stream's time resolution, n_int = 1 the voltages' own.
 * Bounds: n_pol == 2, n_ant % 4 == 0, n_ant <= 256 (|Xr|, |Xi| <= 2048 n_ant <= 2^19 fits the int32 accumulator, a term is <= 2^40),
 * K in 1 ... 16, every beam index in [0, n_beams), n_int dividing S; otherwise BF_ERR_INVALID with a message, and nothing is launched.
 * bf_stokes_create: n_int as above, max_in_flight result sets, each for the n_gemms_per_block units of a block.
 * bf_stokes_set_weights / _device: may be called again at any time, on any queue, and hold for the kernels issued after them; every
 *   write of the weights waits (on the device) for the write issued before it and for the pushes and bf_stokes_device kernels in flight.  The _device form is asynchronous on hip_stream; the host form returns when the copy has run.
 *   A selection of more beams than any before needs the stage drained (BF_ERR_STATE otherwise): the result sets grow with it.
 * bf_stokes_device: the kernel alone, n_units units at d_packed (16-byte aligned) -> d_out (device, n_units * entries * 4 int64, 16-byte
 *   aligned), asynchronously on hip_stream, behind the last gather.
 * bf_stokes_push: the kernel on hip_stream into the next result set, then -- on a queue of the stage's own, so hip_stream is held for
 *   the kernel only -- the copy to that set's pinned memory.  bf_stokes_push_block: the units [first_unit, first_unit + n_units) of ring
 *   slot `slot` (what bf_enqueue_block reads; any unit of it, 4-byte aligned at least) on compute queue stream_idx, behind what that queue holds.  A push before any weights, or
 *   with max_in_flight sets uncollected: BF_ERR_STATE; n_units > n_gemms_per_block: BF_ERR_INVALID; nothing is queued.
 * bf_stokes_collect waits for the OLDEST uncollected set and copies it to `out` (host; the size of ITS push: n_units * entries at the
 *   beams selected when it was pushed) and its units to *n_units (may be NULL); nothing pending: BF_ERR_STATE.  bf_stokes_pending: sets
 *   not yet collected.  A handle that goes first releases the device side; the stage then answers BF_ERR_STATE and can still be
 *   destroyed.  Every entry point leaves the caller's current device as it found it. */
#define BF_STOKES_MAX_BEAMS 16
typedef struct bf_stokes bf_stokes;
size_t bf_stokes_entries(const bf_config *cfg, int n_sel, int n_int);
int bf_stokes_create(bf_handle *h, int n_int, int max_in_flight, bf_stokes **out);
int bf_stokes_destroy(bf_stokes *s);
int bf_stokes_set_weights(bf_stokes *s, const int8_t *w_host, const int *beams, int n_sel);
int bf_stokes_set_weights_device(bf_stokes *s, const int8_t *d_w, const int *beams, int n_sel, void *hip_stream);
int bf_stokes_device(bf_stokes *s, const void *d_packed, int n_units, int64_t *d_out, void *hip_stream);
int bf_stokes_push(bf_stokes *s, const void *d_packed, int n_units, void *hip_stream);
int bf_stokes_push_block(bf_stokes *s, int stream_idx, int slot, int first_unit, int n_units);
int bf_stokes_collect(bf_stokes *s, int64_t *out, int *n_units);
int bf_stokes_pending(const bf_stokes *s);

/* a1 alone (expand_input, src/beamformer.cuh:66-109): nbytes packed bytes -> 2*nbytes int8 (re, im pairs in
 * order).  nbytes must be a multiple of 16, pointers 16-byte aligned. */
int bf_expand_device(bf_handle *h, const void *d_in, size_t nbytes, void *d_out, void *hip_stream);

/* a2 alone, for stage-level parity checks (the reference's d_C, src/beamformer.cu:470-477): one gemm-unit of
 * packed voltages -> complex float32 [freq][time][beam]{re,im} = (1/127) * W * V. */
int bf_gemm_device(bf_handle *h, const void *d_packed_unit, float *d_c, void *hip_stream);

/* a8 alone (the cublasSgemv of src/beamformer.cu:498-504): d_out_unit [output][freq][beam] -> d_ded [beam] = sum over freq
 * of output 0. */
int bf_dedisperse_device(bf_handle *h, const float *d_out_unit, float *d_ded, void *hip_stream);

/* Incoherent dedispersion beyond DM 0 (the reference stops at the DM-0 sum above,
 * src/beamformer.cu:498-504, and sketches the delay law in sandbox/Dispersion Theory.ipynb).  d_series: n_t consecutive beam-blocks [t][freq][beam] (the
 * detected stream is exactly that); d_delays: int32 [n_dm][freq] sample delays (dsabf::dm_delays / bfh_dm_delays);
 * d_out [n_dm][n_t_out][beam] = sum over freq, ascending, fp32, of d_series[t + delay][freq][beam]; rows outside [0, n_t)
 * contribute nothing, so size n_t_out = n_t - (largest delay) for complete sums.  Groups of 32 consecutive trials whose
 * delays, at every channel, span no more than ~100 samples (any fine DM ladder) run a kernel that fetches each window of
 * input rows once for the whole group (csrc/bf_dm_wide.hip); other groups -- coarse or non-monotonic ladders -- a kernel with
 * a window per thread; the result does not depend on which (one thread, one ascending-f sum either way).  Delays are read
 * on the device: nothing about them has to be known to the host. */
int bf_dedisperse_dm_device(bf_handle *h, const float *d_series, int n_t, const int32_t *d_delays, int n_dm, int n_t_out,
                            float *d_out, void *hip_stream);

/* ---- DM-trial dedispersion as a STAGE of the observation loop ---------------------------------
 * The reference collapses frequency INSIDE its loop, right behind each gemm-unit's detect (src/beamformer.cu:492-511: the
 * cublasSgemv of :498-504 and the copy of :506-510) -- at DM 0 only.  A bf_dm_stream does the same for a ladder of DM trials on
 * the detected stream as it is produced: the caller pushes the beam-blocks of every block it has beamformed ([row][freq][beam],
 * rows in time order: exactly what bf_enqueue_block leaves in bf_block_output_device, or bf_gather_detected in the freq-major
 * layout on the gather root), the stream keeps the last max_delay rows on the device in front of the next push, and every push
 * emits the output times that have just become complete:
 *   chunk [n_dm][n_t_out][beam], out[dm][t][b] = sum over f (ascending, fp32) of series[t + delay[dm][f]][f][b],
 *   t = first_t .. first_t + n_t_out - 1 counted from the first row ever pushed.
 * Chunks follow each other without gaps or overlap (first_t of a push = first_t + n_t_out of the one before); concatenated
 * along t they are BIT-IDENTICAL to one bf_dedisperse_dm_device call over the whole series (same kernels, same ascending-f
 * sum per output; the last max_delay times of a series are never complete, there as here).  n_t_out is 0 until more than
 * max_delay rows have been seen; the first chunk holds the times beyond them, every later one n_rows.
 *   delays: HOST int32 [n_dm][n_freq_total], all >= 0 (dsabf::dm_delays / bfh_dm_delays); n_freq_total = the channels of one
 *   pushed row (cfg.n_freq, or world * cfg.n_freq on a gather root); max_rows_per_push: the largest n_rows of a push
 *   (n_gemms_per_block * n_out_per_gemm for block launches).
 * bf_dm_stream_push is asynchronous on `hip_stream` (the queue that produced d_rows: bf_queue_stream); successive pushes are
 * ordered by the stream itself, whichever queues they are issued on: their chunks complete in push order -- but up to three
 * pushes issued on different queues RUN side by side (each in a chunk buffer and scratch of its own; a push waits for the rows
 * of the one before it, not for its end), so every push in flight needs a host_out of its own.  host_out (optional, pinned, room for n_dm * n_rows *
 * n_beams floats) receives the chunk; first_t / n_t_out are known to the host at once (pure arithmetic).  The device copy of
 * the most recent chunk: bf_dm_stream_output_device.  Destroy the stream before its handle (a handle that goes first releases the
 * stage's device memory; the stage then only answers BF_ERR_STATE and can still be destroyed).
 * Zero-copy feed (what run_observation uses): bf_dm_stream_reserve(s, n_rows, &d_dst, hip_stream) hands out the place of the next
 * n_rows rows INSIDE the stage's buffer, directly behind the carried-over window; the producer writes them there ON hip_stream (or
 * ordered behind it) -- bf_enqueue_block_to(h, q, ..., d_dst, ...), or bf_gather_detected(..., d_full = d_dst, stream) on a gather
 * root -- and bf_dm_stream_push(s, d_dst, n_rows, ...) then launches the kernels without moving a row (a push of rows that live
 * elsewhere copies them in first: one more read and write of every row).  One reservation at a time; it must be pushed as
 * reserved (same pointer, same n_rows).  The stage's buffer is a ring of max_delay + 3 max_rows_per_push rows whose memory is
 * mapped twice, back to back (hipMemCreate / hipMemMap): the delay window in front of a push is contiguous wherever it starts, and
 * no row is ever moved or read twice by anything but the dedispersion itself. */
typedef struct bf_dm_stream bf_dm_stream;
int bf_dm_stream_create(bf_handle *h, const int32_t *delays, int n_dm, int n_freq_total, int max_rows_per_push,
                        bf_dm_stream **out);
int bf_dm_stream_destroy(bf_dm_stream *s);
int bf_dm_stream_max_delay(const bf_dm_stream *s);
int bf_dm_stream_reserve(bf_dm_stream *s, int n_rows, float **d_dst, void *hip_stream);
int bf_dm_stream_push(bf_dm_stream *s, const float *d_rows, int n_rows, float *host_out, uint64_t *first_t, int *n_t_out,
                      void *hip_stream);
int bf_dm_stream_output_device(bf_dm_stream *s, float **d_out);

/* ---- Single-pulse search behind the DM stage (docs/SINGLE_PULSE.md) ----------------------------------------------------
 * The reference exists to "search for FRBs in real time" (README.md:11) and stops at a DM-0 collapse copied to the host
 * (src/beamformer.cu:498-510).  A bf_sps consumes the chunks [n_dm][n_t][beam] of a bf_dm_stream on the device and turns them
 * into "pulse at this time, trial, beam, width, S/N":
 *   boxcar sums of widths w_k = 2^k, k < n_widths <= 8, as the balanced pairwise tree S_0[t] = x[t],
 *   S_k[t] = S_{k-1}[t] + S_{k-1}[t - 2^(k-1)] (fp32, one rounding per add, no running sum), defined for t >= 2^k - 1 counted
 *   from the first sample the stage was given; the stage carries the last 2^(n_widths-1) - 1 samples of every (trial, beam) on
 *   the device, so the bits of S_k[t] do not depend on how the series was cut into pushes;
 *   per push and (k, trial, beam) one bf_sps_peak: the maximum of S_k over the push's times and the FIRST time attaining it,
 *   relative to the push's first time (value -inf, t_end -1: no time of the push qualifies) -- layout [n_widths][n_dm][n_beams];
 *   per push and (trial, beam) one bf_sps_stat: fp64 sum and sum of squares of x -- layout [n_dm][n_beams].
 * bf_sps_push is asynchronous on hip_stream; pushes of one stage are ordered by the stage itself, whichever queues they are
 * issued on (they share the carried samples).  Push j leaves its records in pinned set j % max_in_flight; a push whose set is
 * still uncollected returns BF_ERR_STATE.  bf_sps_collect waits for the oldest uncollected push, selects its candidates
 * (bf_sps_select over the statistics of the last baseline_pushes pushes, that one included) and returns them; max_out must be
 * at least n_dm * n_beams (BF_ERR_INVALID, nothing consumed); nothing pending: BF_ERR_STATE.  bf_sps_last_records: host pointers
 * to the raw records of the push just collected, valid until the next collect.  Lifetime as for a bf_dm_stream: a handle that
 * goes first releases the device memory, the stage then answers BF_ERR_STATE and can still be destroyed.
 * bf_sps_select is the selection as a pure host function (fp64, no GPU): totals[d][b] = the window's sums over n samples,
 *   mu = sum / n, sigma = sqrt(max(sumsq / n - mu^2, 0)); (d, b) is skipped if n < min_samples or sigma == 0;
 *   snr_k = (value_k - w_k mu) / (sigma sqrt(w_k)) for records with t_end >= 0; at most one candidate per (d, b): the k of the
 *   largest snr_k (lowest k on ties), if snr_k >= threshold; t_start = first_t + t_end - (w_k - 1), dm = dm_first + d;
 *   candidates leave in (d, b) order.  Returns BF_ERR_INVALID if they do not fit max_out.
 * bf_dm_stream_attach_search(dm, sps) (sps == NULL detaches): from then on every bf_dm_stream_push that emits n_t_out > 0 also
 * issues the search push for its chunk, on the same queue and before the chunk's buffer can be handed to a later push.  n_dm
 * must match and the stage's max_t_per_push must cover the DM stage's max_rows_per_push. */
typedef struct bf_sps bf_sps;
typedef struct bf_sps_peak {
    float value;
    int32_t t_end;
} bf_sps_peak;
typedef struct bf_sps_stat {
    double sum, sumsq;
} bf_sps_stat;
typedef struct bf_sps_candidate {
    uint64_t t_start; /* first sample of the boxcar, counted like first_t */
    int32_t dm;       /* global trial index */
    int32_t beam;
    int32_t width;    /* w_k */
    float peak;       /* S_k at the peak */
    double snr;
} bf_sps_candidate;
int bf_sps_create(bf_handle *h, int n_dm, int dm_first, int n_widths, int max_t_per_push, int max_in_flight, int baseline_pushes,
                  int min_samples, double threshold, bf_sps **out);
int bf_sps_destroy(bf_sps *s);
int bf_sps_push(bf_sps *s, const float *d_chunk, int n_t, uint64_t first_t, void *hip_stream);
int bf_sps_collect(bf_sps *s, bf_sps_candidate *out, size_t max_out, size_t *n_out);
int bf_sps_pending(const bf_sps *s);
int bf_sps_last_records(const bf_sps *s, const bf_sps_peak **peaks, const bf_sps_stat **stats, uint64_t *first_t, int *n_t);
int bf_sps_select(const bf_sps_peak *peaks, const bf_sps_stat *totals, uint64_t n, int n_widths, int n_dm, int n_beams,
                  uint64_t first_t, int dm_first, uint64_t min_samples, double threshold, bf_sps_candidate *out, size_t max_out,
                  size_t *n_out);
int bf_dm_stream_attach_search(bf_dm_stream *dm, bf_sps *sps);

/* ---- Conditioning the detected stream in front of the DM stage (docs/CONDITIONING.md) -----------------------------------
 * The reference collapses the detected powers as they come (src/beamformer.cu:498-510): no bandpass, no mask, no veto of
 * what arrives in every beam at DM 0.  A bf_cond rewrites pushed rows x[t][f][b] (fp32, the layout bf_dm_stream_push takes,
 * n_beams = the handle's) IN PLACE on the device; docs/CONDITIONING.md section 1 is the contract, to the bit:
 *   per push and (f, b): fp64 sum and sum of squares of the raw rows, in segments of 32 rows, ascending;
 *   over the last baseline_pushes pushes (1 .. 64, this one included, oldest first): mu, var = Q / n - mu mu, sigma;
 *     a cell is dead unless var > mu mu 2^-40;
 *   per channel: the means of mu and of max(var, 0) over the beams; mask[f] = the static mask, or a mean that is not > 0, or
 *     -- auto_threshold > 0 -- cv / cm^2 more than auto_threshold * 1.4826 median absolute deviations above the median of the
 *     channels still unmasked (high side only);
 *   y = (x - (float)mu) * (float)(1 / sigma), +0 in masked channels and dead cells;
 *   zero_dm: per (t, b) the mean of y over the unmasked channels (ascending fp32 sum * (float)(1 / n_good)) is subtracted
 *     from them.
 * The output depends on how the stream is cut into pushes (the statistics are per push), not on queues or launch shapes.
 * bf_cond_push is asynchronous on hip_stream; pushes of one stage are ordered by the stage itself, whichever queues they are
 * issued on (they share the window).  bf_cond_set_mask copies a host uint8 [n_freq_total] (nonzero = masked) that holds from
 * the next push on; bf_cond_mask_device: the device's uint8 mask[f] of the most recent push (valid behind that push).
 * BF_ERR_INVALID, with nothing launched: n_freq_total < 1, max_rows_per_push < 1, baseline_pushes outside 1 .. 64, a negative
 * or NaN auto_threshold, n_rows outside 1 .. max_rows_per_push, NULL pointers.  Lifetime as for a bf_sps: a handle that goes
 * first releases the device memory, the stage then answers BF_ERR_STATE and can still be destroyed.
 * bf_dm_stream_attach_conditioner(dm, c) (c == NULL detaches): from then on every bf_dm_stream_push conditions its new rows
 * where they lie in the DM stage's buffer -- behind the copy-in of rows that live elsewhere (the caller's source rows stay
 * raw), behind the rows of the push before it, and before its own rows are announced to the push behind it.  Same handle,
 * same n_freq_total, max_rows_per_push >= the DM stage's; attaching in mid-stream starts with an empty window.  Host copies
 * that bf_enqueue_block_to queued are in front of the push on the same queue: they carry the raw rows. */
typedef struct bf_cond bf_cond;
typedef struct bf_cond_options {
    int baseline_pushes;   /* 1 .. 64 */
    int zero_dm;           /* nonzero: subtract the per-(t, b) mean over the unmasked channels */
    double auto_threshold; /* 0: no automatic mask */
} bf_cond_options;
void bf_cond_default_options(bf_cond_options *o); /* 8, 1, 0.0 (src/beamformer.cu:498-510 has no such stage) */
int bf_cond_create(bf_handle *h, int n_freq_total, int max_rows_per_push, const bf_cond_options *o, bf_cond **out);
int bf_cond_destroy(bf_cond *c);
int bf_cond_set_mask(bf_cond *c, const uint8_t *host_mask);
int bf_cond_push(bf_cond *c, float *d_rows, int n_rows, void *hip_stream);
int bf_cond_mask_device(bf_cond *c, const uint8_t **d_mask);
int bf_dm_stream_attach_conditioner(bf_dm_stream *dm, bf_cond *c);

/* ---- Candidate events and dedispersed stamps behind the search (docs/EVENTS.md) -----------------------------------------
 * The reference stops at a DM-0 collapse copied to the host (src/beamformer.cu:498-510); the search behind the DM stage ends
 * in bf_sps_candidate records, one per (trial, beam) and push.  Two opt-in pieces turn those into "one thing happened" and
 * into the evidence for it; with neither in use nothing changes.
 * (1) bf_evt: a streaming friends-of-friends grouping of candidates -- host, fp64, no GPU, a pure function of the feeds.
 *   A candidate covers the closed interval [a0, a1] = [t_start, t_start + width - 1].  A and B are LINKED iff
 *   a0 <= b1 + t_tol, b0 <= a1 + t_tol and |dmA - dmB| <= dm_tol (beams play no part); a cluster is a connected component of
 *   the links.  bf_evt_feed takes the candidates of one collected push; next_t = that push's first_t + n_t, and every LATER
 *   candidate has t_start >= next_t - (max_width - 1).  A member is live while a1 + t_tol >= next_t - (max_width - 1); a
 *   cluster closes at the first feed after which it has no live member, and leaves as one bf_evt_event.  A cluster that is
 *   fed without pause stays one event.  bf_evt_flush closes everything; bf_evt_open: clusters still open.
 *   best: the member with the largest snr among beams other than ib_beam (ties: smaller t_start, dm, beam, width); only
 *   ib_beam members: the best of those and BF_EVT_IB_ONLY.  t_lo / t_hi: min a0 / max a1; dm_lo / dm_hi; n_members; n_beams:
 *   distinct beams other than ib_beam; snr_ib: largest snr of an ib_beam member, 0.0 without one.  BF_EVT_WIDE: n_beams >
 *   max_beams.  BF_EVT_INCOHERENT: ib_beam >= 0 and (IB_ONLY or snr_ib >= ib_ratio * best.snr).  The events of one call
 *   leave sorted by (best.t_start, best.dm, best.beam).  BF_ERR_INVALID: negative tolerances, max_width < 1, max_beams < 0,
 *   a NaN or negative ib_ratio, NULL pointers, max_out smaller than the events that close (nothing is consumed then).
 * (2) stamps: bf_dm_stream_create_history is bf_dm_stream_create with a ring of at least max_delay + 3 max_rows_per_push +
 *   history_rows rows (bf_dm_stream_create is that call with 0).  bf_dm_stream_history: rows [*oldest_row, *next_row) of the
 *   series are readable; next_row = rows pushed, oldest_row = max(0, pushed + reserved rows - cap_rows) (the producer of an
 *   outstanding reservation is already overwriting the oldest rows).  bf_dm_stream_cut, asynchronous on hip_stream:
 *     out[r][g][tau] = sum over f = g fbin .. g fbin + fbin - 1, ascending, of
 *                      ( sum over i = 0 .. tbin - 1, ascending, of x[t0 + tau tbin + i + delay[dm][f]][f][beam] ),
 *   fp32, [n_req][n_freq_total / fbin][n_tau] on the device, every sum sequential from its first element, one rounding per
 *   add; x is the row as it lies in the ring (conditioned behind an attached conditioner: what the search saw); dm is the
 *   LOCAL trial index.  Request r needs rows [t0, t0 + n_tau tbin + max_f delay[dm][f]).  status[r] (host, filled before the
 *   call returns): 0 cut, 1 a row is older than oldest_row, 2 a row is not pushed yet (1 wins where both hold); a request
 *   with a non-zero status launches nothing and its cells stay untouched.  A producer queued after a cut waits for it.
 *   bf_dm_stream_cut_host is the cut for a host consumer (run_observation): on a queue of the stage's own, into a device buffer of
 *   the stage, copied to host_out ([n_req][n_freq_total / fbin][n_tau], pinned) and waited for THERE; the caller's queues keep running.
 *   BF_ERR_INVALID, nothing launched: dm, beam or n_req out of range, n_tau, tbin or fbin < 1, fbin not dividing
 *   n_freq_total, NULL pointers.  BF_ERR_STATE: the linear fallback buffer (it keeps no history), or an orphaned stage. */
typedef struct bf_evt bf_evt;
typedef struct bf_evt_options {
    int32_t t_tol, dm_tol; /* samples, trials */
    int32_t max_width;     /* 2^(n_widths - 1) of the search that feeds it */
    int32_t max_beams;     /* more distinct beams than this: BF_EVT_WIDE */
    int32_t ib_beam;       /* the incoherent column, -1: none */
    double ib_ratio;
} bf_evt_options;
#define BF_EVT_IB_ONLY 1u
#define BF_EVT_WIDE 2u
#define BF_EVT_INCOHERENT 4u
typedef struct bf_evt_event {
    bf_sps_candidate best;
    uint64_t t_lo, t_hi;
    int32_t dm_lo, dm_hi;
    int32_t n_members, n_beams;
    double snr_ib;
    uint32_t flags;
} bf_evt_event;
typedef struct bf_stamp_request {
    uint64_t t0;
    int32_t dm; /* local trial index */
    int32_t beam;
} bf_stamp_request;
void bf_evt_default_options(bf_evt_options *o); /* 0, 1, 128, 4, -1, 0.5: design defaults (src/beamformer.cu:498-510 has no such step) */
int bf_evt_create(const bf_evt_options *o, bf_evt **out);
int bf_evt_destroy(bf_evt *e);
int bf_evt_feed(bf_evt *e, const bf_sps_candidate *cands, size_t n, uint64_t next_t, bf_evt_event *out, size_t max_out,
                size_t *n_out);
int bf_evt_flush(bf_evt *e, bf_evt_event *out, size_t max_out, size_t *n_out);
int bf_evt_open(const bf_evt *e);
int bf_dm_stream_create_history(bf_handle *h, const int32_t *delays, int n_dm, int n_freq_total, int max_rows_per_push,
                                int history_rows, bf_dm_stream **out);
int bf_dm_stream_history(const bf_dm_stream *s, uint64_t *oldest_row, uint64_t *next_row, uint64_t *cap_rows);
int bf_dm_stream_cut(bf_dm_stream *s, const bf_stamp_request *reqs, int n_req, int n_tau, int tbin, int fbin, float *d_out,
                     int32_t *status, void *hip_stream);
int bf_dm_stream_cut_host(bf_dm_stream *s, const bf_stamp_request *reqs, int n_req, int n_tau, int tbin, int fbin,
                          float *host_out, int32_t *status);

/* ---- Voltage history: dedispersed voltage cuts (docs/VOLTAGE_CUTS.md) -----------------------------------------------------
 * The reference keeps its packed voltages in a device ring of N_BLOCKS_ON_GPU blocks (src/beamformer.hh:124) that the H2D copy
 * of src/beamformer.cu:425-431 refills slot by slot: the voltages under a pulse are gone a few blocks after it.  A bf_vhist is
 * that ring generalised to a history of whole gemm-units deep enough to outlive the search, and a cut that leaves a burst as
 * DEDISPERSED gemm-units in the input layout, so that bf_stokes_device, bf_correlate_device, bf_sk_device and
 * bf_beamform_device run on it unchanged.  Opt-in: with no bf_vhist created nothing changes.  No arithmetic: bytes are moved.
 * Geometry (the handle's bf_config): a SAMPLE is the n_pol consecutive columns of one time step, B = n_pol n_ant bytes (a
 *   multiple of 4); a unit has S = n_out_per_gemm n_avg samples, [freq][S][n_pol][ant]: a channel of a unit is S B contiguous bytes.
 * bf_vhist_create: delays[n_dm][n_freq] int32 >= 0 in SAMPLES (host; copied to the device), n_freq the handle's; a device ring of
 *   cap_units >= history_units whole units, a plain allocation that wraps at unit granularity.  Sample s of the series, counted
 *   from the first unit ever pushed, lies in unit s / S, physical unit (s / S) mod cap_units, at sample s % S.
 * bf_vhist_push: n_units units at d_packed (device, 4-byte aligned) take the next unit positions, asynchronously on hip_stream (at
 *   most two copies, because of the wrap).  bf_vhist_push_block: the units [first_unit, first_unit + n_units) of ring slot `slot` of
 *   the handle (what bf_enqueue_block reads) on compute queue stream_idx, behind what that queue holds.  n_units > cap_units:
 *   BF_ERR_INVALID.  bf_vhist_history: units [*oldest_unit, *next_unit) are readable; next_unit = units pushed, oldest_unit =
 *   max(0, next_unit - cap_units).
 * bf_vhist_cut, asynchronous on hip_stream: d_out (device, 4-byte aligned) [n_req][n_units_out][freq][S][n_pol][ant] packed bytes,
 *     out[r][u][f][j][c][a] = v[t0_r + u S + j + delays[dm_r][f]][f][c][a];
 *   request r needs samples [t0, t0 + n_units_out S + max_f delays[dm][f]).  status[r] (host, filled before the call returns, by
 *   arithmetic alone): 0 cut, 1 a sample lies in a unit older than oldest_unit, 2 a sample is not pushed yet (1 wins where both
 *   hold); a request with a non-zero status launches nothing and its cells stay untouched.  16-byte accesses where B % 16 == 0 and
 *   d_out is 16-byte aligned, 4-byte ones otherwise.  bf_vhist_cut_host is the cut for a host consumer (run_observation): on a
 *   queue of the stage's own, into a device buffer of the stage, copied to host_out (the same layout, pinned) and waited for THERE.
 * Ordering: every push records an event behind its copy and behind the event of the push before it ("every unit < next_unit is in
 *   place"), so pushes may alternate between queues; a cut waits for the newest one and records its own behind the cut before it; a
 *   push queued after a cut waits for that before it writes.  While no cut has been issued a push waits for nothing new.
 * BF_ERR_INVALID, nothing launched: NULL pointers, n_dm < 1, a negative delay, history_units < 1, dm or n_req out of range,
 *   n_units_out < 1 (or n_freq n_units_out > 65535), d_out or d_packed not 4-byte aligned.  A handle that goes first releases the
 *   device side; the stage then answers BF_ERR_STATE and can still be destroyed.  Every entry point leaves the caller's current
 *   device as it found it.
 * bf_vhist_units_needed: pure host arithmetic, no device (docs/VOLTAGE_CUTS.md section 3): the history_units with which a consumer
 *   that cuts cut_units units around an event when it closes misses nothing -- rows of the detected stream = max_delay_rows +
 *   3 dm_rows (the DM stage's own) + cut_units n_out_per_gemm / 2 + t_tol + max_width + (n_buf + 1) dm_rows, as whole units
 *   (ceil(rows / n_out_per_gemm) + 1: a window may begin inside a unit), plus the n_gemms_per_block units of a block in flight.
 *   0 where undefined (NULL, a geometry or a dm_rows < 1, a negative argument, cut_units < 1). */
typedef struct bf_vhist bf_vhist;
typedef struct bf_vcut_request {
    uint64_t t0; /* samples, from the first unit ever pushed */
    int32_t dm;  /* row of the stage's delay table */
    int32_t pad;
} bf_vcut_request;
int bf_vhist_units_needed(const bf_config *cfg, int max_delay_rows, int dm_rows, int n_buf, int t_tol, int max_width,
                          int cut_units);
int bf_vhist_create(bf_handle *h, const int32_t *delays, int n_dm, int history_units, bf_vhist **out);
int bf_vhist_destroy(bf_vhist *v);
int bf_vhist_push(bf_vhist *v, const void *d_packed, int n_units, void *hip_stream);
int bf_vhist_push_block(bf_vhist *v, int stream_idx, int slot, int first_unit, int n_units);
int bf_vhist_history(const bf_vhist *v, uint64_t *oldest_unit, uint64_t *next_unit, uint64_t *cap_units);
int bf_vhist_cut(bf_vhist *v, const bf_vcut_request *reqs, int n_req, int n_units_out, void *d_out, int32_t *status,
                 void *hip_stream);
int bf_vhist_cut_host(bf_vhist *v, const bf_vcut_request *reqs, int n_req, int n_units_out, void *host_out, int32_t *status);

/* ---- Coherent dedispersion: beam voltages and an FFT chirp filter (docs/COHERENT_DEDISPERSION.md) -----------------------------
 * bf_vhist_cut aligns the channels of a burst by whole samples and bf_stokes_device forms Stokes parameters at every voltage
 * sample, but the dispersion INSIDE a channel (tens of samples at the DMs of the search) stays.  The reference holds the beam
 * voltages only as the GEMM's scratch d_C (src/beamformer.cu:178) and squares them away at once (src/beamformer.cuh:149-152), so
 * it has nothing to dedisperse coherently.  Two pieces remove the smear; both are opt-in, and with neither used nothing changes.
 * bf_stokes_voltages_device: the tied-array beam samples the Stokes kernel forms, kept instead of multiplied out.  n_units units
 *   at d_packed (16-byte aligned, as for bf_stokes_device) -> d_out (device, 8-byte aligned) [freq][k][pol][n_units S]{re, im}
 *   float32, S = n_out_per_gemm n_avg: time runs across the units, so a series is contiguous.  The values are the exact integers
 *   n[u][f][2 j + pol][k] of docs/STOKES.md section 1 (|re|, |im| <= 2^19).  Ordered exactly as bf_stokes_device (behind the last
 *   write of the weights; a later write waits for it).  bf_stokes_voltage_entries(cfg, K) = n_freq K 2 S complex samples per unit
 *   (0 if undefined).  BF_ERR_INVALID, nothing launched: NULL pointers, n_units < 1, misalignment, n_units S >= 2^31;
 *   BF_ERR_STATE before any weights.
 * bf_cdd: the chirp filter.  Input x[chan][k][pol][n]{re, im} float32 (device, 8-byte aligned), n in [0, n_time) -- the layout
 *   above, from anywhere.  bf_cdd_create: n_chan >= 1, an FFT length n_fft = 2^m with 6 <= m <= 12, an edge 0 <= n_edge <=
 *   n_fft / 4, and a HOST table chirp[n_chan][n_fft]{re, im} float32 that is copied to the device.  With V = n_fft - 2 n_edge,
 *   segment g = 0 ... ceil(n_time / V) - 1 reads the samples [g V - n_edge, g V - n_edge + n_fft), zero outside [0, n_time), and
 *     y_g = IDFT( DFT(segment) * chirp[chan] )   (no other scale: the 1 / n_fft belongs to the table),
 *   output sample g V + i = y_g[n_edge + i] for 0 <= i < V, g V + i < n_time (overlap-save).  float32 throughout, every operation
 *   rounded on its own, in ONE operation order (docs section 2) that does not depend on K, n_chan, n_time or the segment; the
 *   twiddle factors are a table computed on the host in double and rounded.
 * bf_cdd_voltages_device: d_out in the input's shape.  bf_cdd_stokes_device: d_out[t][chan][k]{I, Q, U, V} float32, t < n_time /
 *   n_int; per sample px = xr xr + xi xi, py likewise, uu = xr yr + xi yi, vv = xi yr - xr yi, I = px + py, Q = px - py, U = 2 uu,
 *   V = 2 vv, summed over the window in ascending order of the samples (the first term is not added to a zero).  n_int must divide
 *   both V and n_time.  Both are asynchronous on hip_stream and write every cell once.
 * bf_cdd_set_chirp: waits for the stage's kernels in flight, uploads, returns when the table is in place.
 * BF_ERR_INVALID, nothing launched: NULL pointers, n_fft not one of the seven lengths, n_edge out of range, K < 1, n_time < 1 or
 *   >= 2^31, n_int < 1 or not dividing V and n_time, d_in or d_out not 8-byte aligned, more than 2^31 - 1 (segment, channel, beam)
 *   workgroups.  A handle that goes first: BF_ERR_STATE, and the stage can still be destroyed.
 * Host helpers, plain double, no device, with the dispersion constant 4.15 ms GHz^2 of dm_delays:
 *   bf_cdd_sweep_samples(dm, f_ghz, bw_mhz) = 4.15e3 dm ((f - bw/2000)^-2 - (f + bw/2000)^-2) bw_mhz: the sweep across a channel of
 *     width bw_mhz centred on f_ghz, in samples of 1 / bw_mhz microseconds.
 *   bf_cdd_edge: the largest ceil(sweep) over the channels (negative: an error code).
 *   bf_cdd_chirp fills out[n_chan][n_fft]{re, im}: for bin j, nu = sideband (j < N/2 ? j : j - N) bw_mhz / N MHz, F = 1000 f MHz,
 *     phi = 2 pi 4.15e9 dm nu^2 / (F^2 (F + nu)), out = (cos phi, sin phi) / N rounded to float32.  sideband = +1 or -1: whether
 *     baseband frequency rises with sky frequency. */
typedef struct bf_cdd bf_cdd;
size_t bf_stokes_voltage_entries(const bf_config *cfg, int n_sel);
int bf_stokes_voltages_device(bf_stokes *s, const void *d_packed, int n_units, void *d_out, void *hip_stream);
double bf_cdd_sweep_samples(double dm, double f_ghz, double bw_mhz);
int bf_cdd_edge(double dm, const double *freq_ghz, int n_chan, double bw_mhz);
int bf_cdd_chirp(double dm, const double *freq_ghz, int n_chan, double bw_mhz, int sideband, int n_fft, float *out);
int bf_cdd_create(bf_handle *h, int n_chan, int n_fft, int n_edge, const float *chirp, bf_cdd **out);
int bf_cdd_destroy(bf_cdd *c);
int bf_cdd_set_chirp(bf_cdd *c, const float *chirp);
int bf_cdd_voltages_device(bf_cdd *c, const void *d_in, int K, int64_t n_time, void *d_out, void *hip_stream);
int bf_cdd_stokes_device(bf_cdd *c, const void *d_in, int K, int64_t n_time, int n_int, void *d_out, void *hip_stream);

/* ---- Faraday synthesis: rotation-measure spectra and peaks of Stokes beams (docs/FARADAY.md) -----------------------------------
 * The reference squares its beam voltages away at once (src/beamformer.cuh:149-152) and keeps total power only, so it has no linear
 * polarisation to derotate; behind bf_cdd_stokes_device this project has Q and U per channel.  A bf_rm evaluates
 *     F(phi_p) = sum_c wn_c (Q_c + i U_c) exp(-2 i phi_p (lambda_c^2 - lambda_0^2))
 * for every row and follow-up beam on a grid of Faraday depths and finds the peak of |F|^2.  Opt-in: with no stage nothing changes.
 * Input s[t][chan][k]{I, Q, U, V} float32 (device), t < n_rows, k < K -- what bf_cdd_stokes_device writes, from anywhere; optionally a
 *   baseline base[chan][k]{I, Q, U, V} float32 (device).  Finite values; NaN and Inf are outside the contract but fault nothing.
 * Tables, HOST arrays copied to the device: rot[p][c]{r, s} float32 = wn_c (cos, -sin)(2 phi_p (lambda_c^2 - lambda_0^2)) and
 *   wn[c] float32 = w_c / sum w  (bf_rm_table, or any table).  No sine or cosine runs on the device.
 * ONE operation order, whatever K, n_rows and the launch shape (docs section 2), float32:
 *   per cell q = Q - base.Q, u = U - base.U, i = I - base.I (one subtraction each; none without a baseline);
 *   F_re: acc = fmaf(q_c, r_pc, acc), acc = fmaf(u_c, -s_pc, acc) over ascending c from +0; F_im: fmaf(q_c, s_pc, acc), fmaf(u_c, r_pc, acc);
 *   pow[p] = F_re F_re + F_im F_im (two products, one addition, each rounded);  isum: acc = fmaf(i_c, wn[c], acc) from +0;
 *   the peak: the smallest p whose pow[p] is the maximum.
 * bf_rm_device, asynchronous on hip_stream, every cell written once; either output may be NULL, not both:
 *   d_spec[t][k][p]{re, im} float32;  d_peaks[t][k]: one bf_rm_peak (32 bytes), pow_lo / pow_hi the powers at p -+ 1 (0 outside the
 *   grid), re / im = F at the peak.  With d_spec NULL the spectrum never goes to memory.
 * bf_rm_set_table: waits for the stage's kernels in flight, uploads, returns when the table is in place.
 * BF_ERR_INVALID, nothing launched: NULL stage, handle or table, n_chan or n_phi outside 1 ... 4096, K < 1, n_rows < 1 or
 *   n_rows K >= 2^31, both outputs NULL, a device pointer not 8-byte aligned (16-byte aligned ones take 16-byte accesses).  A handle
 *   that goes first: BF_ERR_STATE, and the stage can still be destroyed.  The caller's current device is left as found.
 * Host helpers, plain double, no device (w_c >= 0, a zero masks a channel):
 *   bf_rm_lambda2(f_ghz) = (0.299792458 / f_ghz)^2 m^2;  lambda_0^2 = sum w_c lambda_c^2 / sum w_c.
 *   bf_rm_resolution: fwhm = 2 sqrt 3 / (max - min lambda^2 of the unmasked channels), phi_max = sqrt 3 / the largest |lambda^2
 *     step| between neighbouring channels of the list (Brentjens & de Bruyn 2005, eqs. 61 and 63).
 *   bf_rm_table fills rot[n_phi][n_chan]{r, s} and wn[n_chan] for phi_p = phi0 + p dphi, and *lambda0_2 (may be NULL).
 *   bf_rm_rmsf: out[n_phi]{re, im} double = sum_c wn_c exp(-2 i phi_p (lambda_c^2 - lambda_0^2)).
 *   bf_rm_refine, per record: delta = 0.5 (lo - hi) / (lo - 2 pk + hi) (0 at a grid end or a zero denominator), rm = phi0 +
 *     (p + delta) dphi, pa = 0.5 atan2(im, re) - rm lambda_0^2 wrapped into [-pi/2, pi/2), lin = sqrt(pk), frac = lin / isum
 *     (0 where isum <= 0). */
typedef struct bf_rm bf_rm;
typedef struct bf_rm_peak {
    int32_t p;
    float pow_lo, pow_pk, pow_hi, re, im, isum;
    int32_t zero;
} bf_rm_peak;
typedef struct bf_rm_fit {
    double rm, pa, lin, frac;
} bf_rm_fit;
double bf_rm_lambda2(double f_ghz);
int bf_rm_resolution(const double *freq_ghz, const double *w, int n_chan, double *fwhm, double *phi_max);
int bf_rm_table(const double *freq_ghz, const double *w, int n_chan, double phi0, double dphi, int n_phi, float *rot, float *wn,
                double *lambda0_2);
int bf_rm_rmsf(const double *freq_ghz, const double *w, int n_chan, double phi0, double dphi, int n_phi, double *out);
int bf_rm_refine(const bf_rm_peak *peaks, size_t n, double phi0, double dphi, int n_phi, double lambda0_2, bf_rm_fit *fits);
int bf_rm_create(bf_handle *h, int n_chan, int n_phi, const float *rot, const float *wn, bf_rm **out);
int bf_rm_destroy(bf_rm *s);
int bf_rm_set_table(bf_rm *s, const float *rot, const float *wn);
int bf_rm_device(bf_rm *s, const void *d_stokes, int K, int64_t n_rows, const void *d_base, void *d_spec, void *d_peaks,
                 void *hip_stream);

/* ---- Pulsar folding: phase-binned profiles of every beam (docs/PULSAR_FOLDING.md) -------------------------------------------
 * The reference stops at a DM-0 collapse copied to the host (src/beamformer.cu:498-510) and keeps nothing across blocks; the
 * search behind the DM stage looks at one push at a time.  A bf_psr integrates the detected rows x[row][freq][beam] (fp32, the
 * layout bf_dm_stream_push takes, n_beams = the handle's) at a KNOWN spin frequency and dispersion, for all beams at once;
 * docs/PULSAR_FOLDING.md section 1 is the contract, to the bit:
 *   phase model, integers only (turns in units of 2^-64, per row): rows r count from the first row the stage was given; for
 *     pulsar k, channel f:  n = r - epoch_row - delay[k][f],
 *     phase = phase0 + (uint64)n dphase + (uint64)(n (n - 1) / 2) (uint64)ddphase  (mod 2^64),  bin = ((phase >> 32) n_bins) >> 32;
 *   delay: HOST int32 [n_psr][n_freq_total], all >= 0, sign and meaning of one row of dsabf::dm_delays / bfh_dm_delays;
 *   profile[k][f][bin][beam] (fp64): acc = acc + (double)x[r][f][beam] over the rows of that bin IN ASCENDING ROW ORDER, from +0.0
 *     at the last dump; hits[k][f][bin] (uint64): the number of those rows.  No fp32 sums, no atomics, no partial sums: the
 *     bits do not depend on how the series is cut into pushes, on queues or on launch shapes.
 *   n_bins 2 .. BF_PSR_MAX_BINS, n_psr 1 .. BF_PSR_MAX_PULSARS (they share one read of the rows).
 * bf_psr_entries: the doubles of a profile, n_psr * n_freq_total * n_bins * n_beams (hits: that / n_beams); 0 out of range.
 * bf_psr_push is asynchronous on hip_stream; pushes and dumps of one stage are ordered by the stage itself, whichever queues
 *   they are issued on (they share the accumulators).  A push that would reach |n| >= 2^31 is refused: re-anchor epoch_row.
 * bf_psr_dump snapshots profile and hits into pinned set j % max_in_flight and zeroes the accumulators, on a queue of the
 *   stage's own, behind the pushes issued before it (hip_stream is not held); a dump whose set is uncollected: BF_ERR_STATE.
 * bf_psr_collect waits for the OLDEST uncollected dump and copies it to profile / hits (host) and the integration's first row and
 *   row count to *first_row / *n_rows (may be NULL); nothing pending: BF_ERR_STATE.  bf_psr_pending: dumps not yet collected.
 * BF_ERR_INVALID, with nothing launched: n_rows outside 1 .. max_rows_per_push, NULL pointers, n_bins, n_psr or
 *   max_in_flight out of range, a negative delay, the |n| limit.  Lifetime as for a bf_cond: a handle that goes first releases
 *   the device memory, the stage then answers BF_ERR_STATE and can still be destroyed.
 * bf_psr_model_from_spin (host, fp64, no GPU): x = f0 row_seconds; dphase = (uint64)ldexp(x - floor(x), 64) (a fraction that
 *   rounds to 1.0: 0); ddphase = (int64)nearbyint(ldexp((f1 row_seconds) row_seconds, 64)), refused at |.| >= 2^62; phase0 from
 *   phase0_turns like dphase; then dphase += (uint64)(ddphase >> 1), so that the phase follows f0 t + f1 t^2 / 2.  NaN, infinite
 *   or row_seconds <= 0: BF_ERR_INVALID.
 * bf_psr_beam_snr (host, fp64, no GPU), for one pulsar's profile [f][bin][beam] and hits [f][bin], per beam: over the channels
 *   with chan_mask[f] == 0 (NULL: all), ascending: S[j] = sum profile, H[j] = sum hits; m[j] = S[j] / H[j] on the bins with H[j] > 0;
 *   fewer than 4 such bins: snr 0, peak_bin -1; med = median of m (even count: (a + b) 0.5), sigma = 1.4826 median |m - med|;
 *   sigma not > 0: snr 0, peak_bin -1; else snr = (max m - med) / sigma and peak_bin = the first bin that attains the maximum.
 * bf_dm_stream_attach_folder(dm, p) (p == NULL detaches): from then on every bf_dm_stream_push also folds its new rows where they
 *   lie in the DM stage's buffer, on the push's queue -- behind an attached conditioner (it folds what is dedispersed), and before
 *   the ring can hand those rows' place to a later push.  Same handle, same n_freq_total, max_rows_per_push >= the DM stage's. */
#define BF_PSR_MAX_PULSARS 4
#define BF_PSR_MAX_BINS 4096
typedef struct bf_psr bf_psr;
typedef struct bf_psr_model {
    uint64_t phase0, dphase; /* turns in units of 2^-64, per row of the detected stream */
    int64_t ddphase;
    int64_t epoch_row;       /* the row (counted from the first row pushed) at which phase = phase0 */
} bf_psr_model;
int bf_psr_model_from_spin(double f0_hz, double f1_hz_s, double phase0_turns, double row_seconds, int64_t epoch_row,
                           bf_psr_model *model);
size_t bf_psr_entries(int n_psr, int n_freq_total, int n_bins, int n_beams);
int bf_psr_create(bf_handle *h, int n_freq_total, int max_rows_per_push, int n_bins, const bf_psr_model *models,
                  const int32_t *delays, int n_psr, int max_in_flight, bf_psr **out);
int bf_psr_destroy(bf_psr *p);
int bf_psr_push(bf_psr *p, const float *d_rows, int n_rows, void *hip_stream);
int bf_psr_dump(bf_psr *p, void *hip_stream);
int bf_psr_collect(bf_psr *p, double *profile, uint64_t *hits, uint64_t *first_row, uint64_t *n_rows);
int bf_psr_pending(const bf_psr *p);
int bf_psr_beam_snr(const double *profile_k, const uint64_t *hits_k, int n_freq_total, int n_bins, int n_beams,
                    const uint8_t *chan_mask, double *snr, int32_t *peak_bin);
int bf_dm_stream_attach_folder(bf_dm_stream *dm, bf_psr *p);

/* ---- Periodicity search: the Fast Folding Algorithm behind the DM trials (docs/PERIODICITY.md) ------------------------------
 * The reference has no search of any kind (its output is the detected stream and a DM-0 collapse, src/beamformer.cu:498-510).
 * A bf_ffa consumes the chunks x[n_dm][n_t][n_beams] (fp32, contiguous, 16-byte aligned, n_beams = the handle's, n_beams % 4 == 0)
 * that bf_dm_stream_push emits, and finds periodic signals nobody predicted; docs/PERIODICITY.md section 1 is the contract, to the bit:
 *   decimation: y[u] = ((x[u tdec] + x[u tdec + 1]) + ...) + x[u tdec + tdec - 1], fp32, ascending time, the first term as it is;
 *     a push that ends inside a group carries the running value and the count over.  tdec 1 .. BF_FFA_MAX_DEC.
 *   segments: consecutive n_seg decimated samples, no overlap; n_seg <= BF_FFA_MAX_SEG.
 *   octaves o < n_oct (1 .. BF_FFA_MAX_OCT): y_0 = y, y_{o+1}[u] = y_o[2u] + y_o[2u + 1], L_o = n_seg >> o; n_seg % 2^(n_oct-1) == 0.
 *   fold, per octave and base period p_lo <= p < p_hi (BF_FFA_MIN_PERIOD <= p_lo < p_hi <= BF_FFA_MAX_PERIOD, samples of the
 *     octave): M = bf_ffa_rows_of(L_o, p) = the largest power of two <= L_o / p, M >= 2 required for every (o, p); the first M p
 *     samples are M rows of p bins, each a group of one row; a merge of two adjacent groups A (earlier), B (later) of g rows:
 *       out[i][j] = A[i >> 1][j] + B[i >> 1][(j + ((i + 1) >> 1)) mod p],   i < 2g,   fp32, A's term the left operand,
 *     log2 M times.  Row i of the last group is the profile at period p + i / (M - 1) samples.
 *   circular boxcars per profile P_i, widths 2^k, k < n_widths (1 .. BF_FFA_MAX_WIDTHS, 2^(n_widths-1) <= p_lo / 2):
 *     C_0 = P_i,  C_k[j] = C_{k-1}[j] + C_{k-1}[(j + 2^(k-1)) mod p].
 *   per segment and (o, p, k, trial, beam) one bf_ffa_peak: the maximum of C_k over (i, j), the smallest i attaining it, the
 *     smallest j at that i -- layout [n_oct][p_hi - p_lo][n_widths][n_dm][n_beams].  A (trial, beam) column with no finite sample in
 *     the segment: value unspecified, shift < M and bin < p all the same, never a candidate; no other column changes;
 *   per segment and (trial, beam) one bf_ffa_stat: fp64 sum and sum of squares of the n_seg samples of y_0 (order free).
 *   Nothing depends on how the series is cut into pushes, on queues or on launch shapes.
 * bf_ffa_entries: peak records of a segment, n_oct (p_hi - p_lo) n_widths n_dm n_beams (statistics: n_dm n_beams); 0 out of range.
 * bf_ffa_push is asynchronous on hip_stream; first_t is the row of the chunk's first time (bf_dm_stream_push's *first_t).  Pushes
 *   of one stage are ordered by the stage itself, whichever queues they come on.  A push may complete none, one or several
 *   segments; each is searched in order on the push's queue, its records go to result set segment % max_in_flight and are copied
 *   to pinned memory on a queue of the stage's own.  A push whose completed segments would not all find a free set -- uncollected
 *   segments + the push's > max_in_flight -- is refused with BF_ERR_STATE before anything is queued.
 * bf_ffa_collect waits for the OLDEST uncollected segment and selects its candidates (bf_ffa_select); max_out >= n_dm * n_beams
 *   (BF_ERR_INVALID, nothing consumed); nothing pending: BF_ERR_STATE.  bf_ffa_pending: segments searched and not yet collected.
 * bf_ffa_last_records: host pointers to the records of the segment last collected, valid until the next collect or destroy.
 * bf_ffa_select (host, fp64, no GPU, no contraction), per (trial, beam): mu = sum / n_seg, sigma = sqrt(max(sumsq / n_seg - mu mu, 0)),
 *   skipped at sigma == 0; per record w = 2^k, snr = (value - (w M) (2^o mu)) / ((sigma sqrt(2^o)) sqrt(w M)); at most one
 *   candidate: the largest snr (ties: lowest o, then p, then k), if >= threshold; period_rows = tdec 2^o (p + shift / (M - 1)) in
 *   input samples; candidates leave in (trial, beam) order.
 * BF_ERR_INVALID, with nothing launched: any bound above, NULL pointers, a misaligned chunk, n_t outside 1 .. max_t_per_push,
 *   n_beams % 4 != 0, n_dm outside 1 .. 65535, max_in_flight < 1, a NaN threshold.  Lifetime as for a bf_sps.
 * bf_dm_stream_attach_periodicity(dm, s) (s == NULL detaches): from then on every bf_dm_stream_push that emits a chunk also pushes
 *   it into s, behind the dedispersion kernels (and an attached search stage) and before the push's `done` event; a push the
 *   stage would refuse is refused by bf_dm_stream_push before it queues anything.  Same handle, same n_dm, max_t_per_push >= the
 *   DM stage's max_rows_per_push.
 * bf_ffa_set_detrend(s, blk, win): red-noise removal in front of the fold (docs/PERIODICITY.md section 1a, to the bit).  Every complete
 *   segment y_0 of every (trial, beam), after the decimation and before the octaves, the fold and the statistics, loses a trend:
 *   the fp32 means of its nb = n_seg / blk blocks (a left fold times 2^-log2(blk)), their running LOWER median over win blocks
 *   (windows truncated at the ends; the order of the keys bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000), so -0 < +0; a pure
 *   selection), and through the block centres the piecewise linear r[c0] + a (r[c0 + 1] - r[c0]) in three fp32 roundings, constant
 *   outside the first and last centre; y'[u] = y[u] - trend[u] in place.  Records and statistics are those of y'.  blk a power of
 *   two 1 .. BF_FFA_MAX_DETREND_BLK that divides n_seg, win odd 1 .. BF_FFA_MAX_DETREND_WIN: BF_ERR_INVALID otherwise, nothing
 *   allocated or launched; blk == 0 switches it off (the default: nothing is launched and no byte of anything changes).  Legal before
 *   the first push only (BF_ERR_STATE afterwards, and for an orphaned stage).  bf_ffa_detrend reads the two back.  A column with a
 *   non-finite sample in the segment: records and statistics unspecified, shift < M and bin < p all the same, no other column changes.
 * bf_ffa_sift (host, fp64, pure, no GPU): groups candidates (what bf_ffa_collect gave, of any number of segments) that are one source
 *   seen in neighbouring trials, several beams and at harmonically related periods.  Candidates are taken in descending snr (ties:
 *   the lower index); each is tested against the existing group heads in the order they were created and joins the FIRST it
 *   matches, else it becomes a head (links are to heads only).  A match: equal first_row and n_rows, |dm - head.dm| <= dm_tol, and
 *   some a, then b, both ascending in 1 .. max_harm, with fabs((period_rows b) / (head.period_rows a) - 1.0) <= tol; the first
 *   matching (a, b) other than (1, 1) counts in n_harmonic.  Groups leave in creation order.  BF_ERR_INVALID with *n_out = 0 and
 *   nothing written: tol outside [0, 1) or NaN, max_harm outside 1 .. BF_FFA_MAX_HARM, dm_tol < 0, a NaN snr, a period_rows that
 *   is not > 0, more groups than max_out, NULL pointers with n > 0.  n == 0: BF_OK, no group. */
#define BF_FFA_MAX_DEC 256
#define BF_FFA_MAX_SEG 16384
#define BF_FFA_MAX_OCT 6
#define BF_FFA_MAX_WIDTHS 6
#define BF_FFA_MIN_PERIOD 8
#define BF_FFA_MAX_PERIOD 512
#define BF_FFA_MAX_DETREND_BLK 256
#define BF_FFA_MAX_DETREND_WIN 129
#define BF_FFA_MAX_HARM 16
typedef struct bf_ffa bf_ffa;
typedef struct bf_ffa_peak {
    float value;
    uint16_t shift; /* the row i of the last group: period p + i / (M - 1) */
    uint16_t bin;   /* the first bin j of the boxcar */
} bf_ffa_peak;
typedef struct bf_ffa_stat {
    double sum, sumsq;
} bf_ffa_stat;
typedef struct bf_ffa_candidate {
    uint64_t first_row, n_rows; /* the segment, in input samples (rows of the detected stream) */
    double period_rows;
    int32_t dm, beam, octave, p, shift, bin, width;
    double snr;
    float value;
} bf_ffa_candidate;
size_t bf_ffa_entries(int n_oct, int p_lo, int p_hi, int n_widths, int n_dm, int n_beams);
int bf_ffa_rows_of(int len, int p);
int bf_ffa_create(bf_handle *h, int n_dm, int dm_first, int tdec, int n_seg, int n_oct, int p_lo, int p_hi, int n_widths,
                  int max_t_per_push, int max_in_flight, double threshold, bf_ffa **out);
int bf_ffa_destroy(bf_ffa *s);
int bf_ffa_push(bf_ffa *s, const float *d_chunk, int n_t, uint64_t first_t, void *hip_stream);
int bf_ffa_collect(bf_ffa *s, bf_ffa_candidate *out, size_t max_out, size_t *n_out);
int bf_ffa_pending(const bf_ffa *s);
int bf_ffa_last_records(const bf_ffa *s, const bf_ffa_peak **peaks, const bf_ffa_stat **stats, uint64_t *first_row,
                        uint64_t *n_rows);
int bf_ffa_select(const bf_ffa_peak *peaks, const bf_ffa_stat *stats, int tdec, int n_seg, int n_oct, int p_lo, int p_hi,
                  int n_widths, int n_dm, int n_beams, uint64_t first_row, uint64_t n_rows, int dm_first, double threshold,
                  bf_ffa_candidate *out, size_t max_out, size_t *n_out);
int bf_dm_stream_attach_periodicity(bf_dm_stream *dm, bf_ffa *s);
typedef struct bf_ffa_group {
    bf_ffa_candidate head;        /* the member with the largest snr */
    int32_t n_members, n_beams;   /* head included; distinct beams among the members */
    int32_t dm_lo, dm_hi;         /* extent in trials */
    int32_t n_harmonic, reserved; /* members that joined at (a, b) != (1, 1); 0 */
} bf_ffa_group;
int bf_ffa_set_detrend(bf_ffa *s, int blk, int win);
int bf_ffa_detrend(const bf_ffa *s, int *blk, int *win);
int bf_ffa_sift(const bf_ffa_candidate *in, size_t n, double tol, int max_harm, int dm_tol, bf_ffa_group *out, size_t max_out,
                size_t *n_out);

/* ---- Pulse injection: test bursts and pulse trains in front of the DM stage (docs/INJECTION.md) -----------------------------
 * The reference is there to "search for FRBs in real time" (README.md:11) and ends at a DM-0 collapse (src/beamformer.cu:498-510);
 * nothing in it, and until here nothing in this library, puts a dispersed pulse into the stream to show that the chain finds it.
 * A bf_inj adds synthetic pulses to the detected rows x[row][freq][beam] (fp32, the layout bf_dm_stream_push takes, n_beams = the
 * handle's, n_beams % 4 == 0) in place; docs/INJECTION.md section 1 is the contract, to the bit:
 *   rows r count from the first row the stage is given; bf_inj_next_row: the rows applied so far (host arithmetic).
 *   burst (t0 >= 0, W 1 .. max_width, HOST tables delay int32 [n_freq_total] >= 0 -- one row of dsabf::dm_delays / bfh_dm_delays --,
 *     profile float [n_freq_total][W], response float [n_beams]): every cell with i = r - t0 - delay[f], 0 <= i < W, becomes
 *     x = fl(x + fl(profile[f][i] response[b])): one fp32 multiply, one fp32 add, never contracted, a zero response included.
 *   train (a bf_psr_model, n_bins 2 .. min(max_width, BF_PSR_MAX_BINS), profile [n_freq_total][n_bins]): for first_row <= r <
 *     first_row + n_rows (n_rows == UINT64_MAX: until the end)  x = fl(x + fl(profile[f][bin(r, f)] response[b])), bin the folder's
 *     formula operation for operation (n = r - epoch_row - delay[f]); at most BF_INJ_MAX_TRAINS alive; an apply that would reach
 *     |n| >= 2^31 on a covered row is refused as bf_psr_push refuses it.
 *   a cell outside every window is NOT WRITTEN.  Order at a cell: the bursts that cover it in ascending id, then the trains in
 *     ascending id; *id (may be NULL) counts adds of either kind from 0.  The bits do not depend on how the series is cut into
 *     applies, on queues or on launch shapes.
 *   lifetime of a pulse: an add whose first touched row (t0 + min delay; first_row) lies before bf_inj_next_row is refused with
 *     BF_ERR_STATE, as is one beyond max_pulses (1 .. BF_INJ_MAX_PULSES) live pulses or BF_INJ_MAX_TRAINS live trains; a burst is
 *     spent once next_row > t0 + max delay + W - 1, a train once its last row is behind next_row, and gives its slot back.  An add may
 *     be called while earlier applies still run on the device: it never writes memory a queued kernel may read.
 * bf_inj_apply takes rows [next_row, next_row + n_rows) at d_rows (16-byte aligned), asynchronously on hip_stream; the stage keeps no
 *   device state from one apply to the next, so applies on different queues need no ordering among themselves.  An apply that no
 *   live pulse overlaps launches nothing and reads nothing; one that bursts overlap reads and writes only rows inside some window.
 *   bf_inj_launches: the kernels launched so far.  An attached injector is applied by the DM stage: bf_inj_apply then answers BF_ERR_STATE.
 * bf_dm_stream_attach_injector(dm, inj) (NULL detaches): from then on every bf_dm_stream_push adds the live pulses to its new rows
 *   where they lie in the DM stage's buffer, behind the copy-in and in front of an attached conditioner -- the caller's source rows
 *   stay raw, everything downstream sees the pulses.  Same handle, same n_freq_total, max_rows_per_push >= the DM stage's, and
 *   bf_inj_next_row == the rows the DM stage has been pushed (else BF_ERR_STATE).
 * BF_ERR_INVALID, with nothing allocated or launched: NULL pointers, a negative delay, t0 < 0, W or n_bins out of range, max_pulses
 *   or max_width outside 1 .. 4096, n_rows outside 1 .. max_rows_per_push.  Lifetime as for a bf_cond: a handle that goes first
 *   releases the device memory, the stage then answers BF_ERR_STATE and can still be destroyed; destroying an attached injector detaches it.
 * Host helpers (fp64, no GPU):
 * bf_inj_burst_profile: per channel, s = smear[f] (rows of intra-channel smearing, >= 1; smear == NULL: 1),
 *   g[i] = (1 / s) sum_{j < s} exp(-(i - centre - j + (s - 1) / 2)^2 / (2 sigma^2)), j ascending; N = sum_i g[i], i ascending;
 *   profile[f][i] = (float)(fluence[f] (g[i] / N)).  N == 0 (the window misses the pulse), sigma not > 0, NaN: BF_ERR_INVALID.
 * bf_inj_nearest_trial: the trial d of ladder int32 [n_dm][n_freq_total] that minimises sum_f |ladder[d][f] - delay[f]| (int64; ties: lowest d).
 * bf_inj_match: candidate c matches truth k iff c.beam == beam, |c.dm - trial| <= dm_tol and [c.t_start, c.t_start + c.width - 1]
 *   meets [t_lo - t_tol, t_hi + t_tol]; best[k] = the matching candidate with the largest snr (ties: lower index), -1 if none. */
#define BF_INJ_MAX_PULSES 4096
#define BF_INJ_MAX_WIDTH 4096
#define BF_INJ_MAX_TRAINS 4
typedef struct bf_inj bf_inj;
typedef struct bf_inj_truth {
    uint64_t t_lo, t_hi; /* first and last output time the pulse occupies at its trial */
    int32_t trial, beam;
} bf_inj_truth;
int bf_inj_create(bf_handle *h, int n_freq_total, int max_rows_per_push, int max_pulses, int max_width, bf_inj **out);
int bf_inj_destroy(bf_inj *s);
int bf_inj_add_burst(bf_inj *s, int64_t t0, int W, const int32_t *delay, const float *profile, const float *response,
                     uint64_t *id);
int bf_inj_add_train(bf_inj *s, const bf_psr_model *model, uint64_t first_row, uint64_t n_rows, int n_bins,
                     const int32_t *delay, const float *profile, const float *response, uint64_t *id);
int bf_inj_apply(bf_inj *s, float *d_rows, int n_rows, void *hip_stream);
uint64_t bf_inj_next_row(const bf_inj *s);
uint64_t bf_inj_launches(const bf_inj *s);
int bf_inj_burst_profile(int n_freq_total, int W, double centre, double sigma, const int32_t *smear, const double *fluence,
                         float *profile);
int bf_inj_nearest_trial(const int32_t *ladder, int n_dm, int n_freq_total, const int32_t *delay, int *trial);
int bf_inj_match(const bf_inj_truth *truth, size_t n, const bf_sps_candidate *cands, size_t m, uint64_t t_tol,
                 int32_t dm_tol, int32_t *best);
int bf_dm_stream_attach_injector(bf_dm_stream *dm, bf_inj *inj);

/* ---- Multi-GPU: frequency shards and the gather of their detected powers -------------------------------
 * The reference runs 8 independent processes, one sub-band per GPU (`-g`, src/beamformer.cu:92-100,233; README.md:168)
 * and never brings their outputs together.  Here a handle may own any contiguous range of frequencies (bf_config.n_freq
 * = the LOCAL count; weights generated for those channels), one process per GPU, and the ONE collective of the path is
 * the gather of the detected powers -- RCCL point-to-point over xGMI, received straight at the final position.
 * The input voltages are never exchanged: [freq][time][ant] is frequency-major, every rank reads its own slice.
 *
 * Row = one detected beam-block of one rank = row_floats = n_freq_local * n_beams consecutive floats; a launch over
 * n_units gemm-units produces n_rows = n_units * n_out_per_gemm rows per rank.  Layout of the gathered array:
 *   BF_GATHER_LAYOUT_FREQ_MAJOR  [row][world * n_freq_local][beam] -- the reference's [o][f][b] over the whole band: rank r's
 *                                row o sits at ((o * world + r) * row_floats): one message per (row, sender)
 *   BF_GATHER_LAYOUT_RANK_MAJOR  [rank][row][n_freq_local][beam]   -- sub-band-major (the reference's own 8-stream shape):
 *                                one contiguous message per sender
 * Who receives (root): a rank >= 0: only that rank (d_full may be NULL elsewhere); BF_GATHER_ROOT_ALL: every rank receives
 * everything; BF_GATHER_ROOT_DISTRIBUTED: rank j becomes the owner of rows [j * n_rows/world, (j+1) * n_rows/world) of
 * the WHOLE band (n_rows % world == 0) -- an all-to-all that loads every xGMI link of every GPU in both directions
 * instead of funnelling world-1 shards into one GPU's links, and leaves all frequencies of a time range on one device,
 * which is what a dedispersion search wants.  In the layouts above `row` then counts from the owner's first row and
 * n_rows is the number of rows the receiver holds (bf_gather_rows_held). */
#define BF_GATHER_ROOT_ALL (-1)
#define BF_GATHER_ROOT_DISTRIBUTED (-2)
typedef struct bf_comm bf_comm;
#define BF_COMM_ID_BYTES 128
#define BF_GATHER_LAYOUT_FREQ_MAJOR 0
#define BF_GATHER_LAYOUT_RANK_MAJOR 1
int bf_comm_unique_id(void *id128);                 /* rank 0: ncclGetUniqueId; hand the 128 bytes to the other ranks */
int bf_comm_create(int rank, int world, const void *id128, int device, bf_comm **out); /* world == 1 needs no id / RCCL */
int bf_comm_destroy(bf_comm *c);
int bf_comm_rank(const bf_comm *c);
int bf_comm_world(const bf_comm *c);
/* Evidence for a scaling record (the reference's 8 processes never meet, src/beamformer.cu:92-100): how many ranks the LIBRARY reports for the communicator (ncclCommCount; 0 = this bf_comm
 * has no RCCL communicator, -1 = the library cannot say), its version (ncclGetVersion, e.g. 22203; 0 = unknown) and the
 * file the point-to-point calls were resolved from.  Any pointer may be NULL. */
int bf_comm_info(const bf_comm *c, int *lib_ranks, int *version, char *lib_path, size_t n);
int bf_comm_library_info(int *version, char *lib_path, size_t n); /* the same two answers BEFORE a communicator exists (dlopen only) */
int bf_gather_detected(bf_comm *c, const float *d_local, size_t n_rows, size_t row_floats, int root, int layout,
                       float *d_full, void *hip_stream);
/* The same gather into BF_GATHER_LAYOUT_FREQ_MAJOR -- the reference's [o][f][b] over the whole band, src/beamformer.cuh:147 --
 * by a second TRANSPORT.  bf_gather_detected receives every (row, sender) run at its final position: no extra pass over the
 * data, but one point-to-point message per row and sender (14,336 messages of 32 KiB per rank for a 128-gemm-unit step of
 * BASELINE configs[3] on 8 GPUs).  This entry point puts ONE message per sender on the wire (the rank-major plan, received
 * into d_stage) and then moves the rows to their freq-major places with one device pass (every float read and written once,
 * whole 128-byte lines, nontemporal); the receiver's own rows go straight from d_local to d_full.  d_stage: caller-owned,
 * as large as d_full (rows held x world x row_floats floats; may be NULL on ranks that receive nothing, and when world == 1);
 * row_floats a multiple of 4, both buffers 16-byte aligned.  Bit-identical d_full either way; which is faster is a property
 * of the fabric and the message count (bench.py times both: gather_modes.*_freq_major[_staged]). */
int bf_gather_detected_staged(bf_comm *c, const float *d_local, size_t n_rows, size_t row_floats, int root, float *d_full,
                              float *d_stage, void *hip_stream);
/* The layout arithmetic as plain host functions (no device, no RCCL): float offset of (rank, row) in the gathered array --
 * [o][f][b] of src/beamformer.cuh:147 with f running over the shards -- and the list of messages one rank issues (kind: send
 * to peer, receive from peer, or copy its own rows). */
size_t bf_gather_offset(int layout, size_t n_rows_held, size_t row_floats, int world, int rank, size_t row);
size_t bf_gather_rows_held(size_t n_rows, int world, int rank, int root); /* rows `rank` ends up holding (0: it only sends) */
#define BF_GATHER_SEND 0
#define BF_GATHER_RECV 1
#define BF_GATHER_COPY 2
typedef struct bf_gather_msg {
    int kind, peer;
    size_t local_offset; /* floats into d_local (send / copy source; for a receive: the sender's offset) */
    size_t full_offset;  /* floats into d_full (receive / copy destination) */
    size_t count;        /* floats */
} bf_gather_msg;
size_t bf_gather_plan(int layout, size_t n_rows, size_t row_floats, int world, int rank, int root, bf_gather_msg *msgs,
                      size_t capacity); /* returns the number of messages (call with capacity 0 to size the array) */

/* Device pointer of the per-queue block buffer bf_enqueue_block fills ([n_gemms_per_block][output][freq][beam]: the
 * reference's d_dedispersed per stream, src/beamformer.cu:258,481) and the hipStream_t of compute queue `stream_idx`
 * (stream[i], src/beamformer.cu:305-312): what a caller needs to chain bf_gather_detected behind a block launch. */
int bf_block_output_device(bf_handle *h, int stream_idx, float **d_out);
int bf_queue_stream(bf_handle *h, int stream_idx, void **hip_stream);
/* A handle-owned device buffer (allocated like src/beamformer.cu:249-266 allocates the per-stream ones) for the gathered block of compute queue `stream_idx`: n_gemms_per_block * world *
 * bf_floats_per_detect floats ([unit][output][world * n_freq][beam] with the freq-major layout); allocated on first use. */
int bf_block_gather_device(bf_handle *h, int stream_idx, int world, float **d_full);
int bf_block_gather_stage_device(bf_handle *h, int stream_idx, int world, float **d_stage); /* same size: d_stage of bf_gather_detected_staged */
/* Asynchronous device-to-host copy of n_floats on compute queue `stream_idx` (the cudaMemcpyAsync of src/beamformer.cu:485-488
 * for a caller-chosen source): behind everything enqueued on that queue before the call, gemm-units included. */
int bf_enqueue_d2h(bf_handle *h, int stream_idx, const float *d_src, float *host_dst, size_t n_floats);

/* The two dedispersion entry points above (src/beamformer.cu:498-504) on a gathered band: the same kernels over n_freq_total = world * n_freq
 * channels of a [row][n_freq_total][beam] array (BF_GATHER_LAYOUT_FREQ_MAJOR on the receiving rank) -- ascending f over the
 * WHOLE band, i.e. the bits one GPU holding all channels would produce. */
int bf_dedisperse_band_device(bf_handle *h, const float *d_out_unit, int n_freq_total, float *d_ded, void *hip_stream);
int bf_dedisperse_dm_band_device(bf_handle *h, const float *d_series, int n_t, int n_freq_total, const int32_t *d_delays,
                                 int n_dm, int n_t_out, float *d_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DSABF_H */
