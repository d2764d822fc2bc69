// bf_scheduler.cpp -- host mirror, part 3: observation_loop_state (src/observation_loop.hh:1-177) on an
// event backend, and the two branches of the reference's main loop (src/beamformer.cu:364-534) on the C-ABI of dsabf.h:
// run_debug_observation (DEBUG) and run_observation (production).
#include "../../include/dsabf_host.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <iostream>

#include "../../include/dsabf_host.h"
#include "bf_host_internal.h"

namespace dsabf {

// ---- event backends ---------------------------------------------------------------------------------------------
namespace {

struct hip_backend : event_backend {
    bf_handle* h;
    explicit hip_backend(bf_handle* hh) : h(hh) {}
    void* create() override
    {
        bf_event* e = nullptr;
        if (bf_event_create_on(h, &e) != BF_OK) return nullptr;   // on the handle's device, not the caller's current one
        return e;
    }
    void destroy(void* ev) override { bf_event_destroy(static_cast<bf_event*>(ev)); }
    int record_transfer(void* ev) override { return ev ? bf_record_transfer_event(h, static_cast<bf_event*>(ev)) : BF_ERR_INVALID; }
    int record_analysis(void* ev) override { return ev ? bf_record_analysis_event(h, static_cast<bf_event*>(ev)) : BF_ERR_INVALID; }
    int query(void* ev) override { return ev ? bf_event_query(static_cast<bf_event*>(ev)) : BF_ERR_INVALID; }
};

}  // namespace

event_backend* make_hip_event_backend(bf_handle* h) { return new hip_backend(h); }

// ---- observation_loop_state (src/observation_loop.hh:54-176) -------------------------------------------------------
observation_loop_state::observation_loop_state(uint64_t max_tsep, uint64_t max_totsep, const bf_config& cfg,
                                               event_backend* backend, bool debug)
    // The device ring has n_blocks_on_gpu slots and block j lives in slot j % n_blocks_on_gpu until its analysis has COMPLETED: a
    // transfer may run at most n_blocks_on_gpu blocks ahead of blocks_analyzed, or it overwrites voltages a kernel is still reading.
    // The reference never meets the case (N_BLOCKS_ON_GPU 8 > MAX_TOTAL_SEP 4, both compile-time: src/beamformer.hh:85,124); with
    // a run-time ring the separations are held to its size (found by the random DEBUG-flow fuzz, round 5: 2 slots, 1 run in 400).
    : maximum_transfer_seperation(std::min<uint64_t>(max_tsep, (uint64_t)std::max(cfg.n_blocks_on_gpu, 1))),
      maximum_total_seperation(std::min<uint64_t>(max_totsep, (uint64_t)std::max(cfg.n_blocks_on_gpu, 1))), debug_mode(debug),
      verbose(cfg.verbose != 0), n_gemms_per_block(cfg.n_gemms_per_block), n_blocks_on_gpu(cfg.n_blocks_on_gpu),
      n_events(5 * cfg.n_blocks_on_gpu), ev(backend)
{
    BlockTransferredSync.resize(n_events);
    BlockAnalyzedSync.resize(n_events);
    for (int i = 0; i < n_events; i++) {  // :58-61
        BlockTransferredSync[i] = ev->create();
        BlockAnalyzedSync[i] = ev->create();
        if (!BlockTransferredSync[i] || !BlockAnalyzedSync[i]) fail(BF_ERR_DEVICE);
    }
}

void observation_loop_state::fail(int code)
{
    if (error == BF_OK) {
        error = code < 0 ? code : BF_ERR_DEVICE;
        std::cerr << "observation_loop_state: event backend failed (" << error << "): " << bf_last_error() << std::endl;
    }
}

observation_loop_state::~observation_loop_state()
{
    for (int event = 0; event < n_events; event++) {  // :65-68
        if (BlockAnalyzedSync[event]) ev->destroy(BlockAnalyzedSync[event]);
        if (BlockTransferredSync[event]) ev->destroy(BlockTransferredSync[event]);
    }
}

namespace {

// generate_*_event (:71-81): records the next event of one direction; the queue counter moves only if the backend took the record.
int record_next_event(event_backend* ev, const std::vector<void*>& sync, uint64_t& queued, int (event_backend::*record)(void*))
{
    void* e = sync[queued % sync.size()];
    const int rc = e ? (ev->*record)(e) : BF_ERR_DEVICE;
    if (rc == BF_OK) queued++;
    return rc;
}

// check_*_events (:83-118): retires, in order, the events of [done, queued) that have fired, and stops at the first that has not.
int retire_fired_events(event_backend* ev, std::vector<void*>& sync, uint64_t& done, uint64_t queued, const char* verbose_text)
{
    for (uint64_t event = done; event < queued; event++) {
        void*& e = sync[event % sync.size()];
        const int rc = ev->query(e);
        if (rc < 0) return rc;   // the reference dies in gpuErrchk here; never treat an error as "not ready yet"
        if (rc != BF_OK) break;  // :98, :116
        done++;
        if (verbose_text) std::cout << "Block " << event << verbose_text << std::endl;
        ev->destroy(e);  // :95-96, :112-113 destroy and recreate
        e = ev->create();
        if (!e) return BF_ERR_DEVICE;
    }
    return BF_OK;
}

}  // namespace

void observation_loop_state::generate_transfer_event()
{
    if (error != BF_OK) return;
    const int rc = record_next_event(ev, BlockTransferredSync, blocks_transfer_queue, &event_backend::record_transfer);  // :73
    if (rc != BF_OK) fail(rc);
}

void observation_loop_state::generate_analysis_event()
{
    if (error != BF_OK) return;
    const int rc = record_next_event(ev, BlockAnalyzedSync, blocks_analysis_queue, &event_backend::record_analysis);  // :79
    if (rc != BF_OK) fail(rc);
}

void observation_loop_state::check_transfer_events()
{
    if (error != BF_OK) return;
    const int rc = retire_fired_events(ev, BlockTransferredSync, blocks_transferred, blocks_transfer_queue,  // :85
                                       verbose ? " transfered to GPU" : nullptr);
    if (rc != BF_OK) fail(rc);
}

void observation_loop_state::check_analysis_events()
{
    if (error != BF_OK) return;
    const int rc = retire_fired_events(ev, BlockAnalyzedSync, blocks_analyzed, blocks_analysis_queue,  // :104
                                       verbose ? " Analyzed" : nullptr);
    if (rc != BF_OK) fail(rc);
}

uint64_t observation_loop_state::get_current_analysis_gemm(int time_slice)
{
    most_recent_gemm = (int)(blocks_analysis_queue * n_gemms_per_block + time_slice);  // :122
    return most_recent_gemm;
}

uint64_t observation_loop_state::get_current_transfer_gemm() const { return blocks_transfer_queue * n_gemms_per_block; }

bool observation_loop_state::check_ready_for_transfer() const
{
    return ((blocks_transfer_queue - blocks_analyzed < maximum_total_seperation) &&
            (blocks_transfer_queue - blocks_transferred < maximum_transfer_seperation) && !transfers_complete);  // :131-133
}

bool observation_loop_state::check_ready_for_dh2_transfer(int time_slice)
{
    int current_gemm = (int)get_current_analysis_gemm(time_slice);  // :137
    return (current_gemm < n_pt_sources);
}

bool observation_loop_state::check_ready_for_analysis() const { return (blocks_analysis_queue < blocks_transferred); }

bool observation_loop_state::check_observations_complete()
{
    if (debug_mode && most_recent_gemm < n_pt_sources - 1) return false;               // :146-151: DEBUG also waits for the last source
    if (blocks_analyzed != blocks_transfer_queue || !transfers_complete) return false;  // :153-157
    std::cout << "obs Complete" << std::endl;
    return true;
}

bool observation_loop_state::check_transfers_complete()
{
    if (blocks_transfer_queue * n_gemms_per_block >= (uint64_t)std::max(n_pt_sources, 0)) {  // :163
        transfers_complete = 1;
        return true;
    }
    return false;
}

std::ostream& operator<<(std::ostream& out, const observation_loop_state& a)
{
    return out << "A: " << a.blocks_analyzed << ", AQ: " << a.blocks_analysis_queue << ", T: " << a.blocks_transferred
               << ", TQ: " << a.blocks_transfer_queue << "\n"
               << "current_gemm: " << a.most_recent_gemm << ", transfers_complete: " << a.transfers_complete;
}

void dm_trial_share(int n_dm, int world, int rank, int* first, int* count)
{
    const int base = world > 0 ? n_dm / world : 0, extra = world > 0 ? n_dm % world : 0;
    if (count) *count = (rank >= 0 && rank < world) ? base + (rank < extra ? 1 : 0) : 0;
    if (first) *first = rank * base + std::min(std::max(rank, 0), extra);
}

// ---- what the two loops share ----------------------------------------------------------------------------------------------
namespace {

// The reference dies inside gpuErrchk with this line (src/beamformer.cuh:19-29); the loops print it and return the code.
int gpu_error(std::ostream& log, int rc)
{
    log << "GPUassert: " << bf_last_error() << std::endl;
    return rc;
}

// What a run holds on the device and in pinned memory.  Released in this order: sync, the search stage and the DM stream (before their handle), the pinned
// buffers in the order they were allocated, the handle.
struct run_resources {
    bf_handle* h = nullptr;
    bf_dm_stream* dm = nullptr;
    bf_sps* sps = nullptr;
    bf_cond* cond = nullptr;
    bf_psr* psr = nullptr;
    bf_ffa* ffa = nullptr;
    bf_inj* inj = nullptr;
    bf_corr* corr = nullptr;
    bf_sk* sk = nullptr;
    bf_stokes* stokes = nullptr;
    bf_evt* evt = nullptr;
    bf_vhist* vhist = nullptr;
    std::vector<void*> pinned;
    ~run_resources()
    {
        if (h) bf_stream_sync(h, -1);
        bf_corr_destroy(corr);
        bf_sk_destroy(sk);
        bf_stokes_destroy(stokes);
        bf_vhist_destroy(vhist);
        bf_sps_destroy(sps);
        bf_evt_destroy(evt);
        bf_cond_destroy(cond);
        bf_psr_destroy(psr);
        bf_ffa_destroy(ffa);
        bf_inj_destroy(inj);
        bf_dm_stream_destroy(dm);
        for (void* p : pinned) bf_free_pinned(p);
        bf_destroy(h);
    }
    int alloc_pinned(size_t n_floats, float** out)
    {
        void* p = nullptr;
        const int rc = bf_alloc_pinned(&p, n_floats * sizeof(float));
        if (rc == BF_OK) pinned.push_back(p);
        *out = static_cast<float*>(p);
        return rc;
    }
};

// The weights of a run onto its handle: `w` as it is, or -- with gains and / or nulls -- calibrated and projected first.  w_set (optional,
// may be `w` itself) receives what was set.  Returns the C-ABI's code; the caller reports a failure its own way.
int set_run_weights(bf_handle* h, int device, const std::vector<int8_t>& w, const double* gains, const null_vectors* nulls, const uint8_t* ant_flags,
                    int8_t* w_set, std::ostream& log)
{
    if (!gains && !nulls) {
        const int rc = bf_set_weights(h, w.data());
        if (rc == BF_OK && w_set && w_set != w.data()) ::memcpy(w_set, w.data(), w.size());
        return rc;
    }
    const int rc = set_weights_conditioned(h, device, w.data(), gains, nulls, w_set, ant_flags);
    if (rc == BF_OK && gains) log << "Calibrated the weights with one layer of gains" << std::endl;
    if (rc == BF_OK && nulls) log << "Projected up to " << nulls->n_null << " interferer vectors per channel out of the weights" << std::endl;
    return rc;
}

// The reference's launch pattern for one block (src/beamformer.cu:454-519): one gemm-unit per launch, round-robin over the compute
// queues.  timeSlice[st] is the unit that stream st takes next (:319); it is back at st when the block is through.  dst(st, unit)
// names the unit's D2H destination (nullptr, already logged: no destination, BF_ERR_STATE); after(st, unit), if any, is what
// follows the enqueue on that stream.
int enqueue_block_by_units(bf_handle* h, const bf_config& cfg, int gpu_block, std::vector<int>& timeSlice, std::ostream& log,
                           const std::function<int(int st, int unit)>& after, const std::function<float*(int st, int unit)>& dst)
{
    const int n_streams = cfg.n_streams;
    for (int part = 0; part < cfg.n_gemms_per_block / n_streams; part++) {
        for (int st = 0; st < n_streams; st++) {
            float* d = dst(st, timeSlice[st]);  // the reference's destination, :485-488
            if (!d) return BF_ERR_STATE;
            int rc = bf_enqueue_gemm_unit(h, st, gpu_block, timeSlice[st], d);  // :464-488
            if (rc == BF_OK && after) rc = after(st, timeSlice[st]);
            if (rc != BF_OK) return gpu_error(log, rc);
            timeSlice[st] += n_streams;  // :515-519
            if (timeSlice[st] >= cfg.n_gemms_per_block) timeSlice[st] -= cfg.n_gemms_per_block;
        }
    }
    return BF_OK;
}

// The closing lines of both loops (src/beamformer.cu:540-562).  "Launch pattern" is not a line of the reference: it says which
// caller-side loop the timing lines above it were measured with.
void closing_report(std::ostream& log, float ms, uint64_t chunks, float ms_per_chunk, double gbytes_per_s, const char* launch_pattern)
{
    log << "Observation ran in " << ms << "milliseconds.\n";
    log << "Code produced outputs for " << chunks << " data chunks.\n";
    log << "Time per data chunk: " << ms_per_chunk << " milliseconds.\n";
    log << "Approximate datarate: " << gbytes_per_s << "GB/s" << std::endl;
    log << "Launch pattern: " << launch_pattern << std::endl;
    log << "Synchronized" << std::endl;
}
const char* const kUnitLaunchPattern = "the reference's loop, one bf_enqueue_gemm_unit per gemm-unit (src/beamformer.cu:454-519)";

// A failed record / query of the loop's events: the reference exits in gpuErrchk, never keep polling.
int event_backend_error(std::ostream& log, const observation_loop_state& obs_state)
{
    log << "GPUassert: event backend failed: " << bf_last_error() << std::endl;
    return obs_state.status();
}

// ---- the DEBUG main() flow (src/beamformer.cu:12-621 with -DDEBUG) ----------------------------------------------------
// Block-granular analysis: one fused launch over the block's gemm-units, their detected powers to the host in ONE copy (a4: every
// unit still travels, as src/beamformer.cu:485-488 has it), one DM-0 launch for all of them (a8).
int debug_block_launch(bf_handle* h, const bf_config& cfg, int q, observation_loop_state& obs_state, int n_src, float* beam_out_blk,
                       float* dedispersed_out, bool verbose, std::ostream& log)
{
    const int first_gemm = (int)obs_state.get_current_analysis_gemm(0);
    if (verbose) log << "Queueing Beamforming. Start Dir = " << first_gemm << std::endl;
    const size_t n_f_per_detect = bf_floats_per_detect(&cfg);
    std::vector<float*> dst((size_t)cfg.n_gemms_per_block);
    for (int u = 0; u < cfg.n_gemms_per_block; u++) dst[(size_t)u] = beam_out_blk + n_f_per_detect * (size_t)u;
    int rc = bf_enqueue_block(h, q, (int)obs_state.get_next_gpu_analysis_block(), 0, cfg.n_gemms_per_block, dst.data());
    const int n_valid = std::min(cfg.n_gemms_per_block, n_src - first_gemm);   // check_ready_for_dh2_transfer, :492
    if (rc == BF_OK && n_valid > 0)
        rc = bf_enqueue_block_dedisperse(h, q, 0, n_valid, &dedispersed_out[(size_t)first_gemm * cfg.n_beams]);
    if (rc != BF_OK) return gpu_error(log, rc);
    (void)obs_state.get_current_analysis_gemm(cfg.n_gemms_per_block - 1);   // most_recent_gemm = the block's last unit
    return BF_OK;
}

}  // namespace

int run_debug_observation(const bf_config& cfg, const debug_run_options& opt, debug_run_result* res,
                          std::vector<float>* dedispersed_result, std::ostream& log)
{
    const int n_streams = cfg.n_streams;
    if (cfg.n_gemms_per_block % n_streams) {
        log << "N_GEMMS_PER_BLOCK must be divisible by N_STREAMS" << std::endl;
        return BF_ERR_INVALID;
    }
    if (kSourcesPerBatch % cfg.n_gemms_per_block) {  // static_assert src/beamformer.hh:151
        log << "N_SOURCES_PER_BATCH must be divisible by N_GEMMS_PER_BLOCK" << std::endl;
        return BF_ERR_INVALID;
    }
    std::vector<antenna> pos((size_t)cfg.n_ant);
    std::vector<beam_direction> dir((size_t)cfg.n_beams);
    test_data_generator input_data_generator(cfg);
    if (!input_data_generator.get_data()) return BF_ERR_DEVICE;
    if (opt.sources && input_data_generator.read_in_source_directions(opt.sources) != 0) {
        log << "beam: could not read source direction file " << opt.sources << std::endl;
        return BF_ERR_INVALID;
    }
    if (opt.positions && read_in_position_locations(opt.positions, cfg.n_ant, pos.data()) != 0) return BF_ERR_INVALID;
    if (opt.directions && read_in_beam_directions(opt.directions, cfg.n_beams, dir.data()) != 0) return BF_ERR_INVALID;
    if (!opt.positions) default_positions(cfg.n_ant, pos.data());      // :135-140
    if (!opt.directions) default_directions(cfg.n_beams, dir.data());  // :142-147
    if (opt.verbose) print_all_defines(cfg, log);

    run_resources dev;
    int rc = bf_create(&cfg, opt.device, &dev.h);
    if (rc != BF_OK) return gpu_error(log, rc);
    bf_handle* const h = dev.h;

    const int n_src = input_data_generator.get_n_pt_sources();
    const size_t n_f_per_detect = bf_floats_per_detect(&cfg);
    const size_t n_dedispersed = (size_t)cfg.n_beams * std::max(n_src, 1);
    float *beam_out = nullptr, *dedispersed_out = nullptr;
    if ((rc = dev.alloc_pinned(n_f_per_detect * n_streams, &beam_out)) != BF_OK) return rc;  // :249
    if ((rc = dev.alloc_pinned(n_dedispersed, &dedispersed_out)) != BF_OK) return rc;         // :212
    ::memset(dedispersed_out, 0, n_dedispersed * sizeof(float));

    {  // :230-241, :251, :272
        std::vector<int8_t> fourier_coefficients((size_t)cfg.n_freq * cfg.n_ant * cfg.n_beams * 2);
        generate_fourier_coefficients(cfg.n_beams, cfg.n_ant, cfg.n_freq, 0, opt.gpu, pos.data(), dir.data(),
                                      fourier_coefficients.data());
        rc = set_run_weights(h, opt.device, fourier_coefficients, opt.gains, opt.nulls, opt.ant_flags, opt.weights_out, log);
        if (rc != BF_OK) return gpu_error(log, rc);
    }

    std::vector<int> timeSlice((size_t)n_streams);
    for (int i = 0; i < n_streams; i++) timeSlice[i] = i;  // :319
    float* beam_out_blk[2] = {nullptr, nullptr};   // block_launch: a block's detected powers on the host, per alternating queue
    uint64_t block_launches = 0;
    for (int q = 0; q < 2 && opt.block_launch; q++) {   // (page-locking 2 x N_GEMMS_PER_BLOCK x 2 MiB is setup, like beam_out)
        if ((rc = dev.alloc_pinned(n_f_per_detect * (size_t)cfg.n_gemms_per_block, &beam_out_blk[q])) != BF_OK) return rc;
        float* d_blk = nullptr;                        // and the queue's device-side block buffer (allocated at first use otherwise)
        if ((rc = bf_block_output_device(h, q % n_streams, &d_blk)) != BF_OK) return rc;
    }

    hip_backend backend(h);
    observation_loop_state obs_state(kMaxTransferSep, kMaxTotalSep, cfg, &backend, /*debug_mode=*/true);  // :322
    obs_state.set_n_pt_sources(n_src);                                                                  // :325

    if (opt.verbose) {
        log << "Executing beamformer.cu" << "\n";
        log << "MAX_TOTAL_SEP: " << kMaxTotalSep << "\n";
        log << "MAX_TRANSFER_SEP: " << kMaxTransferSep << std::endl;
    }

    float time_accumulator_ms = 0, observation_time_ms = 0;
    bf_timer_start(h);  // :358
    const size_t block_bytes = bf_bytes_per_block(&cfg);
    const size_t input_data_size = input_data_generator.input_data_size();

    while (!obs_state.check_observations_complete()) {  // :364
        if (opt.verbose) log << "##########################################" << std::endl << obs_state << std::endl;
        if (obs_state.check_ready_for_transfer()) {  // :378
            if (input_data_generator.check_need_to_generate_more_input_data((int)obs_state.get_blocks_transferred())) {
                log << "Generating new source data" << std::endl;
                bf_timer_stop(h, &time_accumulator_ms);  // :408-409
                observation_time_ms += time_accumulator_ms;
                input_data_generator.generate_test_data(pos.data(), opt.gpu);
                bf_timer_start(h);
                log << "done generating test data" << std::endl;
            }
            if (input_data_generator.check_data_ready_for_transfer((int)obs_state.get_blocks_transfer_queue())) {  // :421
                char* input_data = input_data_generator.get_data();
                rc = bf_submit_block(h, (int)obs_state.get_next_gpu_transfer_block(),
                                     &input_data[(block_bytes * obs_state.get_blocks_transfer_queue()) % input_data_size],
                                     block_bytes, nullptr);  // :425-429
                if (rc != BF_OK) return gpu_error(log, rc);
                obs_state.generate_transfer_event();  // :431
            }
            obs_state.check_transfers_complete();  // :438
        }
        obs_state.check_transfer_events();  // :446

        if (obs_state.check_ready_for_analysis()) {  // :452
            if (opt.block_launch) {
                // Two queues alternate so that block i+1's kernel overlaps block i's copy.
                const int q = (int)(block_launches++ % 2) % n_streams;
                rc = debug_block_launch(h, cfg, q, obs_state, n_src, beam_out_blk[q], dedispersed_out, opt.verbose, log);
            } else {
                const auto dedisperse_unit = [&](int st, int unit) {
                    if (!obs_state.check_ready_for_dh2_transfer(unit)) return (int)BF_OK;  // :492
                    const int current_gemm = (int)obs_state.get_current_analysis_gemm(unit);
                    if (opt.verbose) log << "Current GEMM: " << current_gemm << std::endl;
                    return bf_enqueue_dedisperse(h, st, &dedispersed_out[(size_t)current_gemm * cfg.n_beams]);  // :498-510
                };
                rc = enqueue_block_by_units(h, cfg, (int)obs_state.get_next_gpu_analysis_block(), timeSlice, log, dedisperse_unit, [&](int st, int unit) {
                    if (opt.verbose && st == 0) log << "Queueing Beamforming. Start Dir = " << obs_state.get_current_analysis_gemm(unit) << std::endl;
                    return &beam_out[(size_t)st * n_f_per_detect];
                });
            }
            if (rc != BF_OK) return rc;
            obs_state.generate_analysis_event();  // :525
        }
        obs_state.check_analysis_events();  // :532
        if (obs_state.status() != BF_OK) return event_backend_error(log, obs_state);
    }

    bf_timer_stop(h, &time_accumulator_ms);  // :540
    observation_time_ms += time_accumulator_ms;
    const long long chunks = (long long)n_src * cfg.n_out_per_gemm;
    const double rate = bf_bytes_per_gemm(&cfg) * (double)n_src / observation_time_ms / 1e6;
    bf_stream_sync(h, -1);  // :560-562
    closing_report(log, observation_time_ms, (uint64_t)chunks, observation_time_ms / chunks, rate,
                   opt.block_launch ? "one bf_enqueue_block per PSRDADA block" : kUnitLaunchPattern);

    if (opt.output && opt.output[0])
        if (write_array_to_disk_as_python_file(dedispersed_out, n_src, cfg.n_beams, opt.output) != 0)  // :568-571
            log << "could not write " << opt.output << std::endl;
    if (dedispersed_result) dedispersed_result->assign(dedispersed_out, dedispersed_out + (size_t)n_src * cfg.n_beams);
    if (res) {
        res->observation_time_ms = observation_time_ms;
        res->n_pt_sources = n_src;
        res->data_chunks = chunks;
    }
    return BF_OK;
}

// ---- production observation loop (src/beamformer.cu:364-534, #ifndef DEBUG branches) -------------------------------------
namespace {

// A sharded run enters its first collective -- the gather behind block 0 -- only if EVERY shard got through its setup: each rank
// takes part in ONE exchange of "ready" flags before the loop, whichever way its setup went (a rank that bailed out alone would
// leave the others waiting in that gather for ever: ADVICE r05).  The caller's own preparations count too (local_setup_ok).
struct setup_gate {
    bf_comm* comm;
    bool done = false;
    int fail(int rc)   // an early return of the setup: tell the other shards, once
    {
        if (comm && !done) {
            done = true;
            bool all = false;
            (void)comm_all_ok(comm, false, &all);
        }
        return rc;
    }
    int pass(bool local_setup_ok)   // the end of the setup: BF_OK if every shard (and every caller) is ready
    {
        if (!comm)
            return local_setup_ok ? BF_OK : set_error(BF_ERR_STATE, "run_observation: the caller reported a failed setup (local_setup_ok = false)");
        done = true;
        bool all = false;
        const int rc = comm_all_ok(comm, local_setup_ok, &all);
        if (rc != BF_OK || all) return rc;
        return set_error(BF_ERR_STATE, local_setup_ok ? "run_observation: another shard of this run failed its setup; nothing was started"
                                                      : "run_observation: this shard's caller reported a failed setup (local_setup_ok = false)");
    }
};

// who holds the gathered band after every block: one rank, or (BF_GATHER_ROOT_ALL) every rank
bool holds_band(const observation_options& opt) { return !opt.comm || opt.gather_root == BF_GATHER_ROOT_ALL || opt.rank == opt.gather_root; }

// The option combinations run_observation refuses, before anything is read or created.
int check_options(const bf_config& cfg, const observation_options& opt)
{
    const bool is_root = holds_band(opt);
    if (cfg.n_gemms_per_block % cfg.n_streams) return BF_ERR_INVALID;
    if (opt.world < 1 || opt.rank < 0 || opt.rank >= opt.world || opt.gather_root < BF_GATHER_ROOT_ALL || opt.gather_root >= opt.world)
        return set_error(BF_ERR_INVALID, "run_observation: need 0 <= rank < world and gather_root a rank or BF_GATHER_ROOT_ALL");
    if (opt.comm && (bf_comm_rank(opt.comm) != opt.rank || bf_comm_world(opt.comm) != opt.world))
        return set_error(BF_ERR_INVALID, "run_observation: the communicator's rank / world differ from the options'");
    if (opt.comm && !opt.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the sharded gather needs block-granular launches");
    if (opt.comm && opt.sink && !is_root) return set_error(BF_ERR_INVALID, "run_observation: only the gather root may have a sink");
    if (opt.dm_delays && opt.n_dm <= 0) return set_error(BF_ERR_INVALID, "run_observation: dm_delays without n_dm");
    if (opt.dm_sink && !opt.dm_delays) return set_error(BF_ERR_INVALID, "run_observation: a dm_sink needs dm_delays");
    if (opt.sps_widths < 0 || opt.sps_widths > 8) return set_error(BF_ERR_INVALID, "run_observation: sps_widths must be 0 (off) .. 8");
    if ((opt.sps_widths || opt.sps_sink) && !opt.dm_delays) return set_error(BF_ERR_INVALID, "run_observation: the single-pulse search needs the DM stage (dm_delays)");
    if (opt.sps_sink && !opt.sps_widths) return set_error(BF_ERR_INVALID, "run_observation: a sps_sink needs sps_widths > 0");
    if (opt.evt && !opt.sps_widths) return set_error(BF_ERR_INVALID, "run_observation: the event builder (evt) needs sps_widths > 0");
    if ((opt.event_sink || opt.stamp_sink) && !opt.evt) return set_error(BF_ERR_INVALID, "run_observation: an event_sink or a stamp_sink needs evt");
    if (opt.evt && (opt.stamp_bins < 1 || opt.stamp_tbin < 0 || opt.stamp_fbin < 1 || opt.stamp_max_per_deliver < 0 ||
                    (cfg.n_freq * (opt.comm ? opt.world : 1)) % opt.stamp_fbin != 0))
        return set_error(BF_ERR_INVALID, "run_observation: need stamp_bins >= 1, stamp_tbin >= 0, stamp_max_per_deliver >= 0 and stamp_fbin >= 1 dividing the band");
    if (opt.vcut_sink && !opt.evt) return set_error(BF_ERR_INVALID, "run_observation: a vcut_sink needs evt");
    if (opt.vcut_sink && opt.comm) return set_error(BF_ERR_INVALID, "run_observation: voltage cuts are not available on a sharded run");
    if (opt.vcut_sink && (opt.vcut_units < 1 || opt.vcut_history_units < 0 || opt.vcut_max_per_deliver < 0))
        return set_error(BF_ERR_INVALID, "run_observation: need vcut_units >= 1, vcut_history_units >= 0 and vcut_max_per_deliver >= 0");
    if (opt.cond_baseline < 0 || opt.cond_baseline > 64) return set_error(BF_ERR_INVALID, "run_observation: cond_baseline must be 0 (off) .. 64");
    if (opt.cond_baseline && !opt.dm_delays) return set_error(BF_ERR_INVALID, "run_observation: the conditioner needs the DM stage (dm_delays)");
    if (!opt.cond_baseline && (opt.cond_mask || opt.cond_auto_threshold != 0.0))
        return set_error(BF_ERR_INVALID, "run_observation: cond_mask / cond_auto_threshold need cond_baseline > 0");
    if (opt.incoherent_beam < -1 || opt.incoherent_beam >= cfg.n_beams)
        return set_error(BF_ERR_INVALID, "run_observation: incoherent_beam must be -1 (off) or a beam index");
    if (opt.corr_blocks < 0) return set_error(BF_ERR_INVALID, "run_observation: corr_blocks must be 0 (off) or the blocks per dump");
    if (opt.vis_sink && !opt.corr_blocks) return set_error(BF_ERR_INVALID, "run_observation: a vis_sink needs corr_blocks > 0");
    if (opt.corr_blocks && !opt.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the correlator needs block-granular launches");
    if (opt.n_psr < 0 || opt.n_psr > BF_PSR_MAX_PULSARS) return set_error(BF_ERR_INVALID, "run_observation: n_psr must be 0 (off) .. 4");
    if (opt.n_psr && !opt.dm_delays) return set_error(BF_ERR_INVALID, "run_observation: the pulsar folder needs the DM stage (dm_delays)");
    if (opt.n_psr && (!opt.psr_models || !opt.psr_delays)) return set_error(BF_ERR_INVALID, "run_observation: n_psr > 0 needs psr_models and psr_delays");
    if (opt.n_psr && (opt.psr_bins < 2 || opt.psr_bins > BF_PSR_MAX_BINS || opt.psr_dump_rows < 1))
        return set_error(BF_ERR_INVALID, "run_observation: the pulsar folder needs psr_bins in 2 .. 4096 and psr_dump_rows >= 1");
    if (!opt.n_psr && opt.psr_sink) return set_error(BF_ERR_INVALID, "run_observation: a psr_sink needs n_psr > 0");
    if (opt.inj && !opt.dm_delays) return set_error(BF_ERR_INVALID, "run_observation: pulse injection needs the DM stage (dm_delays)");
    if (opt.inj) {   // the tables' sizes: the whole band (every rank that dedisperses injects all of it), the handle's beams
        const size_t band = (size_t)cfg.n_freq * (size_t)(opt.comm ? opt.world : 1);
        for (const inj_plan::burst& b : opt.inj->bursts)
            if (b.W < 1 || b.delay.size() != band || b.profile.size() != band * (size_t)b.W || b.response.size() != (size_t)cfg.n_beams)
                return set_error(BF_ERR_INVALID, "run_observation: an injected burst needs W >= 1, delay [band], profile [band][W] and response [n_beams]");
        for (const inj_plan::train& t : opt.inj->trains)
            if (t.n_bins < 2 || t.delay.size() != band || t.profile.size() != band * (size_t)t.n_bins || t.response.size() != (size_t)cfg.n_beams)
                return set_error(BF_ERR_INVALID, "run_observation: an injected train needs n_bins >= 2, delay [band], profile [band][n_bins] and response [n_beams]");
        if (opt.inj->trains.size() > (size_t)BF_INJ_MAX_TRAINS || opt.inj->size() > (size_t)BF_INJ_MAX_PULSES)
            return set_error(BF_ERR_INVALID, "run_observation: the injection plan holds more than BF_INJ_MAX_TRAINS trains or BF_INJ_MAX_PULSES pulses");
    }
    if (opt.ffa_p_hi < 0) return set_error(BF_ERR_INVALID, "run_observation: ffa_p_hi must be 0 (off) or the end of the period range");
    if (opt.ffa_p_hi && !opt.dm_delays) return set_error(BF_ERR_INVALID, "run_observation: the periodicity search needs the DM stage (dm_delays)");
    if (!opt.ffa_p_hi && opt.ffa_sink) return set_error(BF_ERR_INVALID, "run_observation: an ffa_sink needs ffa_p_hi > 0");
    if (opt.sk_blocks < 0) return set_error(BF_ERR_INVALID, "run_observation: sk_blocks must be 0 (off) or the blocks per dump");
    if (opt.sk_sink && !opt.sk_blocks) return set_error(BF_ERR_INVALID, "run_observation: a sk_sink needs sk_blocks > 0");
    if (opt.sk_blocks && !opt.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the voltage moments need block-granular launches");
    if (opt.stokes_beams.empty() && (opt.stokes_sink || opt.stokes_int))
        return set_error(BF_ERR_INVALID, "run_observation: a stokes_sink / stokes_int needs stokes_beams");
    if (!opt.stokes_beams.empty()) {
        if (!opt.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the Stokes beams need block-granular launches");
        if (opt.stokes_beams.size() > (size_t)BF_STOKES_MAX_BEAMS)
            return set_error(BF_ERR_INVALID, "run_observation: stokes_beams holds more than BF_STOKES_MAX_BEAMS beams");
        for (int b : opt.stokes_beams)
            if (b < 0 || b >= cfg.n_beams) return set_error(BF_ERR_INVALID, "run_observation: a stokes_beams index is not a beam");
        const int n_int = opt.stokes_int ? opt.stokes_int : cfg.n_avg;
        if (n_int < 1 || (cfg.n_out_per_gemm * cfg.n_avg) % n_int)
            return set_error(BF_ERR_INVALID, "run_observation: stokes_int must divide n_out_per_gemm * n_avg");
    }
    if (opt.comm && opt.dm_sink && !is_root) return set_error(BF_ERR_INVALID, "run_observation: only the gather root may have a dm_sink");
    if (opt.dm_split_trials && (!opt.comm || opt.gather_root != BF_GATHER_ROOT_ALL))
        return set_error(BF_ERR_INVALID, "run_observation: dm_split_trials needs a sharded run gathered to every rank (BF_GATHER_ROOT_ALL)");
    return BF_OK;
}

// How the loop launches, resolved once from the options and the lab switches (DSABF_LAB=1).
struct launch_plan {
    bool block_launch = true;   // bf_enqueue_block launches, or the reference's per-gemm-unit pattern
    int upl = 0;                // gemm-units per launch of the block path
    int n_queues_used = 0;      // compute queues the block launches rotate over
    bool staged = false;        // transport of the sharded gather
    bool is_root = true;        // this rank holds the (gathered) band
    int dm_first = 0, dm_count = 0;   // this rank's share of the DM ladder
    int n_freq_band = 0;        // channels of the band the DM stage sees
    int dm_rows = 0;            // beam-blocks per launch = rows per push
    bool dm_run = false;        // this rank runs a DM stage
};

int resolve_plan(const bf_config& cfg, const observation_options& opt, launch_plan* plan)
{
    launch_plan& p = *plan;
    const char* unit_env = lab_getenv("DSABF_UNIT_LAUNCH");   // measurement / test switch: the reference's per-gemm-unit launches
    p.block_launch = opt.block_launch && !(unit_env && unit_env[0] == '1');
    if (opt.comm && !p.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the sharded gather needs block-granular launches");
    p.upl = opt.units_per_launch;
    if (const char* e = lab_getenv("DSABF_UNITS_PER_LAUNCH")) p.upl = atoi(e);
    if (p.upl <= 0 || p.upl > cfg.n_gemms_per_block || opt.comm) p.upl = cfg.n_gemms_per_block;   // 0 / sharded: the whole block
    while (cfg.n_gemms_per_block % p.upl) p.upl--;                                                  // whole launches only
    // whole blocks alternate between TWO queues (block i + 1's kernel under block i's copies, as in the DEBUG flow):
    // more queues only put more concurrent host copies beside the H2D stream (9.6 -> 9.2 us per beam-block, and
    // 11.6 -> 9.x with other streams alive in the process: tools/stream_queues.py); sub-block launches rotate over all
    p.n_queues_used = p.upl == cfg.n_gemms_per_block ? std::min(cfg.n_streams, 2) : cfg.n_streams;
    p.staged = opt.gather_staged;
    if (const char* e = lab_getenv("DSABF_GATHER_STAGED")) p.staged = e[0] == '1';
    // ---- the DM stage: where the reference's loop has its frequency collapse, src/beamformer.cu:492-511 ----
    p.is_root = holds_band(opt);
    // dm_split_trials: every rank holds the whole band (one all-gather instead of a gather) and takes ITS share of the trial ladder --
    // the DM work scales with the GPUs, the path still has ONE collective; rank r: trials [r n / R, (r + 1) n / R), the first n % R
    // ranks one more
    p.dm_count = opt.n_dm;
    if (opt.dm_split_trials) dm_trial_share(opt.n_dm, opt.world, opt.rank, &p.dm_first, &p.dm_count);
    p.n_freq_band = cfg.n_freq * (opt.comm ? opt.world : 1);
    p.dm_rows = p.upl * cfg.n_out_per_gemm;
    if (opt.dm_delays && !p.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the DM stage needs block-granular launches");
    if (opt.corr_blocks && !p.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the correlator needs block-granular launches");
    if (opt.sk_blocks && !p.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the voltage moments need block-granular launches");
    if (!opt.stokes_beams.empty() && !p.block_launch) return set_error(BF_ERR_INVALID, "run_observation: the Stokes beams need block-granular launches");
    // a sharded run dedisperses the gathered band (more ranks than trials: the surplus ranks only beamform)
    p.dm_run = opt.dm_delays && p.is_root && p.dm_count > 0;
    return BF_OK;
}

constexpr size_t kStokesSetBytesMax = (size_t)8 << 30;   // all result sets of a run's Stokes stage, per side (device, pinned)

// A stamp that is wanted: the request (local trial index), and what the sink is told about the event it belongs to.
struct stamp_want {
    bf_stamp_request rq;
    int tbin, width, dm_global;
    double snr;
};

// A voltage cut that is wanted: the request (samples, local trial index), and what the sink is told about the event it belongs to.
struct vcut_want {
    bf_vcut_request rq;
    int beam, width, dm_global;
    double snr;
};

struct dm_chunk {
    uint64_t block, first_t;
    int n_t;
    float* host;
};

// A tap on the resident voltage blocks that integrates over whole blocks -- the correlator, the voltage moments: a push per launch on
// the launch's queue, a dump after every `blocks`-th analysed block, each dump collected and delivered once that block's analysis
// event has fired.  What the stage is comes as calls of the C-ABI; the bookkeeping is written once, in production_run.
struct accum_tap {
    const char* title;   // "Correlator": the closing line
    const char* noun;    // "visibility": the sink's error line
    int blocks;          // blocks per dump (0: off)
    std::function<int(int max_in_flight, size_t* n_int64)> create;   // the stage, and the size of one dump
    std::function<int(int q, int slot, int first_unit, int n_units)> push_block;
    std::function<int()> dump;
    std::function<int(int64_t* out, uint64_t* n_columns)> collect;
    std::function<bool(uint64_t first_block, uint64_t n_columns, const int64_t* data, size_t n_int64)> deliver;   // to the sink, if there is one
    std::deque<std::pair<uint64_t, uint64_t>> pending;   // dumps issued and not yet collected -- {first block of the integration, its last block}
    std::vector<int64_t> host;                           // what collect returns for one dump
    uint64_t blocks_pushed = 0, dumps = 0;
};

// One production run: its resources, its plan and what the steps of the loop hand to each other.
struct production_run {
    const bf_config& cfg;
    const observation_options& opt;
    std::ostream& log;
    run_resources dev;
    launch_plan plan;
    // beam_out: the reference's pinned D2H destination (:249), [stream][beam_out_stride]; the root of a sharded run receives the whole band there
    const size_t n_f_per_detect = bf_floats_per_detect(&cfg), beam_out_stride = n_f_per_detect * (size_t)(opt.comm ? opt.world : 1);
    float* beam_out = nullptr;
    std::vector<int> timeSlice = std::vector<int>((size_t)cfg.n_streams);              // :319
    std::vector<long long> last_gemm = std::vector<long long>((size_t)cfg.n_streams, -1);   // the gemm-unit beam_out[q] ends up holding
    std::vector<float*> unit_dst;         // the D2H destination of every unit of the block being launched
    uint64_t launch_seq = 0, sink_committed = 0;
    std::deque<dm_chunk> dm_pending;      // pushed, not yet delivered (their block's analysis event has not fired)
    std::vector<float*> dm_host;          // pinned chunk buffers, used round robin
    uint64_t dm_seq = 0, dm_times = 0, dm_chunks = 0;
    std::vector<bf_sps_candidate> cands;  // what bf_sps_collect returns for one chunk
    uint64_t sps_candidates = 0;
    bf_evt_options evt_opt{};              // opt.evt with max_width and ib_beam filled in
    std::vector<bf_evt_event> events_out;  // what one feed closes
    std::deque<stamp_want> stamp_pending;  // wanted, not yet cut: new ones, and those answered "not pushed yet"
    float* stamp_host = nullptr;           // pinned: the stamps of one cut
    size_t stamp_batch = 0;                // requests one cut takes
    uint64_t events = 0, stamps = 0, stamps_dropped = 0, stamps_missed = 0, stamps_beyond_end = 0;
    std::deque<vcut_want> vcut_pending;    // wanted, not yet cut: new ones, and those answered "not pushed yet"
    uint8_t* vcut_host = nullptr;          // pinned: the units of one cut
    size_t vcut_batch = 0, vcut_bytes = 0; // requests one cut takes; bytes of one request's units
    uint64_t vcuts = 0, vcuts_dropped = 0, vcuts_missed = 0, vcuts_beyond_end = 0;
    uint64_t psr_rows_folded = 0, psr_dumps = 0;   // the pulsar folder: rows folded since the last dump; dumps delivered
    std::deque<uint64_t> psr_pending;              // the block behind whose last launch each uncollected dump was issued
    uint64_t ffa_times = 0, ffa_segments = 0, ffa_candidates = 0;   // the periodicity search: output times of the delivered chunks; segments collected
    std::vector<bf_ffa_candidate> ffa_cands;
    std::vector<double> psr_prof;
    std::vector<uint64_t> psr_hits;
    float* cond_mask_host = nullptr;      // pinned, whole dwords: where the conditioner's mask of the last push is read back at the end

    // channels the conditioner masked in the last push (-1: no conditioner, or no push)
    int cond_masked_channels()
    {
        const uint8_t* d_mask = nullptr;
        if (!dev.cond || !dm_seq || bf_cond_mask_device(dev.cond, &d_mask) != BF_OK) return -1;
        if (bf_enqueue_d2h(dev.h, 0, reinterpret_cast<const float*>(d_mask), cond_mask_host, ((size_t)plan.n_freq_band + 3) / 4) != BF_OK) return -1;
        if (bf_stream_sync(dev.h, 0) != BF_OK) return -1;
        int n = 0;
        for (int f = 0; f < plan.n_freq_band; f++) n += reinterpret_cast<const uint8_t*>(cond_mask_host)[f] != 0;
        return n;
    }
    accum_tap corr{"Correlator", "visibility", opt.corr_blocks,
                   [this](int n, size_t* n_int64) { *n_int64 = 2 * bf_corr_entries(&cfg); return bf_corr_create(dev.h, n, &dev.corr); },
                   [this](int q, int slot, int first, int n) { return bf_corr_push_block(dev.corr, q, slot, first, n); },
                   [this] { return bf_corr_dump(dev.corr, nullptr); },
                   [this](int64_t* out, uint64_t* n) { return bf_corr_collect(dev.corr, out, n); },
                   [this](uint64_t b, uint64_t n, const int64_t* d, size_t k) { return !opt.vis_sink || opt.vis_sink->deliver(b, n, d, k); }};
    accum_tap sk{"Voltage moments", "moments", opt.sk_blocks,
                 [this](int n, size_t* n_int64) { *n_int64 = 2 * bf_sk_entries(&cfg); return bf_sk_create(dev.h, n, &dev.sk); },
                 [this](int q, int slot, int first, int n) { return bf_sk_push_block(dev.sk, q, slot, first, n); },
                 [this] { return bf_sk_dump(dev.sk, nullptr); },
                 [this](int64_t* out, uint64_t* n) { return bf_sk_collect(dev.sk, out, n); },
                 [this](uint64_t b, uint64_t n, const int64_t* d, size_t k) { return !opt.sk_sink || opt.sk_sink->deliver(b, n, d, k); }};
    accum_tap* const taps[2] = {&corr, &sk};   // in the order they follow the detect launch on its queue
    // the Stokes stage (stokes_beams non-empty): pushes issued and not yet collected -- {block of the launch, its first gemm-unit}
    std::deque<std::pair<uint64_t, uint64_t>> stokes_pending;
    std::vector<int8_t> stokes_weights;   // the host weights the handle got: what the stage's beams are picked from
    std::vector<int64_t> stokes;          // what bf_stokes_collect returns for one push
    uint64_t stokes_units = 0;

    int create_handle_and_weights(const antenna* pos, const beam_direction* dir)
    {
        int rc = bf_create(&cfg, opt.device, &dev.h);
        if (rc != BF_OK) return gpu_error(log, rc);
        if ((rc = dev.alloc_pinned(beam_out_stride * cfg.n_streams, &beam_out)) != BF_OK) return rc;
        ::memset(beam_out, 0, beam_out_stride * cfg.n_streams * sizeof(float));
        std::vector<int8_t> fourier_coefficients((size_t)cfg.n_freq * cfg.n_ant * cfg.n_beams * 2);
        generate_fourier_coefficients(cfg.n_beams, cfg.n_ant, cfg.n_freq, opt.rank * cfg.n_freq, opt.gpu, pos, dir, fourier_coefficients.data());
        const bool follow = !opt.stokes_beams.empty();   // (the Stokes stage takes the weights as they were set: calibrated, in place)
        rc = set_run_weights(dev.h, opt.device, fourier_coefficients, opt.gains, opt.nulls, opt.ant_flags, follow ? fourier_coefficients.data() : nullptr, log);
        if (rc != BF_OK) return rc;
        if (follow) stokes_weights.swap(fourier_coefficients);
        return opt.incoherent_beam >= 0 ? bf_set_incoherent_beam(dev.h, opt.incoherent_beam) : BF_OK;
    }

    int create_dm_stage_and_buffers()
    {
        int rc = BF_OK;
        if (plan.dm_run) {
            // chunks in flight: the launches of MAX_TOTAL_SEP blocks queued + the one being delivered
            const size_t n_buf = (size_t)(kMaxTotalSep + 2) * (size_t)(cfg.n_gemms_per_block / plan.upl);
            int history_rows = 0;
            if (opt.evt && opt.stamp_sink) {   // docs/EVENTS.md section 3: span / 2 + t_tol + max_width + (n_buf + 1) dm_rows
                const int max_width = 1 << (opt.sps_widths - 1), tbin_max = opt.stamp_tbin ? opt.stamp_tbin : std::max(1, max_width / 2);
                history_rows = opt.stamp_bins * tbin_max / 2 + opt.evt->t_tol + max_width + (int)(n_buf + 1) * plan.dm_rows;
            }
            rc = bf_dm_stream_create_history(dev.h, opt.dm_delays + (size_t)plan.dm_first * plan.n_freq_band, plan.dm_count, plan.n_freq_band,
                                             plan.dm_rows, history_rows, &dev.dm);
            if (rc != BF_OK) return gpu_error(log, rc);
            if (history_rows) {
                uint64_t oldest = 0, next = 0, cap = 0;
                bf_dm_stream_history(dev.dm, &oldest, &next, &cap);
                log << "Stamps: DM ring of " << cap << " rows (" << ((cap * (uint64_t)plan.n_freq_band * (uint64_t)cfg.n_beams * 4) >> 20) << " MiB), "
                    << history_rows << " of them history" << std::endl;
            }
            for (size_t i = 0; i < n_buf; i++) {
                float* chunk = nullptr;
                if ((rc = dev.alloc_pinned((size_t)plan.dm_count * plan.dm_rows * cfg.n_beams, &chunk)) != BF_OK) return rc;
                dm_host.push_back(chunk);
            }
            if (opt.inj && opt.inj->size()) {   // the injector: in front of the conditioner, on the rows in the stage's buffer (docs/INJECTION.md)
                int max_width = 1;
                for (const inj_plan::burst& b : opt.inj->bursts) max_width = std::max(max_width, b.W);
                for (const inj_plan::train& t : opt.inj->trains) max_width = std::max(max_width, t.n_bins);
                rc = bf_inj_create(dev.h, plan.n_freq_band, plan.dm_rows, (int)opt.inj->size(), max_width, &dev.inj);
                // every pulse before the first push: the bursts' ids first, then the trains'
                for (size_t i = 0; rc == BF_OK && i < opt.inj->bursts.size(); i++) {
                    const inj_plan::burst& b = opt.inj->bursts[i];
                    rc = bf_inj_add_burst(dev.inj, b.t0, b.W, b.delay.data(), b.profile.data(), b.response.data(), nullptr);
                }
                for (size_t i = 0; rc == BF_OK && i < opt.inj->trains.size(); i++) {
                    const inj_plan::train& t = opt.inj->trains[i];
                    rc = bf_inj_add_train(dev.inj, &t.model, t.first_row, t.n_rows, t.n_bins, t.delay.data(), t.profile.data(), t.response.data(), nullptr);
                }
                if (rc == BF_OK) rc = bf_dm_stream_attach_injector(dev.dm, dev.inj);
                if (rc != BF_OK) return gpu_error(log, rc);
            }
            if (opt.cond_baseline > 0) {   // the conditioner: in front of the DM stage, on the rows in its buffer (docs/CONDITIONING.md)
                bf_cond_options co;
                bf_cond_default_options(&co);
                co.baseline_pushes = opt.cond_baseline;
                co.zero_dm = opt.cond_zero_dm ? 1 : 0;
                co.auto_threshold = opt.cond_auto_threshold;
                rc = bf_cond_create(dev.h, plan.n_freq_band, plan.dm_rows, &co, &dev.cond);
                if (rc == BF_OK && opt.cond_mask) rc = bf_cond_set_mask(dev.cond, opt.cond_mask);
                if (rc == BF_OK) rc = bf_dm_stream_attach_conditioner(dev.dm, dev.cond);
                if (rc != BF_OK) return gpu_error(log, rc);
                if ((rc = dev.alloc_pinned(((size_t)plan.n_freq_band + 3) / 4, &cond_mask_host)) != BF_OK) return rc;
            }
            if (opt.n_psr > 0) {   // the pulsar folder: behind the conditioner, on the rows in the stage's buffer (docs/PULSAR_FOLDING.md); a dump per launch at most
                rc = bf_psr_create(dev.h, plan.n_freq_band, plan.dm_rows, opt.psr_bins, opt.psr_models, opt.psr_delays, opt.n_psr, (int)n_buf, &dev.psr);
                if (rc == BF_OK) rc = bf_dm_stream_attach_folder(dev.dm, dev.psr);
                if (rc != BF_OK) return gpu_error(log, rc);
                psr_prof.resize(bf_psr_entries(opt.n_psr, plan.n_freq_band, opt.psr_bins, cfg.n_beams));
                psr_hits.resize(psr_prof.size() / (size_t)cfg.n_beams);
            }
            if (opt.ffa_p_hi > 0) {   // the periodicity search (docs/PERIODICITY.md)
                // a result set for every segment the chunks in flight can complete: at most n_buf chunks of dm_rows times are pushed
                // and not yet delivered, and X times behind a segment in progress complete at most X / seg_rows + 1 segments
                const uint64_t seg_rows = (uint64_t)std::max(opt.ffa_seg, 1) * (uint64_t)std::max(opt.ffa_dec, 1);
                const int in_flight = (int)((uint64_t)n_buf * (uint64_t)plan.dm_rows / seg_rows + 1);
                rc = bf_ffa_create(dev.h, plan.dm_count, plan.dm_first, opt.ffa_dec, opt.ffa_seg, opt.ffa_oct, opt.ffa_p_lo, opt.ffa_p_hi, opt.ffa_widths,
                                   plan.dm_rows, in_flight, opt.ffa_threshold, &dev.ffa);
                if (rc == BF_OK && (opt.ffa_detrend_blk || opt.ffa_detrend_win)) rc = bf_ffa_set_detrend(dev.ffa, opt.ffa_detrend_blk, opt.ffa_detrend_win);
                if (rc == BF_OK) rc = bf_dm_stream_attach_periodicity(dev.dm, dev.ffa);
                if (rc != BF_OK) return gpu_error(log, rc);
                ffa_cands.resize((size_t)plan.dm_count * cfg.n_beams);
            }
            if (opt.sps_widths > 0) {   // the search stage: as many result sets as chunk buffers (a chunk in flight = a search push in flight)
                rc = bf_sps_create(dev.h, plan.dm_count, plan.dm_first, opt.sps_widths, plan.dm_rows, (int)n_buf, /*baseline_pushes=*/8,
                                   /*min_samples=*/64, opt.sps_threshold, &dev.sps);
                if (rc == BF_OK) rc = bf_dm_stream_attach_search(dev.dm, dev.sps);
                if (rc != BF_OK) return gpu_error(log, rc);
                cands.resize((size_t)plan.dm_count * cfg.n_beams);
            }
            if (opt.evt) {
                evt_opt = *opt.evt;
                evt_opt.max_width = 1 << (opt.sps_widths - 1);
                if (evt_opt.ib_beam < 0) evt_opt.ib_beam = opt.incoherent_beam;
                if ((rc = bf_evt_create(&evt_opt, &dev.evt)) != BF_OK) return gpu_error(log, rc);
                if (opt.stamp_sink) {
                    stamp_batch = (size_t)std::max(1, opt.stamp_max_per_deliver);
                    const size_t stamp_floats = (size_t)(plan.n_freq_band / opt.stamp_fbin) * (size_t)opt.stamp_bins;
                    if ((rc = dev.alloc_pinned(stamp_batch * stamp_floats, &stamp_host)) != BF_OK) return rc;
                }
                if (opt.vcut_sink && (rc = create_voltage_history((int)n_buf)) != BF_OK) return rc;
            }
        }
        for (accum_tap* t : taps) {
            if (t->blocks <= 0) continue;
            size_t n_int64 = 0;   // dumps in flight: one per block queued at most, + the one being delivered
            if ((rc = t->create(kMaxTotalSep + 2, &n_int64)) != BF_OK) return gpu_error(log, rc);
            t->host.resize(n_int64);
        }
        if (!opt.stokes_beams.empty()) {   // sets in flight: as the DM chunks -- the launches of the blocks queued + the one being delivered
            const int n_int = opt.stokes_int ? opt.stokes_int : cfg.n_avg, n_sel = (int)opt.stokes_beams.size();
            const int n_sets = (kMaxTotalSep + 2) * (cfg.n_gemms_per_block / plan.upl);
            // The C-ABI sizes every set for a whole block, on the device and again pinned: small launches multiply that.  Reported, and
            // refused beyond kStokesSetBytesMax per side before anything is allocated.
            const size_t set_bytes = (size_t)cfg.n_gemms_per_block * bf_stokes_entries(&cfg, n_sel, n_int) * 4 * sizeof(int64_t);
            log << "Stokes beams: " << n_sets << " result sets of " << (set_bytes >> 20) << " MiB, on the device and pinned" << std::endl;
            if ((size_t)n_sets * set_bytes > kStokesSetBytesMax) {
                log << "ERROR: the Stokes result sets exceed " << (kStokesSetBytesMax >> 30) << " GiB per side" << std::endl;
                return set_error(BF_ERR_INVALID, "run_observation: the Stokes result sets (sets in flight x a block of entries) exceed 8 GiB on the device "
                                                 "and pinned: fewer stokes_beams, a longer stokes_int or more units_per_launch");
            }
            if ((rc = bf_stokes_create(dev.h, n_int, n_sets, &dev.stokes)) != BF_OK) return gpu_error(log, rc);
            if ((rc = bf_stokes_set_weights(dev.stokes, stokes_weights.data(), opt.stokes_beams.data(), n_sel)) != BF_OK) return gpu_error(log, rc);
            stokes.resize(4 * (size_t)plan.upl * bf_stokes_entries(&cfg, n_sel, n_int));
            std::vector<int8_t>().swap(stokes_weights);
        }
        if (plan.block_launch)   // the per-queue block buffers are allocated on first use: do that here, not inside the timed loop
            for (int q = 0; q < plan.n_queues_used; q++) {
                float* unused = nullptr;
                if ((!plan.dm_run || opt.comm) && (rc = bf_block_output_device(dev.h, q, &unused)) != BF_OK) return rc;   // (a DM stage takes the rows itself)
                if (opt.comm && plan.is_root && !plan.dm_run && (rc = bf_block_gather_device(dev.h, q, opt.world, &unused)) != BF_OK) return rc;
                if (opt.comm && plan.staged && plan.is_root && (rc = bf_block_gather_stage_device(dev.h, q, opt.world, &unused)) != BF_OK) return rc;
            }
        return BF_OK;
    }

    // The voltage history (docs/VOLTAGE_CUTS.md): the delay table is the DM stage's row delays of this rank's trials in samples -- the
    // ladder of the detected stream, nothing finer -- and the ring what bf_vhist_units_needed says, unless the caller sizes it.
    int create_voltage_history(int n_buf)
    {
        const size_t n_del = (size_t)plan.dm_count * (size_t)cfg.n_freq;
        std::vector<int32_t> delays(n_del);
        const int32_t* rows = opt.dm_delays + (size_t)plan.dm_first * plan.n_freq_band;
        for (size_t i = 0; i < n_del; i++) delays[i] = rows[i] * cfg.n_avg;
        const int max_width = 1 << (opt.sps_widths - 1);
        const int units = opt.vcut_history_units
                              ? opt.vcut_history_units
                              : bf_vhist_units_needed(&cfg, bf_dm_stream_max_delay(dev.dm), plan.dm_rows, n_buf, opt.evt->t_tol, max_width, opt.vcut_units);
        int rc = bf_vhist_create(dev.h, delays.data(), plan.dm_count, units, &dev.vhist);
        if (rc != BF_OK) return gpu_error(log, rc);
        uint64_t oldest = 0, next = 0, cap = 0;
        bf_vhist_history(dev.vhist, &oldest, &next, &cap);
        vcut_bytes = (size_t)opt.vcut_units * (size_t)bf_bytes_per_gemm(&cfg);
        log << "Voltage cuts: history of " << cap << " gemm-units (" << ((cap * (uint64_t)bf_bytes_per_gemm(&cfg)) >> 20) << " MiB), cuts of " << opt.vcut_units
            << " units" << std::endl;
        vcut_batch = (size_t)std::max(1, opt.vcut_max_per_deliver);
        float* p = nullptr;
        if ((rc = dev.alloc_pinned((vcut_batch * vcut_bytes + 3) / 4, &p)) != BF_OK) return rc;
        vcut_host = reinterpret_cast<uint8_t*>(p);
        return BF_OK;
    }

    // :378-401: the next block of the source to its slot of the device ring, or the end of the observation
    int transfer_block(observation_loop_state& obs_state, block_source& source, size_t block_bytes)
    {
        char* block = source.read();             // :384
        if (!source.check_transfers_complete()) {  // :386
            const int rc = bf_submit_block(dev.h, (int)obs_state.get_next_gpu_transfer_block(), block, block_bytes, nullptr);  // :389-393
            if (rc != BF_OK) return gpu_error(log, rc);
            obs_state.generate_transfer_event();  // :396
            if (source.close_releases_block())      // not in the reference: see block_source::close_releases_block
                while (obs_state.status() == BF_OK && obs_state.get_blocks_transferred() < obs_state.get_blocks_transfer_queue())
                    obs_state.check_transfer_events();
        } else {
            obs_state.set_transfers_complete(true);  // :398
        }
        source.close();  // :401
        return BF_OK;
    }

    // unit gemm_index's powers go to its sink slot, or to `fallback`; nullptr (logged): the sink is full
    float* unit_destination(float* fallback, uint64_t gemm_index)
    {
        if (!opt.sink) return fallback;
        float* slot = opt.sink->acquire(gemm_index);
        if (!slot) log << "ERROR: detected sink has no free slot" << std::endl;
        return slot;
    }

    // :452-519: the launches of the block at the head of the analysis queue, in the plan's pattern
    int analyse_block(const observation_loop_state& obs_state)
    {
        const int n_units = cfg.n_gemms_per_block;
        const long long block_index = (long long)obs_state.get_blocks_analysis_queue();
        const int gpu_block = (int)obs_state.get_next_gpu_analysis_block();
        if (!plan.block_launch)   // the reference's launch pattern; beam_out[st] is the reference's destination, :485-488
            return enqueue_block_by_units(dev.h, cfg, gpu_block, timeSlice, log, nullptr, [&](int st, int unit) {
                last_gemm[st] = block_index * n_units + unit;
                return unit_destination(&beam_out[(size_t)st * n_f_per_detect], (uint64_t)last_gemm[st]);
            });
        unit_dst.assign((size_t)n_units, nullptr);
        for (int first = 0; first < n_units; first += plan.upl)
            if (const int rc = launch_units(block_index, gpu_block, first)) return rc;
        for (accum_tap* t : taps)
            if (t->blocks > 0 && ++t->blocks_pushed % (uint64_t)t->blocks == 0) {   // the integration is complete: snapshot and zero
                if (const int rc = t->dump()) return gpu_error(log, rc);
                t->pending.emplace_back((uint64_t)block_index + 1 - (uint64_t)t->blocks, (uint64_t)block_index);
            }
        return BF_OK;
    }

    // One block launch over the gemm-units [first, first + upl) of the block, with everything that follows it on its queue.
    int launch_units(long long block_index, int gpu_block, int first)
    {
        const int n_units = cfg.n_gemms_per_block, upl = plan.upl;
        const int q = (int)(launch_seq++ % (uint64_t)plan.n_queues_used);   // (why these queues: resolve_plan)
        // unit u's powers go to its sink slot, or to beam_out[queue of its launch] (later units on that queue
        // overwrite earlier ones, in order: beam_out[q] ends up holding gemm-unit last_gemm[q])
        for (int u = first; u < first + upl; u++) {
            unit_dst[u] = unit_destination(&beam_out[(size_t)q * beam_out_stride], (uint64_t)block_index * n_units + u);
            if (!unit_dst[u]) return BF_ERR_STATE;
            last_gemm[q] = block_index * n_units + u;
        }
        // The DM stage owns the place its rows belong in -- directly behind its carried-over delay window: the beamformer
        // (one GPU) or the gather (a holder of a sharded run) writes them THERE, and the push below only launches.  The
        // reference's collapse reads what detect wrote, no copy in between (src/beamformer.cu:481,492-511).
        float* d_rows = nullptr;     // where this launch's beam-blocks are on the device, [row][freq (over the band)][beam]
        void* dm_qs = nullptr;
        int rc = BF_OK;
        if (plan.dm_run && (rc = bf_queue_stream(dev.h, q, &dm_qs)) == BF_OK) rc = bf_dm_stream_reserve(dev.dm, plan.dm_rows, &d_rows, dm_qs);
        if (rc == BF_OK)
            rc = (plan.dm_run && !opt.comm) ? bf_enqueue_block_to(dev.h, q, gpu_block, first, upl, d_rows, &unit_dst[first])
                                            : bf_enqueue_block(dev.h, q, gpu_block, first, upl, opt.comm ? nullptr : &unit_dst[first]);
        if (rc == BF_OK && opt.comm) rc = gather_block(q, d_rows);
        if (rc == BF_OK && plan.dm_run) rc = push_dm_rows(block_index, d_rows, dm_qs);
        // the correlator reads the same resident units on the same queue, behind the detect launch and what follows it; so do the voltage moments
        for (accum_tap* t : taps)
            if (rc == BF_OK && t->blocks > 0) rc = t->push_block(q, gpu_block, first, upl);
        if (rc == BF_OK && dev.stokes) {   // and the Stokes beams, one set per launch
            rc = bf_stokes_push_block(dev.stokes, q, gpu_block, first, upl);
            if (rc == BF_OK) stokes_pending.emplace_back((uint64_t)block_index, (uint64_t)block_index * (uint64_t)n_units + (uint64_t)first);
        }
        if (rc == BF_OK && dev.vhist) rc = bf_vhist_push_block(dev.vhist, q, gpu_block, first, upl);   // and the voltage history: a device copy of the units
        return rc == BF_OK ? BF_OK : gpu_error(log, rc);
    }

    // sharded (upl == n_units): bring the shards' powers together on the root, in [unit][o][f over the band][b], behind the launch on
    // the same queue; only the root copies to the host
    int gather_block(int q, float* d_rows)
    {
        const int n_units = cfg.n_gemms_per_block;
        float *d_blk = nullptr, *d_full = nullptr, *d_stage = nullptr;
        void* qs = nullptr;
        const size_t full_det = n_f_per_detect * (size_t)opt.world;
        const size_t rows = (size_t)n_units * cfg.n_out_per_gemm, row_floats = (size_t)cfg.n_freq * cfg.n_beams;
        const bool root = plan.is_root;
        if (plan.dm_run) d_full = d_rows;     // (a holder with a DM stage receives straight into the stage's buffer)
        int rc = bf_block_output_device(dev.h, q, &d_blk);
        if (rc == BF_OK) rc = bf_queue_stream(dev.h, q, &qs);
        if (rc == BF_OK && root && !plan.dm_run) rc = bf_block_gather_device(dev.h, q, opt.world, &d_full);
        if (rc == BF_OK && root && plan.staged) rc = bf_block_gather_stage_device(dev.h, q, opt.world, &d_stage);
        if (rc == BF_OK)
            rc = plan.staged ? bf_gather_detected_staged(opt.comm, d_blk, rows, row_floats, opt.gather_root, d_full, d_stage, qs)
                             : bf_gather_detected(opt.comm, d_blk, rows, row_floats, opt.gather_root, BF_GATHER_LAYOUT_FREQ_MAJOR, d_full, qs);
        for (int u = 0; rc == BF_OK && root && u < n_units; u++)
            rc = bf_enqueue_d2h(dev.h, q, d_full + full_det * (size_t)u, unit_dst[u], full_det);
        return rc;
    }

    // the DM stage, where the reference's loop collapses frequency (src/beamformer.cu:492-511): this launch's rows are in the stream's
    // buffer already; its kernels run on the launch's own queue, the chunk that becomes complete travels to a pinned buffer
    int push_dm_rows(long long block_index, float* d_rows, void* dm_qs)
    {
        uint64_t first_t = 0;
        int n_t = 0;
        float* chunk = dm_host[(size_t)(dm_seq++ % dm_host.size())];
        int rc = bf_dm_stream_push(dev.dm, d_rows, plan.dm_rows, chunk, &first_t, &n_t, dm_qs);
        if (rc == BF_OK && n_t > 0) dm_pending.push_back({(uint64_t)block_index, first_t, n_t, chunk});
        if (rc == BF_OK && dev.psr && (psr_rows_folded += (uint64_t)plan.dm_rows) >= (uint64_t)opt.psr_dump_rows) {   // the attached folder has folded these rows
            rc = bf_psr_dump(dev.psr, dm_qs);
            psr_pending.push_back((uint64_t)block_index);
            psr_rows_folded = 0;
        }
        return rc;
    }

    // The events one feed (or the flush) closed: to the sink; then the stamps that are wanted of them -- unflagged ones unless
    // stamp_flagged, by snr descending, then event order, at most stamp_max_per_deliver; the rest are counted as dropped.
    int take_events(size_t n)
    {
        events += n;
        if (opt.event_sink && n && !opt.event_sink->deliver(events_out.data(), n)) {
            log << "ERROR: event sink failed" << std::endl;
            return BF_ERR_STATE;
        }
        if (opt.vcut_sink) want_voltage_cuts(n);
        if (!opt.stamp_sink) return BF_OK;
        std::vector<size_t> pick;
        for (size_t i = 0; i < n; i++)
            if (opt.stamp_flagged || !events_out[i].flags) pick.push_back(i);
        std::stable_sort(pick.begin(), pick.end(), [&](size_t a, size_t b) { return events_out[a].best.snr > events_out[b].best.snr; });
        const size_t cap = (size_t)opt.stamp_max_per_deliver;
        if (pick.size() > cap) {
            stamps_dropped += pick.size() - cap;
            pick.resize(cap);
        }
        for (size_t i : pick) {
            const bf_sps_candidate& b = events_out[i].best;
            const int tbin = opt.stamp_tbin ? opt.stamp_tbin : std::max(1, b.width / 2);
            const uint64_t centre = b.t_start + (uint64_t)(b.width / 2), half = (uint64_t)opt.stamp_bins * (uint64_t)tbin / 2;
            stamp_pending.push_back({{centre > half ? centre - half : 0, b.dm - plan.dm_first, b.beam}, tbin, b.width, b.dm, b.snr});
        }
        return BF_OK;
    }

    // The stamps' selection rule for the voltage cuts of one feed's events: unflagged ones unless vcut_flagged, by snr descending, then
    // event order, at most vcut_max_per_deliver; the rest are counted as dropped.  vcut_units units centred on the best member.
    void want_voltage_cuts(size_t n)
    {
        std::vector<size_t> pick;
        for (size_t i = 0; i < n; i++)
            if (opt.vcut_flagged || !events_out[i].flags) pick.push_back(i);
        std::stable_sort(pick.begin(), pick.end(), [&](size_t a, size_t b) { return events_out[a].best.snr > events_out[b].best.snr; });
        const size_t cap = (size_t)opt.vcut_max_per_deliver;
        if (pick.size() > cap) {
            vcuts_dropped += pick.size() - cap;
            pick.resize(cap);
        }
        const uint64_t S = (uint64_t)cfg.n_out_per_gemm * (uint64_t)cfg.n_avg;
        for (size_t i : pick) {
            const bf_sps_candidate& b = events_out[i].best;
            const uint64_t centre = (b.t_start + (uint64_t)(b.width / 2)) * (uint64_t)cfg.n_avg, half = (uint64_t)opt.vcut_units * S / 2;
            vcut_pending.push_back({{centre > half ? centre - half : 0, b.dm - plan.dm_first, 0}, b.beam, b.width, b.dm, b.snr});
        }
    }

    // One round of voltage cuts over everything pending (vcut_batch requests at most per call): as cut_stamps.
    int cut_voltages(bool last)
    {
        std::deque<vcut_want> todo;
        todo.swap(vcut_pending);
        while (!todo.empty()) {
            std::vector<vcut_want> group;
            while (!todo.empty() && group.size() < vcut_batch) {
                group.push_back(todo.front());
                todo.pop_front();
            }
            std::vector<bf_vcut_request> rq;
            for (const vcut_want& w : group) rq.push_back(w.rq);
            std::vector<int32_t> status(group.size(), -1);
            const int rc = bf_vhist_cut_host(dev.vhist, rq.data(), (int)rq.size(), opt.vcut_units, vcut_host, status.data());
            if (rc != BF_OK) return gpu_error(log, rc);
            for (size_t i = 0; i < group.size(); i++) {
                const vcut_want& w = group[i];
                if (status[i] == 2) {   // not pushed yet: retried at the next deliver -- or, at the end of the run, never there
                    if (last) vcuts_beyond_end++; else vcut_pending.push_back(w);
                } else if (status[i] == 1) {
                    vcuts_missed++;
                } else {
                    vcuts++;
                    if (!opt.vcut_sink->deliver(w.rq.t0, w.dm_global, w.beam, w.width, w.snr, vcut_host + i * vcut_bytes, vcut_bytes)) {
                        log << "ERROR: voltage sink failed at sample " << w.rq.t0 << std::endl;
                        return BF_ERR_STATE;
                    }
                }
            }
        }
        return BF_OK;
    }

    // One round of cuts over everything pending (a call per time binning, stamp_batch requests at most): cut ones go to the sink, those
    // whose rows have left the ring are counted as missed, those not pushed yet stay -- at the end of the run they are counted as
    // beyond it: their window passes the last row the run produced.
    int cut_stamps(bool last)
    {
        if (stamp_pending.empty()) return BF_OK;
        std::deque<stamp_want> todo;
        todo.swap(stamp_pending);
        const int n_freq_out = plan.n_freq_band / opt.stamp_fbin;
        const size_t stamp_floats = (size_t)n_freq_out * (size_t)opt.stamp_bins;
        while (!todo.empty()) {
            const int tbin = todo.front().tbin;
            std::vector<stamp_want> group;
            std::deque<stamp_want> rest;
            for (const stamp_want& w : todo)
                if (w.tbin == tbin && group.size() < stamp_batch) group.push_back(w); else rest.push_back(w);
            todo.swap(rest);
            std::vector<bf_stamp_request> rq;
            for (const stamp_want& w : group) rq.push_back(w.rq);
            std::vector<int32_t> status(group.size(), -1);
            const int rc = bf_dm_stream_cut_host(dev.dm, rq.data(), (int)rq.size(), opt.stamp_bins, tbin, opt.stamp_fbin, stamp_host, status.data());
            if (rc != BF_OK) return gpu_error(log, rc);
            for (size_t i = 0; i < group.size(); i++) {
                const stamp_want& w = group[i];
                if (status[i] == 2) {   // not pushed yet: retried at the next deliver -- or, at the end of the run, never there
                    if (last) stamps_beyond_end++; else stamp_pending.push_back(w);
                } else if (status[i] == 1) {
                    stamps_missed++;
                } else {
                    stamps++;
                    if (!opt.stamp_sink->deliver(w.rq.t0, w.dm_global, w.rq.beam, w.tbin, w.width, w.snr, stamp_host + i * stamp_floats, n_freq_out, opt.stamp_bins)) {
                        log << "ERROR: stamp sink failed at time " << w.rq.t0 << std::endl;
                        return BF_ERR_STATE;
                    }
                }
            }
        }
        return BF_OK;
    }

    // The end of the run: every open cluster closes, and one last round of cuts.
    int flush_events()
    {
        if (!dev.evt) return BF_OK;
        size_t n = 0;
        events_out.resize((size_t)bf_evt_open(dev.evt));
        int rc = bf_evt_flush(dev.evt, events_out.data(), events_out.size(), &n);
        if (rc != BF_OK) return gpu_error(log, rc);
        if ((rc = take_events(n)) != BF_OK) return rc;
        if (opt.vcut_sink && (rc = cut_voltages(/*last=*/true)) != BF_OK) return rc;
        return opt.stamp_sink ? cut_stamps(/*last=*/true) : BF_OK;
    }

    // What the blocks analysed so far finished: their DM chunks have landed (their copies sit on the queues the analysis event joins),
    // and so has every D2H copy of their gemm-units: hand those over, in order.
    int deliver(uint64_t blocks_analyzed)
    {
        while (!dm_pending.empty() && dm_pending.front().block < blocks_analyzed) {
            const dm_chunk c = dm_pending.front();
            dm_pending.pop_front();
            dm_times += (uint64_t)c.n_t;
            if (dev.sps) {   // one search push per chunk, in the same order: its kernels ran on the chunk's queue; the collect waits for its records
                size_t n = 0;
                const int rc = bf_sps_collect(dev.sps, cands.data(), cands.size(), &n);
                if (rc != BF_OK) return gpu_error(log, rc);
                sps_candidates += n;
                if (opt.sps_sink && !opt.sps_sink->deliver(cands.data(), n)) {
                    log << "ERROR: candidate sink failed at output time " << c.first_t << std::endl;
                    return BF_ERR_STATE;
                }
                if (dev.evt) {   // the chunk's candidates (global trial indices) into the builder; what closes goes to the sinks
                    size_t n_ev = 0;
                    events_out.resize((size_t)bf_evt_open(dev.evt) + n);
                    const int rc_e = bf_evt_feed(dev.evt, cands.data(), n, c.first_t + (uint64_t)c.n_t, events_out.data(), events_out.size(), &n_ev);
                    if (rc_e != BF_OK) return gpu_error(log, rc_e);
                    if (int rc_t = take_events(n_ev)) return rc_t;
                }
            }
            if (dev.ffa) {   // the segments this chunk completed: their kernels ran behind the chunk's on its queue; the collect waits for their records
                ffa_times += (uint64_t)c.n_t;
                const uint64_t seg_rows = (uint64_t)opt.ffa_seg * (uint64_t)opt.ffa_dec;
                while (ffa_segments < ffa_times / seg_rows) {
                    size_t n = 0;
                    const int rc = bf_ffa_collect(dev.ffa, ffa_cands.data(), ffa_cands.size(), &n);
                    if (rc != BF_OK) return gpu_error(log, rc);
                    ffa_segments++;
                    ffa_candidates += n;
                    if (opt.ffa_sink && !opt.ffa_sink->deliver(ffa_cands.data(), n)) {
                        log << "ERROR: periodicity sink failed at segment " << ffa_segments - 1 << std::endl;
                        return BF_ERR_STATE;
                    }
                }
            }
            if (!opt.dm_sink) continue;
            dm_chunks++;
            if (!opt.dm_sink->deliver(c.first_t, c.n_t, plan.dm_count, cfg.n_beams, c.host)) {
                log << "ERROR: DM sink failed at output time " << c.first_t << std::endl;
                return BF_ERR_STATE;
            }
        }
        if (opt.stamp_sink)   // one round of cuts per deliver, on the stage's own queue: the compute queues keep running
            if (int rc = cut_stamps(/*last=*/false)) return rc;
        if (opt.vcut_sink)    // and one round of voltage cuts, on the history's own queue
            if (int rc = cut_voltages(/*last=*/false)) return rc;
        for (accum_tap* t : taps)
            while (!t->pending.empty() && t->pending.front().second < blocks_analyzed) {   // (the collect waits for the dump's own copy)
                const uint64_t first_block = t->pending.front().first;
                t->pending.pop_front();
                uint64_t n_columns = 0;
                const int rc = t->collect(t->host.data(), &n_columns);
                if (rc != BF_OK) return gpu_error(log, rc);
                t->dumps++;
                if (!t->deliver(first_block, n_columns, t->host.data(), t->host.size())) {
                    log << "ERROR: " << t->noun << " sink failed at block " << first_block << std::endl;
                    return BF_ERR_STATE;
                }
            }
        while (!psr_pending.empty() && psr_pending.front() < blocks_analyzed) {   // (the collect waits for the dump's own copy)
            psr_pending.pop_front();
            uint64_t first_row = 0, n_rows = 0;
            const int rc = bf_psr_collect(dev.psr, psr_prof.data(), psr_hits.data(), &first_row, &n_rows);
            if (rc != BF_OK) return gpu_error(log, rc);
            psr_dumps++;
            if (opt.psr_sink && !opt.psr_sink->deliver(first_row, n_rows, opt.n_psr, plan.n_freq_band, opt.psr_bins, cfg.n_beams, psr_hits.data(), psr_prof.data())) {
                log << "ERROR: fold sink failed at row " << first_row << std::endl;
                return BF_ERR_STATE;
            }
        }
        while (!stokes_pending.empty() && stokes_pending.front().first < blocks_analyzed) {   // (the collect waits for the set's own copy)
            const uint64_t first_unit = stokes_pending.front().second;
            stokes_pending.pop_front();
            int n = 0;
            const int rc = bf_stokes_collect(dev.stokes, stokes.data(), &n);
            if (rc != BF_OK) return gpu_error(log, rc);
            stokes_units += (uint64_t)n;
            if (opt.stokes_sink && !opt.stokes_sink->deliver(first_unit, (uint64_t)n, stokes.data(), stokes.size())) {
                log << "ERROR: Stokes sink failed at gemm-unit " << first_unit << std::endl;
                return BF_ERR_STATE;
            }
        }
        for (; opt.sink && sink_committed < blocks_analyzed * (uint64_t)cfg.n_gemms_per_block; sink_committed++)
            if (!opt.sink->commit(sink_committed)) {
                log << "ERROR: detected sink failed at gemm-unit " << sink_committed << std::endl;
                return BF_ERR_STATE;
            }
        return BF_OK;
    }
};

}  // namespace

int run_observation(const bf_config& cfg, const observation_options& opt, block_source& source, const antenna* pos,
                    const beam_direction* dir, observation_result* res, std::ostream& log)
{
    setup_gate gate{opt.comm};
    int rc = check_options(cfg, opt);
    if (rc != BF_OK) return gate.fail(rc);
    source.read_headers();  // :334 (before the device exists here: the block-size check below needs no GPU)
    const size_t block_bytes = bf_bytes_per_block(&cfg);
    if (source.get_block_size() != block_bytes) {
        // The reference prints this (src/beamformer.cu:336-339) and carries on; every ring block is then copied with the
        // GEOMETRY's size: a smaller ring block is read past its end (past the mapping on the last one), a larger one is
        // silently truncated.  Neither can produce a meaningful beam: refuse.
        log << "ERROR: block size " << source.get_block_size() << ", Should also be " << block_bytes << std::endl;
        return gate.fail(set_error(BF_ERR_INVALID, "run_observation: the source's block size does not match bf_bytes_per_block(cfg)"));
    }

    production_run run{cfg, opt, log};
    for (int i = 0; i < cfg.n_streams; i++) run.timeSlice[i] = i;  // :319
    if ((rc = run.create_handle_and_weights(pos, dir)) != BF_OK) return gate.fail(rc);
    bf_handle* const h = run.dev.h;
    hip_backend backend(h);
    observation_loop_state obs_state(kMaxTransferSep, kMaxTotalSep, cfg, &backend, /*debug_mode=*/false);  // :322
    if (opt.burn_in > 0) {  // :348-355
        log << "Burning IN" << std::endl;
        for (int i = 0; i < opt.burn_in; i++) {
            source.read();
            source.close();
        }
        log << "Done Burn in" << std::endl;
    }
    if ((rc = resolve_plan(cfg, opt, &run.plan)) != BF_OK) return gate.fail(rc);
    if ((rc = run.create_dm_stage_and_buffers()) != BF_OK) return gate.fail(rc);
    if ((rc = gate.pass(opt.local_setup_ok)) != BF_OK) return rc;

    bf_timer_start(h);  // :358
    while (!obs_state.check_observations_complete()) {  // :364
        if (opt.verbose) log << "##########################################" << std::endl << obs_state << std::endl;
        if (obs_state.check_ready_for_transfer())  // :378
            if ((rc = run.transfer_block(obs_state, source, block_bytes)) != BF_OK) return rc;
        obs_state.check_transfer_events();  // :446
        if (obs_state.check_ready_for_analysis()) {  // :452
            if ((rc = run.analyse_block(obs_state)) != BF_OK) return rc;
            obs_state.generate_analysis_event();  // :525
        }
        obs_state.check_analysis_events();  // :532
        if (obs_state.status() != BF_OK) return event_backend_error(log, obs_state);
        if ((rc = run.deliver(obs_state.get_blocks_analyzed())) != BF_OK) return rc;
    }
    float ms = 0;
    bf_timer_stop(h, &ms);
    bf_stream_sync(h, -1);  // :560-562
    if ((rc = run.flush_events()) != BF_OK) return rc;
    if (opt.event_sink) opt.event_sink->close();
    if (opt.stamp_sink) opt.stamp_sink->close();
    if (opt.vcut_sink) opt.vcut_sink->close();
    if (opt.sink) opt.sink->close();
    if (opt.dm_sink) opt.dm_sink->close();
    if (opt.sps_sink) opt.sps_sink->close();
    if (opt.vis_sink) opt.vis_sink->close();
    if (opt.sk_sink) opt.sk_sink->close();
    if (opt.stokes_sink) opt.stokes_sink->close();
    if (opt.psr_sink) opt.psr_sink->close();
    if (opt.ffa_sink) opt.ffa_sink->close();
    const uint64_t chunks = obs_state.get_current_transfer_gemm() * cfg.n_out_per_gemm;  // :552
    const double rate = (double)source.get_block_size() * obs_state.get_blocks_transfer_queue() / ms / 1e6;  // :554
    closing_report(log, ms, chunks, ms / (chunks ? chunks : 1), rate, run.plan.block_launch ? "bf_enqueue_block" : kUnitLaunchPattern);
    if (res) {
        res->observation_time_ms = ms;
        res->blocks = obs_state.get_blocks_analyzed();
        res->data_chunks = chunks;
        res->gbytes_per_s = rate;
        res->beam_out.assign(run.beam_out, run.beam_out + run.beam_out_stride * cfg.n_streams);
        res->last_gemm = run.last_gemm;
        res->dm_times = run.dm_times;
        res->dm_chunks = run.dm_chunks;
        res->sps_candidates = run.sps_candidates;
        res->events = run.events;
        res->stamps = run.stamps;
        res->stamps_dropped = run.stamps_dropped;
        res->stamps_missed = run.stamps_missed;
        res->stamps_beyond_end = run.stamps_beyond_end;
        res->vcuts = run.vcuts;
        res->vcuts_dropped = run.vcuts_dropped;
        res->vcuts_missed = run.vcuts_missed;
        res->vcuts_beyond_end = run.vcuts_beyond_end;
        res->vis_dumps = run.corr.dumps;
        res->sk_dumps = run.sk.dumps;
        res->stokes_units = run.stokes_units;
        res->psr_dumps = run.psr_dumps;
        res->inj_pulses = run.dev.inj ? (uint64_t)opt.inj->size() : 0;
        res->ffa_segments = run.ffa_segments;
        res->ffa_candidates = run.ffa_candidates;
        res->cond_masked = run.cond_masked_channels();
    }
    if (run.plan.dm_run)
        log << "DM stage: trials " << run.plan.dm_first << " .. " << run.plan.dm_first + run.plan.dm_count - 1 << " of " << opt.n_dm << ", "
            << run.dm_times << " output times (largest delay " << bf_dm_stream_max_delay(run.dev.dm) << " samples carried over on the device)"
            << std::endl;
    if (run.dev.cond) {
        log << "Conditioner: window of " << opt.cond_baseline << " pushes, zero-DM " << (opt.cond_zero_dm ? "on" : "off") << ", automatic mask ";
        if (opt.cond_auto_threshold > 0.0)
            log << "at " << opt.cond_auto_threshold << " deviations";
        else
            log << "off";
        log << std::endl;
        if (opt.verbose) log << "Conditioner: " << run.cond_masked_channels() << " of " << run.plan.n_freq_band << " channels masked in the last push" << std::endl;
    }
    if (opt.incoherent_beam >= 0) log << "Incoherent beam: in beam column " << opt.incoherent_beam << " of the detected stream" << std::endl;
    for (const accum_tap* t : run.taps)
        if (t->blocks > 0)
            log << t->title << ": " << t->dumps << " dumps of " << t->blocks << " blocks each (an incomplete integration at the end is dropped)" << std::endl;
    if (run.dev.stokes)
        log << "Stokes beams: " << opt.stokes_beams.size() << " beams, windows of " << (opt.stokes_int ? opt.stokes_int : cfg.n_avg) << " samples, "
            << run.stokes_units << " gemm-units" << std::endl;
    if (run.dev.inj)
        log << "Injector: " << opt.inj->bursts.size() << " bursts and " << opt.inj->trains.size() << " trains added to the rows in front of the DM stage, "
            << bf_inj_launches(run.dev.inj) << " kernels launched" << std::endl;
    if (run.dev.psr)
        log << "Pulsar folder: " << opt.n_psr << " pulsars, " << opt.psr_bins << " bins, " << run.psr_dumps << " dumps of at least " << opt.psr_dump_rows
            << " rows each (an incomplete integration at the end is dropped)" << std::endl;
    if (run.dev.ffa)
        log << "Periodicity search: periods " << opt.ffa_p_lo << " .. " << opt.ffa_p_hi - 1 << " samples x " << opt.ffa_oct << " octaves at decimation "
            << opt.ffa_dec << ", " << run.ffa_segments << " segments of " << opt.ffa_seg << " samples, " << run.ffa_candidates << " candidates at S/N >= "
            << opt.ffa_threshold << " (an incomplete segment at the end is dropped)" << std::endl;
    if (run.dev.sps)
        log << "Single-pulse search: boxcar widths 1 .. " << (1 << (opt.sps_widths - 1)) << ", " << run.sps_candidates << " candidates at S/N >= "
            << opt.sps_threshold << std::endl;
    if (run.dev.evt) {
        log << "Events: " << run.events << " events";
        if (opt.stamp_sink)
            log << ", stamps " << run.stamps << ", stamps_dropped " << run.stamps_dropped << ", stamps_missed " << run.stamps_missed
                << ", beyond the end of the run " << run.stamps_beyond_end;
        log << std::endl;
    }
    if (run.dev.vhist)
        log << "Voltage cuts: " << run.vcuts << " cuts of " << opt.vcut_units << " gemm-units, vcuts_dropped " << run.vcuts_dropped << ", vcuts_missed "
            << run.vcuts_missed << ", beyond the end of the run " << run.vcuts_beyond_end << std::endl;
    return BF_OK;
}

}  // namespace dsabf
