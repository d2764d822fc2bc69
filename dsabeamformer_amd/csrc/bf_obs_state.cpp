// bf_obs_state.cpp -- host mirror, part 3: observation_loop_state (src/observation_loop.hh:1-177) on an
// event backend, and what the two branches of the reference's main loop (src/beamformer.cu:364-534) share: run_debug_observation
// (DEBUG, bf_run_debug.cpp) and run_observation (production, bf_run_observation.cpp).
#include <algorithm>
#include <cstring>
#include <iostream>

#include "../../include/dsabf_host.h"
#include "bf_host_internal.h"
#include "bf_loop_internal.h"

namespace dsabf {

// ---- event backends (hip_backend: bf_loop_internal.h) -------------------------------------------------------------
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

// ---- what the two loops share (bf_loop_internal.h) -------------------------------------------------------------------------
// The reference dies inside gpuErrchk with this line (src/beamformer.cuh:19-29); the loops print it and return the code.
int gpu_error(std::ostream& log, int rc)
{
    log << "GPUassert: " << bf_last_error() << std::endl;
    return rc;
}

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

}  // namespace dsabf
