// bf_loop_internal.h -- what the two loops of the host mirror share (bf_run_debug.cpp, bf_run_observation.cpp; defined in
// bf_obs_state.cpp).  Host-only, not installed, not part of the ABI: no .hip file includes it.
#pragma once
#include <functional>
#include <ostream>
#include <vector>

#include "../../include/dsabf_host.hpp"

namespace dsabf {

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

// The handle of a run and what it holds in pinned memory.  Released in this order: sync, the pinned buffers in the order they were
// allocated, the handle.  (A loop with stages on the handle destroys those first, behind a sync of its own.)
struct run_device {
    bf_handle* h = nullptr;
    std::vector<void*> pinned;
    ~run_device()
    {
        if (h) bf_stream_sync(h, -1);
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

int gpu_error(std::ostream& log, int rc);
int set_run_weights(bf_handle* h, int device, const std::vector<int8_t>& w, const double* gains, const null_vectors* nulls, const uint8_t* ant_flags,
                    int8_t* w_set, std::ostream& log);
int enqueue_block_by_units(bf_handle* h, const bf_config& cfg, int gpu_block, std::vector<int>& timeSlice, std::ostream& log,
                           const std::function<int(int st, int unit)>& after, const std::function<float*(int st, int unit)>& dst);
void closing_report(std::ostream& log, float ms, uint64_t chunks, float ms_per_chunk, double gbytes_per_s, const char* launch_pattern);
extern const char* const kUnitLaunchPattern;
int event_backend_error(std::ostream& log, const observation_loop_state& obs_state);

}  // namespace dsabf
