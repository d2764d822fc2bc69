// bf_corr.cpp -- the correlator (include/dsabf.h: bf_correlate_device, bf_corr_*; contract and measurements: docs/CORRELATOR.md).
// The device code is csrc/corr/bf_corr.hip; this file checks the bounds, owns a stage's accumulator and orders its pushes and dumps.
#include <cstring>
#include <new>

#include "bf_runtime_internal.h"
#include "corr/bf_corr_kernels.h"

struct bf_corr : bf_stage {
    bf_corr() : bf_stage("correlator stage") {}
    int max_in_flight = 0;
    size_t n_int64 = 0;                // 2 * bf_corr_entries
    long long* d_acc = nullptr;        // the integration in progress: every push adds to it, a dump copies it out and zeroes it
    uint64_t columns = 0;              // columns per polarisation pushed since the last dump
    // Pushes and dumps share d_acc, so each waits for the one before it, whatever queue that was issued on: `last` is the event
    // behind the most recent kernel (push_done, two taking turns) or behind the most recent dump's copy and memset (its set's).
    hipEvent_t push_done[2] = {nullptr, nullptr};
    hipEvent_t last = nullptr;
    uint64_t n_push = 0;
    struct result_set {
        long long* h_vis = nullptr;    // pinned
        hipEvent_t copied = nullptr;
        uint64_t columns = 0;
    };
    std::vector<result_set> sets;      // dump j leaves its snapshot in set j % max_in_flight
    hipStream_t copy_q = nullptr;
    uint64_t n_dump = 0, n_collected = 0;
};

// The bounds of one launch (include/dsabf.h): n_ant <= 256, fewer than 2^24 columns per polarisation.
static int check_launch(const bf_handle* h, int n_units, const char* who)
{
    if (n_units <= 0) return fail(BF_ERR_INVALID, "%s: n_units must be positive", who);
    if (h->cfg.n_ant > dsabf::kCorrMaxAnt)
        return fail(BF_ERR_INVALID, "%s: %d antennas; the correlator is defined up to %d (the output grows as n_ant^2)", who, h->cfg.n_ant,
                    dsabf::kCorrMaxAnt);
    const long long n = (long long)n_units * h->cfg.n_out_per_gemm * h->cfg.n_avg;
    if (n > dsabf::kCorrMaxColumns)
        return fail(BF_ERR_INVALID, "%s: %lld columns per polarisation in one call; the sums of a call are exact below 2^24 (128 * N <= 2^31 - 1)",
                    who, n);
    return BF_OK;
}

static int launch(bf_handle* h, const void* d_packed, int n_units, long long* d_vis, bool accumulate, hipStream_t q)
{
    HIP_TRY(dsabf::launch_correlate(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_pol, h->cfg.n_out_per_gemm * h->cfg.n_avg, d_packed, n_units, d_vis,
                                    accumulate, q));
    return BF_OK;
}

// One push of a stage, already checked: behind whatever used the accumulator last, and the new end of that chain.
static int push_impl(bf_corr* c, const void* d_packed, int n_units, hipStream_t q)
{
    bf_handle* h = c->h;
    if (c->last) HIP_TRY(hipStreamWaitEvent(q, c->last, 0));
    if (int rc = launch(h, d_packed, n_units, c->d_acc, true, q)) return rc;
    hipEvent_t ev = c->push_done[c->n_push++ % 2];
    HIP_TRY(hipEventRecord(ev, q));
    c->last = ev;
    c->columns += (uint64_t)n_units * (uint64_t)h->cfg.n_out_per_gemm * (uint64_t)h->cfg.n_avg;
    return BF_OK;
}

extern "C" {

size_t bf_corr_entries(const bf_config* cfg)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_pol <= 0 || cfg->n_ant <= 0) return 0;
    return (size_t)cfg->n_freq * (size_t)cfg->n_pol * dsabf::corr_baselines(cfg->n_ant);
}

int bf_correlate_device(bf_handle* h, const void* d_packed, int n_units, int64_t* d_vis, int accumulate, void* hip_stream)
{
    if (!h || !d_packed || !d_vis) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_launch(h, n_units, "bf_correlate_device")) return rc;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_vis & 7))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned, d_vis 8-byte aligned");
    ON_DEVICE(h);
    return launch(h, d_packed, n_units, (long long*)d_vis, accumulate != 0, as_stream(hip_stream));
}

int bf_corr_create(bf_handle* h, int max_in_flight, bf_corr** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h) return fail(BF_ERR_INVALID, "bf_corr_create: the handle is NULL");
    if (max_in_flight <= 0) return fail(BF_ERR_INVALID, "bf_corr_create: max_in_flight must be positive");
    if (h->cfg.n_ant > dsabf::kCorrMaxAnt)
        return fail(BF_ERR_INVALID, "bf_corr_create: %d antennas; the correlator is defined up to %d", h->cfg.n_ant, dsabf::kCorrMaxAnt);
    ON_DEVICE(h);
    bf_corr* c = new (std::nothrow) bf_corr();
    if (!c) return fail(BF_ERR_DEVICE, "out of host memory");
    c->h = h;
    c->max_in_flight = max_in_flight;
    c->n_int64 = 2 * bf_corr_entries(&h->cfg);
    const size_t bytes = c->n_int64 * sizeof(long long);
    bf_resources& res = c->res;
    res.dev(&c->d_acc, bytes, true);
    res.queue(&c->copy_q);
    for (auto& ev : c->push_done) res.event(&ev);
    c->sets.resize((size_t)max_in_flight);
    for (auto& r : c->sets) {
        res.host(&r.h_vis, bytes);
        res.event(&r.copied);
    }
    res.device_sync();
    if (int rc = stage_adopt(c, "bf_corr_create")) return rc;
    *out = c;
    return BF_OK;
}

int bf_corr_destroy(bf_corr* c) { return stage_destroy(c); }

int bf_corr_pending(const bf_corr* c) { return c ? (int)(c->n_dump - c->n_collected) : fail(BF_ERR_INVALID, "the stage is NULL"); }

int bf_corr_push(bf_corr* c, const void* d_packed, int n_units, void* hip_stream)
{
    if (!c || !d_packed) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(c)) return rc;
    if (int rc = check_launch(c->h, n_units, "bf_corr_push")) return rc;
    if ((uintptr_t)d_packed & 15) return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned");
    ON_DEVICE(c->h);
    return push_impl(c, d_packed, n_units, as_stream(hip_stream));
}

int bf_corr_push_block(bf_corr* c, int stream_idx, int slot, int first_unit, int n_units)
{
    if (!c) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(c)) return rc;
    bf_handle* h = c->h;
    if (stream_idx < 0 || stream_idx >= h->cfg.n_streams) return fail(BF_ERR_INVALID, "stream %d out of range", stream_idx);
    if (slot < 0 || slot >= h->cfg.n_blocks_on_gpu) return fail(BF_ERR_INVALID, "slot %d out of range", slot);
    if (first_unit < 0 || n_units <= 0 || first_unit + n_units > h->cfg.n_gemms_per_block)
        return fail(BF_ERR_INVALID, "gemm-units [%d, %d) are not inside a block of %d", first_unit, first_unit + n_units, h->cfg.n_gemms_per_block);
    if (int rc = check_launch(h, n_units, "bf_corr_push_block")) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);   // the push is ordered on queue stream_idx: nothing of the handle's may still be only queued
    const uint8_t* in = h->d_data + bf_bytes_per_gemm(&h->cfg) * ((size_t)h->cfg.n_gemms_per_block * slot + first_unit);
    return push_impl(c, in, n_units, h->streams[stream_idx]);
}

int bf_corr_dump(bf_corr* c, void* hip_stream)
{
    (void)hip_stream;   // the dump never holds the caller's queue: it is ordered by the stage's own chain
    if (!c) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(c)) return rc;
    if (c->n_dump - c->n_collected >= (uint64_t)c->max_in_flight)
        return fail(BF_ERR_STATE, "bf_corr_dump: %d dumps are uncollected (max_in_flight): bf_corr_collect first", c->max_in_flight);
    ON_DEVICE(c->h);
    bf_corr::result_set& r = c->sets[c->n_dump % c->max_in_flight];
    if (c->last) HIP_TRY(hipStreamWaitEvent(c->copy_q, c->last, 0));
    const size_t bytes = c->n_int64 * sizeof(long long);
    HIP_TRY(hipMemcpyAsync(r.h_vis, c->d_acc, bytes, hipMemcpyDeviceToHost, c->copy_q));
    HIP_TRY(hipMemsetAsync(c->d_acc, 0, bytes, c->copy_q));
    HIP_TRY(hipEventRecord(r.copied, c->copy_q));
    c->last = r.copied;
    r.columns = c->columns;
    c->columns = 0;
    c->n_dump++;
    return BF_OK;
}

int bf_corr_collect(bf_corr* c, int64_t* out, uint64_t* n_columns_per_pol)
{
    if (!c || !out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(c)) return rc;
    if (c->n_collected == c->n_dump) return fail(BF_ERR_STATE, "bf_corr_collect: no dump is pending");
    ON_DEVICE(c->h);
    bf_corr::result_set& r = c->sets[c->n_collected % c->max_in_flight];
    HIP_TRY(hipEventSynchronize(r.copied));
    std::memcpy(out, r.h_vis, c->n_int64 * sizeof(long long));
    if (n_columns_per_pol) *n_columns_per_pol = r.columns;
    c->n_collected++;   // (the set is free from here on)
    return BF_OK;
}

}  // extern "C"
