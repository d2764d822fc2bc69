// bf_accum.cpp -- the accumulator stage under the correlator and the voltage moments (bf_accum_stage, bf_runtime_internal.h): one int64
// accumulator on the device that pushes add to and a dump snapshots and zeroes.  This file owns the accumulator, orders its pushes and
// dumps whatever queues they come on, and keeps the result sets; what a kind of stage computes is its bf_accum_kind (bf_corr.cpp, bf_sk.cpp).
#include <cstring>
#include <memory>
#include <string>

#include "bf_runtime_internal.h"

// "bf_corr" + "_push": the entry point's name, as the messages carry it
static std::string entry(const bf_accum_stage* s, const char* suffix) { return std::string(s->kind.abi) + suffix; }

// One push of a stage, already checked: behind whatever used the accumulator last, and the new end of that chain.
static int push_impl(bf_accum_stage* s, const void* d_packed, int n_units, hipStream_t q)
{
    bf_handle* h = s->h;
    if (s->last) HIP_TRY(hipStreamWaitEvent(q, s->last, 0));
    if (int rc = s->kind.launch(h, d_packed, n_units, s->d_acc, true, q)) return rc;
    hipEvent_t ev = s->push_done[s->n_push++ % 2];
    HIP_TRY(hipEventRecord(ev, q));
    s->last = ev;
    s->columns += (uint64_t)n_units * (uint64_t)h->cfg.n_out_per_gemm * (uint64_t)h->cfg.n_avg;
    return BF_OK;
}

int dsabf::rt::accum_init(bf_accum_stage* fresh, bf_handle* h, int max_in_flight)
{
    std::unique_ptr<bf_accum_stage> keep(fresh);   // (until its handle adopts it)
    if (!fresh) return fail(BF_ERR_DEVICE, "out of host memory");
    bf_accum_stage* s = fresh;
    const std::string who = entry(s, "_create");
    if (!h) return fail(BF_ERR_INVALID, "%s: the handle is NULL", who.c_str());
    if (max_in_flight <= 0) return fail(BF_ERR_INVALID, "%s: max_in_flight must be positive", who.c_str());
    if (int rc = s->kind.check_create(h)) return rc;
    ON_DEVICE(h);
    s->h = h;
    s->max_in_flight = max_in_flight;
    s->n_int64 = 2 * s->kind.entries(&h->cfg);
    const size_t bytes = s->n_int64 * sizeof(long long);
    bf_resources& res = s->res;
    res.dev(&s->d_acc, bytes, true);
    res.queue(&s->copy_q);
    for (auto& ev : s->push_done) res.event(&ev);
    s->sets.resize((size_t)max_in_flight);
    for (auto& r : s->sets) {
        res.host(&r.h_acc, bytes);
        res.event(&r.copied);
    }
    res.device_sync();
    return stage_adopt(keep.release(), who.c_str());
}

int dsabf::rt::accum_pending(const bf_accum_stage* s) { return s ? (int)(s->n_dump - s->n_collected) : fail(BF_ERR_INVALID, "the stage is NULL"); }

int dsabf::rt::accum_push(bf_accum_stage* s, const void* d_packed, int n_units, void* hip_stream)
{
    if (!s || !d_packed) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (int rc = s->kind.check_launch(s->h, n_units, entry(s, "_push").c_str())) return rc;
    if ((uintptr_t)d_packed & 15) return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned");
    ON_DEVICE(s->h);
    return push_impl(s, d_packed, n_units, as_stream(hip_stream));
}

int dsabf::rt::accum_push_block(bf_accum_stage* s, int stream_idx, int slot, int first_unit, int n_units)
{
    if (!s) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(s)) return rc;
    bf_handle* h = s->h;
    const uint8_t* in = nullptr;
    if (int rc = resident_units(h, stream_idx, slot, first_unit, n_units, &in)) return rc;
    if (int rc = s->kind.check_launch(h, n_units, entry(s, "_push_block").c_str())) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);   // the push is ordered on queue stream_idx: nothing of the handle's may still be only queued
    return push_impl(s, in, n_units, h->streams[stream_idx]);
}

// (the dump never holds the caller's queue: it is ordered by the stage's own chain)
int dsabf::rt::accum_dump(bf_accum_stage* s)
{
    if (!s) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(s)) return rc;
    if (s->n_dump - s->n_collected >= (uint64_t)s->max_in_flight)
        return fail(BF_ERR_STATE, "%s_dump: %d dumps are uncollected (max_in_flight): %s_collect first", s->kind.abi, s->max_in_flight, s->kind.abi);
    ON_DEVICE(s->h);
    bf_accum_stage::result_set& r = s->sets[s->n_dump % s->max_in_flight];
    if (s->last) HIP_TRY(hipStreamWaitEvent(s->copy_q, s->last, 0));
    const size_t bytes = s->n_int64 * sizeof(long long);
    HIP_TRY(hipMemcpyAsync(r.h_acc, s->d_acc, bytes, hipMemcpyDeviceToHost, s->copy_q));
    HIP_TRY(hipMemsetAsync(s->d_acc, 0, bytes, s->copy_q));
    HIP_TRY(hipEventRecord(r.copied, s->copy_q));
    s->last = r.copied;
    r.columns = s->columns;
    s->columns = 0;
    s->n_dump++;
    return BF_OK;
}

int dsabf::rt::accum_collect(bf_accum_stage* s, int64_t* out, uint64_t* n_columns_per_pol)
{
    if (!s || !out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (s->n_collected == s->n_dump) return fail(BF_ERR_STATE, "%s_collect: no dump is pending", s->kind.abi);
    ON_DEVICE(s->h);
    bf_accum_stage::result_set& r = s->sets[s->n_collected % s->max_in_flight];
    HIP_TRY(hipEventSynchronize(r.copied));
    std::memcpy(out, r.h_acc, s->n_int64 * sizeof(long long));
    if (n_columns_per_pol) *n_columns_per_pol = r.columns;
    s->n_collected++;   // (the set is free from here on)
    return BF_OK;
}
