// bf_accum.cpp -- the snapshot-and-zero accumulator (bf_accumulator, bf_runtime_internal.h): bytes on the device that pushes add to and a
// dump copies out and zeroes, ordered by a bf_chain whatever queues they come on, the snapshots in a bf_result_ring.  The pulsar folder
// (bf_psr.cpp) holds one; so does the accumulator stage under the correlator and the voltage moments (bf_accum_stage), whose entry points
// are here too: what a kind of stage computes is its bf_accum_kind (bf_corr.cpp, bf_sk.cpp).
#include <cstring>
#include <memory>
#include <string>

#include "bf_runtime_internal.h"

void bf_accumulator::create(bf_resources& res, size_t bytes_, int max_in_flight)
{
    bytes = bytes_;
    res.dev(&d_acc, bytes, true);
    chain.create(res);
    ring.create(res, max_in_flight);
    for (auto& r : ring.sets) res.host(&r.h_acc, bytes);
}

int bf_accumulator::dump(uint64_t record0, uint64_t record1)
{
    snapshot& r = ring.next();
    HIP_TRY(chain.wait(ring.copy_q));
    HIP_TRY(hipMemcpyAsync(r.h_acc, d_acc, bytes, hipMemcpyDeviceToHost, ring.copy_q));
    HIP_TRY(hipMemsetAsync(d_acc, 0, bytes, ring.copy_q));
    HIP_TRY(hipEventRecord(r.copied, ring.copy_q));
    chain.adopt(r.copied);
    r.record[0] = record0;
    r.record[1] = record1;
    ring.issued();
    return BF_OK;
}

int bf_accumulator::collect(const char** h_acc, uint64_t record[2])
{
    HIP_TRY(ring.wait_oldest());
    const snapshot& r = ring.oldest();
    *h_acc = r.h_acc;
    record[0] = r.record[0];
    record[1] = r.record[1];
    ring.collected();
    return BF_OK;
}

// "bf_corr" + "_push": the entry point's name, as the messages carry it
static std::string entry(const bf_accum_stage* s, const char* suffix) { return std::string(s->kind.abi) + suffix; }

// One push of a stage, already checked: behind whatever used the accumulator last, and the new end of that chain.
static int push_impl(bf_accum_stage* s, const void* d_packed, int n_units, hipStream_t q)
{
    bf_handle* h = s->h;
    HIP_TRY(s->acc.chain.wait(q));
    if (int rc = s->kind.launch(h, d_packed, n_units, reinterpret_cast<long long*>(s->acc.d_acc), true, q)) return rc;
    HIP_TRY(s->acc.chain.extend(q));
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
    s->acc.create(s->res, 2 * s->kind.entries(&h->cfg) * sizeof(long long), max_in_flight);
    s->res.device_sync();
    return stage_adopt(keep.release(), who.c_str());
}

int dsabf::rt::accum_pending(const bf_accum_stage* s) { return s ? s->acc.ring.pending() : fail(BF_ERR_INVALID, "the stage is NULL"); }

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
    if (!s->acc.ring.room())
        return fail(BF_ERR_STATE, "%s_dump: %d dumps are uncollected (max_in_flight): %s_collect first", s->kind.abi, s->acc.ring.max_in_flight, s->kind.abi);
    ON_DEVICE(s->h);
    if (int rc = s->acc.dump(s->columns)) return rc;
    s->columns = 0;
    return BF_OK;
}

int dsabf::rt::accum_collect(bf_accum_stage* s, int64_t* out, uint64_t* n_columns_per_pol)
{
    if (!s || !out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (!s->acc.ring.pending()) return fail(BF_ERR_STATE, "%s_collect: no dump is pending", s->kind.abi);
    ON_DEVICE(s->h);
    const char* h_acc = nullptr;
    uint64_t record[2];
    if (int rc = s->acc.collect(&h_acc, record)) return rc;
    std::memcpy(out, h_acc, s->acc.bytes);
    if (n_columns_per_pol) *n_columns_per_pol = record[0];
    return BF_OK;
}
