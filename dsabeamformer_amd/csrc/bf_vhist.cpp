// bf_vhist.cpp -- the voltage history and its dedispersed cuts (include/dsabf.h: bf_vhist_*; contract, ordering and measurements:
// docs/VOLTAGE_CUTS.md).  The device code is csrc/vcut/bf_vcut.hip; this file checks the bounds, owns the ring of whole gemm-units,
// works out the statuses of a cut on the host and orders pushes and cuts (the pattern is the DM stage's stamp cut, docs/EVENTS.md 2.3).
#include <algorithm>
#include <new>

#include "bf_runtime_internal.h"
#include "vcut/bf_vcut_kernels.h"

struct bf_vhist : bf_stage {
    bf_vhist() : bf_stage("voltage history") {}
    int n_dm = 0;
    uint32_t S = 0, B = 0;             // samples of a unit; bytes of a sample (n_pol n_ant)
    size_t unit_bytes = 0;             // n_freq S B
    uint64_t cap_units = 0, next_unit = 0;
    uint8_t* d_ring = nullptr;         // [cap_units][n_freq][S][B]: a plain allocation, it wraps at unit granularity
    int32_t* d_delays = nullptr;       // [n_dm][n_freq], samples
    std::vector<int32_t> trial_delay;  // the largest delay of each row
    // pushed[k % 2] is recorded behind push k's copy and behind push k - 1's event: "every unit < next_unit is in place".
    hipEvent_t pushed[2] = {nullptr, nullptr};
    uint64_t n_push = 0;
    std::vector<std::pair<hipStream_t, uint64_t>> seen;   // per queue that has pushed: every unit below this is ordered before what it does next
    // the end of the most recent cut, recorded behind the cut before it: what a later push waits for before it writes
    hipEvent_t cut_done = nullptr;
    bool cut_recorded = false;
    hipStream_t cut_q = nullptr;       // bf_vhist_cut_host: a queue of the stage's own, made at the first call ...
    uint8_t* d_cut = nullptr;          // ... and its device buffer, grown to the largest call
    size_t cut_bytes = 0;
};

// One push, already checked: the copy of n_units whole units (two copies where the range wraps) on `q`, then the event.
static int push_impl(bf_vhist* v, const uint8_t* in, int n_units, hipStream_t q)
{
    if (v->cut_recorded) HIP_TRY(hipStreamWaitEvent(q, v->cut_done, 0));   // a cut may still be reading the units this push overwrites
    hipEvent_t prev = v->n_push ? v->pushed[(v->n_push + 1) % 2] : nullptr;
    // This push overwrites the units [next_unit - cap_units, next_unit + n_units - cap_units).  Whoever wrote them must have finished:
    // `q` has seen every unit below `seen` (its own pushes, and what the chain held when it last joined it).  With a ring much deeper
    // than a push that is always so, the queue joins the chain behind its copy only, and copies on different queues overlap; a small
    // ring makes the copy itself wait for the push before it.
    uint64_t* seen = nullptr;
    for (auto& qs : v->seen)
        if (qs.first == q) seen = &qs.second;
    if (!seen) {
        v->seen.emplace_back(q, 0);
        seen = &v->seen.back().second;
    }
    const bool early = prev && v->next_unit + (uint64_t)n_units > v->cap_units + *seen;
    if (early) HIP_TRY(hipStreamWaitEvent(q, prev, 0));
    const uint64_t p0 = v->next_unit % v->cap_units;
    const uint64_t first = std::min<uint64_t>((uint64_t)n_units, v->cap_units - p0);
    HIP_TRY(hipMemcpyAsync(v->d_ring + p0 * v->unit_bytes, in, first * v->unit_bytes, hipMemcpyDeviceToDevice, q));
    if (first < (uint64_t)n_units)
        HIP_TRY(hipMemcpyAsync(v->d_ring, in + first * v->unit_bytes, ((uint64_t)n_units - first) * v->unit_bytes, hipMemcpyDeviceToDevice, q));
    if (prev && !early) HIP_TRY(hipStreamWaitEvent(q, prev, 0));
    HIP_TRY(hipEventRecord(v->pushed[v->n_push % 2], q));
    v->n_push++;
    v->next_unit += (uint64_t)n_units;
    *seen = v->next_unit;
    return BF_OK;
}

static int check_push(const bf_vhist* v, int n_units, const char* who)
{
    if (n_units <= 0) return fail(BF_ERR_INVALID, "%s: n_units must be positive", who);
    if ((uint64_t)n_units > v->cap_units)
        return fail(BF_ERR_INVALID, "%s: %d gemm-units; the ring holds %llu", who, n_units, (unsigned long long)v->cap_units);
    return BF_OK;
}

extern "C" {

int bf_vhist_units_needed(const bf_config* cfg, int max_delay_rows, int dm_rows, int n_buf, int t_tol, int max_width, int cut_units)
{
    if (!cfg || cfg->n_out_per_gemm < 1 || cfg->n_gemms_per_block < 1 || max_delay_rows < 0 || dm_rows < 1 || n_buf < 0 || t_tol < 0 || max_width < 0 ||
        cut_units < 1)
        return 0;
    const long long o = cfg->n_out_per_gemm;
    const long long rows = (long long)max_delay_rows + 3LL * dm_rows                                             // the DM stage's own
                           + (long long)cut_units * o / 2 + t_tol + max_width + ((long long)n_buf + 1) * dm_rows;   // docs/EVENTS.md "History"
    const long long units = (rows + o - 1) / o + 1 + cfg->n_gemms_per_block;
    return units > 0x7fffffffLL ? 0 : (int)units;
}

int bf_vhist_create(bf_handle* h, const int32_t* delays, int n_dm, int history_units, bf_vhist** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h) return fail(BF_ERR_INVALID, "bf_vhist_create: the handle is NULL");
    if (!delays) return fail(BF_ERR_INVALID, "bf_vhist_create: delays is NULL");
    if (n_dm < 1) return fail(BF_ERR_INVALID, "bf_vhist_create: n_dm must be >= 1");
    if (history_units < 1) return fail(BF_ERR_INVALID, "bf_vhist_create: history_units must be >= 1");
    const bf_config& cfg = h->cfg;
    const size_t n_del = (size_t)n_dm * (size_t)cfg.n_freq;
    for (size_t i = 0; i < n_del; i++)
        if (delays[i] < 0) return fail(BF_ERR_INVALID, "bf_vhist_create: delays[%zu][%zu] = %d is negative", i / cfg.n_freq, i % cfg.n_freq, delays[i]);
    if ((uint64_t)cfg.n_out_per_gemm * cfg.n_avg * cfg.n_pol * cfg.n_ant >= (1ull << 31))
        return fail(BF_ERR_INVALID, "bf_vhist_create: a channel of a gemm-unit is 2 GiB or more");
    ON_DEVICE(h);
    bf_vhist* v = new (std::nothrow) bf_vhist();
    if (!v) return fail(BF_ERR_DEVICE, "out of host memory");
    v->h = h;
    v->n_dm = n_dm;
    v->S = (uint32_t)(cfg.n_out_per_gemm * cfg.n_avg);
    v->B = (uint32_t)(cfg.n_pol * cfg.n_ant);
    v->unit_bytes = (size_t)cfg.n_freq * v->S * v->B;
    v->cap_units = (uint64_t)history_units;
    v->trial_delay.resize((size_t)n_dm);
    for (int d = 0; d < n_dm; d++) v->trial_delay[(size_t)d] = *std::max_element(delays + (size_t)d * cfg.n_freq, delays + (size_t)(d + 1) * cfg.n_freq);
    bf_resources& res = v->res;
    res.dev(&v->d_ring, v->cap_units * v->unit_bytes);
    res.dev(&v->d_delays, n_del * sizeof(int32_t));
    for (auto& ev : v->pushed) res.event(&ev);
    res.event(&v->cut_done);
    if (res.err == hipSuccess) res.err = hipMemcpy(v->d_delays, delays, n_del * sizeof(int32_t), hipMemcpyHostToDevice);
    if (int rc = stage_adopt(v, "bf_vhist_create")) return rc;
    *out = v;
    return BF_OK;
}

int bf_vhist_destroy(bf_vhist* v) { return stage_destroy(v); }

int bf_vhist_push(bf_vhist* v, const void* d_packed, int n_units, void* hip_stream)
{
    if (!v || !d_packed) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(v)) return rc;
    if ((uintptr_t)d_packed & 3) return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 4-byte aligned");
    if (int rc = check_push(v, n_units, "bf_vhist_push")) return rc;
    ON_DEVICE(v->h);
    return push_impl(v, static_cast<const uint8_t*>(d_packed), n_units, as_stream(hip_stream));
}

int bf_vhist_push_block(bf_vhist* v, int stream_idx, int slot, int first_unit, int n_units)
{
    if (!v) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(v)) return rc;
    bf_handle* h = v->h;
    const uint8_t* in = nullptr;
    if (int rc = resident_units(h, stream_idx, slot, first_unit, n_units, &in)) return rc;
    if (int rc = check_push(v, n_units, "bf_vhist_push_block")) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);   // the push is ordered on queue stream_idx: nothing of the handle's may still be only queued
    return push_impl(v, in, n_units, h->streams[stream_idx]);
}

int bf_vhist_history(const bf_vhist* v, uint64_t* oldest_unit, uint64_t* next_unit, uint64_t* cap_units)
{
    if (!v || !oldest_unit || !next_unit || !cap_units) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(v)) return rc;
    *next_unit = v->next_unit;
    *cap_units = v->cap_units;
    *oldest_unit = v->next_unit > v->cap_units ? v->next_unit - v->cap_units : 0;
    return BF_OK;
}

int bf_vhist_cut(bf_vhist* v, const bf_vcut_request* reqs, int n_req, int n_units_out, void* d_out, int32_t* status, void* hip_stream)
{
    if (!v) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_req < 0) return fail(BF_ERR_INVALID, "n_req must be >= 0");
    if (n_req > 0 && (!reqs || !d_out || !status)) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(v)) return rc;
    bf_handle* h = v->h;
    if (n_units_out < 1) return fail(BF_ERR_INVALID, "bf_vhist_cut: n_units_out must be >= 1");
    if ((uint64_t)n_units_out * (uint64_t)h->cfg.n_freq > dsabf::kVcutMaxRuns)
        return fail(BF_ERR_INVALID, "bf_vhist_cut: %d units of %d channels are more than %u runs per request", n_units_out, h->cfg.n_freq, dsabf::kVcutMaxRuns);
    if ((uintptr_t)d_out & 3) return fail(BF_ERR_INVALID, "misaligned device pointer: d_out must be 4-byte aligned");
    for (int r = 0; r < n_req; r++)
        if (reqs[r].dm < 0 || reqs[r].dm >= v->n_dm) return fail(BF_ERR_INVALID, "request %d: trial %d outside [0, %d)", r, reqs[r].dm, v->n_dm);
    // the statuses: pure arithmetic on what the host knows
    const uint64_t next_s = v->next_unit * v->S, oldest_s = (v->next_unit > v->cap_units ? v->next_unit - v->cap_units : 0) * v->S;
    int n_cut = 0;
    for (int r = 0; r < n_req; r++) {
        const uint64_t span = (uint64_t)n_units_out * v->S + (uint64_t)v->trial_delay[(size_t)reqs[r].dm];   // (< 2^51 + 2^31)
        const uint64_t t0 = reqs[r].t0;
        status[r] = t0 < oldest_s ? 1 : (t0 > next_s || span > next_s - t0) ? 2 : 0;
        n_cut += status[r] == 0;
    }
    if (!n_cut) return BF_OK;
    ON_DEVICE(h);
    hipStream_t q = as_stream(hip_stream);
    // (1) the newest push's event: every unit < next_unit is in place
    HIP_TRY(hipStreamWaitEvent(q, v->pushed[(v->n_push + 1) % 2], 0));   // (status 0 means something has been pushed)
    const dsabf::VcutRing ring{v->d_ring, v->cap_units, (uint32_t)h->cfg.n_freq, v->S, v->B};
    dsabf::VcutBatch batch{};
    hipError_t launch_err = hipSuccess;
    int n_items = 0;
    for (int r = 0; r < n_req; r++) {
        if (status[r] == 0) {
            dsabf::VcutItem& it = batch.item[n_items++];
            it.phys = (uint32_t)(reqs[r].t0 / v->S % v->cap_units);
            it.rest = (uint32_t)(reqs[r].t0 % v->S);
            it.dm = reqs[r].dm;
            it.slot = r;
        }
        if (n_items == dsabf::kVcutBatch || (r == n_req - 1 && n_items)) {
            launch_err = dsabf::launch_vcut(ring, v->d_delays, batch, n_items, n_units_out, static_cast<uint8_t*>(d_out), q);
            if (launch_err != hipSuccess) break;   // (what was launched before it is still recorded below)
            n_items = 0;
        }
    }
    // (2) cut_done, behind the cut before this one: "this cut and every earlier one have read their units"; (3) push_impl waits for it.
    if (v->cut_recorded) HIP_TRY(hipStreamWaitEvent(q, v->cut_done, 0));
    HIP_TRY(hipEventRecord(v->cut_done, q));
    v->cut_recorded = true;
    if (launch_err != hipSuccess) return fail(BF_ERR_DEVICE, "bf_vhist_cut: the launch failed: %s", hipGetErrorString(launch_err));
    return BF_OK;
}

// The cut for a host consumer (run_observation): on a queue of the stage's own, into the stage's device buffer, copied to host_out
// (pinned for an asynchronous copy) and waited for THERE -- the caller's queues keep running.  The units of requests with a non-zero
// status are not written.
int bf_vhist_cut_host(bf_vhist* v, const bf_vcut_request* reqs, int n_req, int n_units_out, void* host_out, int32_t* status)
{
    if (!v) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_req < 0) return fail(BF_ERR_INVALID, "n_req must be >= 0");
    if (n_req > 0 && (!reqs || !host_out || !status)) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(v)) return rc;
    if (n_units_out < 1) return fail(BF_ERR_INVALID, "bf_vhist_cut_host: n_units_out must be >= 1");
    if (!n_req) return BF_OK;
    bf_handle* h = v->h;
    ON_DEVICE(h);
    const size_t req_bytes = (size_t)n_units_out * v->unit_bytes, need = req_bytes * (size_t)n_req;
    if (!v->cut_q) {
        v->res.queue(&v->cut_q);
        if (v->res.err != hipSuccess) return fail(BF_ERR_DEVICE, "bf_vhist_cut_host: %s", hipGetErrorString(v->res.err));
    }
    if (need > v->cut_bytes) {   // (nothing of an earlier call is in flight: every call ends with a wait for its queue)
        uint8_t* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, need));
        for (void*& d : v->res.device)
            if (d == v->d_cut && d) {
                (void)hipFree(d);
                d = nullptr;
            }
        v->res.device.push_back(p);
        v->d_cut = p;
        v->cut_bytes = need;
    }
    if (int rc = bf_vhist_cut(v, reqs, n_req, n_units_out, v->d_cut, status, v->cut_q)) return rc;
    for (int r = 0; r < n_req; r++)
        if (status[r] == 0)
            HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(host_out) + (size_t)r * req_bytes, v->d_cut + (size_t)r * req_bytes, req_bytes,
                                   hipMemcpyDeviceToHost, v->cut_q));
    HIP_TRY(hipStreamSynchronize(v->cut_q));
    return BF_OK;
}

}  // extern "C"
