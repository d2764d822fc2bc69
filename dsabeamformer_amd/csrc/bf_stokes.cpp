// bf_stokes.cpp -- full-Stokes follow-up beams (include/dsabf.h: bf_stokes_*; contract and measurements: docs/STOKES.md).  The device
// code is csrc/stokes/bf_stokes.hip; this file checks the bounds, owns a stage's compact weights and result sets (a bf_result_ring:
// bf_runtime_internal.h), and orders its weight gathers, pushes and copies on two bf_chains (the caller's queue is held for the kernel only).
#include <cstring>
#include <new>

#include "bf_runtime_internal.h"
#include "stokes/bf_stokes_kernels.h"

struct bf_stokes : bf_stage {
    bf_stokes() : bf_stage("Stokes stage") {}
    int n_int = 0;
    int n_sel = 0;                     // 0: no weights yet
    int cap_sel = 0;                   // beams the result sets are sized for: the largest selection so far
    int8_t* d_w = nullptr;             // the compact weights (ONE copy: a gather waits for the pushes in flight, docs/STOKES.md section 2)
    int8_t* h_w = nullptr;             // pinned: where bf_stokes_set_weights builds them
    // Whatever writes d_w (a gather, an upload) waits for the write before it and for every kernel that may still read d_w, whichever
    // queues those were issued on; whatever reads it waits for the last write.
    bf_chain gathers;                  // the writes of d_w: every later kernel waits for its end
    bf_chain direct;                   // its end fires when EVERY bf_stokes_device / _voltages_device kernel issued so far has run (each joins the one before it)
    struct result_set : bf_result_set {
        long long* d_out = nullptr;    // n_gemms_per_block units of entries at cap_sel beams (allocated by the first set_weights)
        long long* h_out = nullptr;    // pinned, the same size
        hipEvent_t computed = nullptr; // the kernel, on the caller's queue (`copied`: the D2H copy)
        int n_units = 0, n_sel = 0;
    };
    bf_result_ring<result_set> ring;   // one issue per push
};

static size_t entries(const bf_config& cfg, int n_sel, int n_int)
{
    return (size_t)(cfg.n_out_per_gemm * cfg.n_avg / n_int) * (size_t)cfg.n_freq * (size_t)n_sel;
}

// What the geometry and the window must satisfy (include/dsabf.h), apart from the beams.
static int check_geometry(const bf_config& cfg, int n_int, const char* who)
{
    if (cfg.n_pol != 2) return fail(BF_ERR_INVALID, "%s: %d polarisations; Stokes parameters need the column pairs (X, Y) of n_pol = 2", who, cfg.n_pol);
    if (cfg.n_ant > dsabf::kStokesMaxAnt || cfg.n_ant % 4)
        return fail(BF_ERR_INVALID, "%s: %d antennas; the Stokes beams are defined for a multiple of 4 up to %d (|X| <= 2048 n_ant fits the int32 accumulator)",
                    who, cfg.n_ant, dsabf::kStokesMaxAnt);
    const int S = cfg.n_out_per_gemm * cfg.n_avg;
    if (n_int < 1 || S % n_int) return fail(BF_ERR_INVALID, "%s: n_int %d does not divide the %d samples of a gemm-unit", who, n_int, S);
    if (!dsabf::stokes_supported(cfg.n_ant, cfg.n_pol, S, 1, n_int)) return fail(BF_ERR_INVALID, "%s: %d samples per gemm-unit are beyond 2^20", who, S);
    return BF_OK;
}

static int check_beams(const bf_config& cfg, const int* beams, int n_sel, const char* who)
{
    if (n_sel < 1 || n_sel > BF_STOKES_MAX_BEAMS) return fail(BF_ERR_INVALID, "%s: %d beams; a stage follows 1 ... %d", who, n_sel, BF_STOKES_MAX_BEAMS);
    for (int i = 0; i < n_sel; i++)
        if (beams[i] < 0 || beams[i] >= cfg.n_beams) return fail(BF_ERR_INVALID, "%s: beam %d is not one of the %d beams", who, beams[i], cfg.n_beams);
    return BF_OK;
}

static int check_push(const bf_stokes* s, const void* d_packed, int n_units, const char* who)
{
    if (n_units <= 0) return fail(BF_ERR_INVALID, "%s: n_units must be positive", who);
    if (n_units > s->h->cfg.n_gemms_per_block)
        return fail(BF_ERR_INVALID, "%s: %d gemm-units; a result set holds the %d of a block", who, n_units, s->h->cfg.n_gemms_per_block);
    if (!s->n_sel) return fail(BF_ERR_STATE, "%s: bf_stokes_set_weights has not been called", who);
    if (!s->ring.room())
        return fail(BF_ERR_STATE, "%s: %d result sets are uncollected (max_in_flight): bf_stokes_collect first", who, s->ring.max_in_flight);
    return BF_OK;
}

static int launch(const bf_stokes* s, const void* d_packed, int n_units, long long* d_out, hipStream_t q)
{
    const bf_config& cfg = s->h->cfg;
    HIP_TRY(dsabf::launch_stokes(cfg.n_ant, cfg.n_freq, cfg.n_out_per_gemm * cfg.n_avg, s->n_sel, s->n_int, d_packed, n_units, s->d_w, d_out,
                                 s->h->n_cus, q));
    return BF_OK;
}

// One push, already checked: the kernel on the caller's queue behind the last gather, its copy on the stage's own queue.
static int push_impl(bf_stokes* s, const void* d_packed, int n_units, hipStream_t q)
{
    bf_stokes::result_set& r = s->ring.next();
    HIP_TRY(s->gathers.wait(q));
    if (int rc = launch(s, d_packed, n_units, r.d_out, q)) return rc;
    HIP_TRY(hipEventRecord(r.computed, q));
    HIP_TRY(hipStreamWaitEvent(s->ring.copy_q, r.computed, 0));
    const size_t bytes = (size_t)n_units * entries(s->h->cfg, s->n_sel, s->n_int) * 4 * sizeof(long long);
    HIP_TRY(hipMemcpyAsync(r.h_out, r.d_out, bytes, hipMemcpyDeviceToHost, s->ring.copy_q));
    HIP_TRY(hipEventRecord(r.copied, s->ring.copy_q));
    r.n_units = n_units;
    r.n_sel = s->n_sel;
    s->ring.issued();
    return BF_OK;
}

// The queue `q` behind the last write of the weights and behind every kernel that may still read them -- the pushes' and the
// bf_stokes_device launches' (an event never recorded, or long fired, holds nothing up).
static int wait_for_weight_users(bf_stokes* s, hipStream_t q)
{
    HIP_TRY(s->gathers.wait(q));
    for (auto& r : s->ring.sets) HIP_TRY(hipStreamWaitEvent(q, r.computed, 0));
    HIP_TRY(s->direct.wait(q));
    return BF_OK;
}

// The tail of the two direct entry points, behind their kernel (which is not held up): q joins the direct launch before it.
static int direct_launched(bf_stokes* s, hipStream_t q)
{
    HIP_TRY(s->direct.join(q));
    return BF_OK;
}

// The write of the weights just queued on `q` is the new last one.
static int weights_written(bf_stokes* s, hipStream_t q, int n_sel)
{
    HIP_TRY(s->gathers.extend(q));
    s->n_sel = n_sel;
    return BF_OK;
}

// The result sets hold n_gemms_per_block units of the LARGEST selection so far (16 beams at n_int = 1 are 512 MiB per set at the
// production geometry, three beams 96 MiB): a selection of more beams than any before it finds the stage drained, and replaces them.
static int ensure_sets(bf_stokes* s, int n_sel, const char* who)
{
    if (n_sel <= s->cap_sel) return BF_OK;
    if (s->ring.pending())
        return fail(BF_ERR_STATE, "%s: %d beams are more than any selection before (%d), so the result sets grow: collect the %d pending ones first", who,
                    n_sel, s->cap_sel, s->ring.pending());
    bf_resources& res = s->res;
    auto drop = [](std::vector<void*>& list, void* p) {
        for (size_t i = 0; i < list.size(); i++)
            if (list[i] == p) {
                list.erase(list.begin() + (long)i);
                return true;
            }
        return false;
    };
    s->cap_sel = 0;
    for (auto& r : s->ring.sets) {   // (nothing is pending: every kernel and copy into them has run)
        if (r.d_out && drop(res.device, r.d_out)) (void)hipFree(r.d_out);
        if (r.h_out && drop(res.pinned, r.h_out)) (void)hipHostFree(r.h_out);
        r.d_out = r.h_out = nullptr;
    }
    const size_t bytes = (size_t)s->h->cfg.n_gemms_per_block * entries(s->h->cfg, n_sel, s->n_int) * 4 * sizeof(long long);
    for (auto& r : s->ring.sets) {
        res.dev(&r.d_out, bytes);
        res.host(&r.h_out, bytes);
    }
    if (res.err != hipSuccess) {
        const hipError_t e = res.err;
        res.err = hipSuccess;
        s->n_sel = 0;   // no sets, no pushes: the next set_weights tries again
        return fail(BF_ERR_DEVICE, "%s: the result sets for %d beams: %s", who, n_sel, hipGetErrorString(e));
    }
    s->cap_sel = n_sel;
    return BF_OK;
}

extern "C" {

size_t bf_stokes_entries(const bf_config* cfg, int n_sel, int n_int)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_out_per_gemm <= 0 || cfg->n_avg <= 0 || cfg->n_pol != 2 || n_sel < 1 || n_sel > BF_STOKES_MAX_BEAMS || n_int < 1 ||
        (cfg->n_out_per_gemm * cfg->n_avg) % n_int)
        return 0;
    return entries(*cfg, n_sel, n_int);
}

int bf_stokes_create(bf_handle* h, int n_int, int max_in_flight, bf_stokes** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h) return fail(BF_ERR_INVALID, "bf_stokes_create: the handle is NULL");
    if (max_in_flight <= 0) return fail(BF_ERR_INVALID, "bf_stokes_create: max_in_flight must be positive");
    if (int rc = check_geometry(h->cfg, n_int, "bf_stokes_create")) return rc;
    ON_DEVICE(h);
    bf_stokes* s = new (std::nothrow) bf_stokes();
    if (!s) return fail(BF_ERR_DEVICE, "out of host memory");
    s->h = h;
    s->n_int = n_int;
    const size_t w_bytes = dsabf::stokes_weight_bytes(h->cfg.n_ant, h->cfg.n_freq);
    bf_resources& res = s->res;
    res.dev(&s->d_w, w_bytes);
    res.host(&s->h_w, w_bytes);
    s->gathers.create(res);
    s->direct.create(res);
    s->ring.create(res, max_in_flight);
    for (auto& r : s->ring.sets) res.event(&r.computed);
    if (int rc = stage_adopt(s, "bf_stokes_create")) return rc;
    *out = s;
    return BF_OK;
}

int bf_stokes_destroy(bf_stokes* s) { return stage_destroy(s); }

int bf_stokes_pending(const bf_stokes* s) { return s ? s->ring.pending() : fail(BF_ERR_INVALID, "the stage is NULL"); }

int bf_stokes_set_weights(bf_stokes* s, const int8_t* w_host, const int* beams, int n_sel)
{
    if (!s || !w_host || !beams) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    const bf_config& cfg = s->h->cfg;
    if (int rc = check_beams(cfg, beams, n_sel, "bf_stokes_set_weights")) return rc;
    ON_DEVICE(s->h);
    if (int rc = ensure_sets(s, n_sel, "bf_stokes_set_weights")) return rc;
    // (h_w is free: this call returns only after its copy has run)
    dsabf::stokes_gather_host(w_host, beams, n_sel, cfg.n_ant, cfg.n_freq, cfg.n_beams, s->h_w);
    if (int rc = wait_for_weight_users(s, s->ring.copy_q)) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_w, s->h_w, dsabf::stokes_weight_bytes(cfg.n_ant, cfg.n_freq), hipMemcpyHostToDevice, s->ring.copy_q));
    if (int rc = weights_written(s, s->ring.copy_q, n_sel)) return rc;
    HIP_TRY(hipEventSynchronize(s->gathers.end));
    return BF_OK;
}

int bf_stokes_set_weights_device(bf_stokes* s, const int8_t* d_w, const int* beams, int n_sel, void* hip_stream)
{
    if (!s || !d_w || !beams) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    const bf_config& cfg = s->h->cfg;
    if (int rc = check_beams(cfg, beams, n_sel, "bf_stokes_set_weights_device")) return rc;
    ON_DEVICE(s->h);
    if (int rc = ensure_sets(s, n_sel, "bf_stokes_set_weights_device")) return rc;
    hipStream_t q = as_stream(hip_stream);
    if (int rc = wait_for_weight_users(s, q)) return rc;
    HIP_TRY(dsabf::launch_stokes_gather(d_w, beams, n_sel, cfg.n_ant, cfg.n_freq, cfg.n_beams, s->d_w, q));
    return weights_written(s, q, n_sel);
}

int bf_stokes_device(bf_stokes* s, const void* d_packed, int n_units, int64_t* d_out, void* hip_stream)
{
    if (!s || !d_packed || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (n_units <= 0) return fail(BF_ERR_INVALID, "bf_stokes_device: n_units must be positive");
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 15))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed and d_out must be 16-byte aligned");
    if (!s->n_sel) return fail(BF_ERR_STATE, "bf_stokes_device: bf_stokes_set_weights has not been called");
    ON_DEVICE(s->h);
    hipStream_t q = as_stream(hip_stream);
    HIP_TRY(s->gathers.wait(q));
    if (int rc = launch(s, d_packed, n_units, (long long*)d_out, q)) return rc;
    return direct_launched(s, q);
}

size_t bf_stokes_voltage_entries(const bf_config* cfg, int n_sel)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_out_per_gemm <= 0 || cfg->n_avg <= 0 || cfg->n_pol != 2 || n_sel < 1 || n_sel > BF_STOKES_MAX_BEAMS) return 0;
    return (size_t)cfg->n_freq * (size_t)n_sel * 2 * (size_t)(cfg->n_out_per_gemm * cfg->n_avg);
}

// The beam samples before the products (docs/COHERENT_DEDISPERSION.md section 1): one more reader of the weights, ordered as bf_stokes_device.
int bf_stokes_voltages_device(bf_stokes* s, const void* d_packed, int n_units, void* d_out, void* hip_stream)
{
    if (!s || !d_packed || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (n_units <= 0) return fail(BF_ERR_INVALID, "bf_stokes_voltages_device: n_units must be positive");
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte and d_out 8-byte aligned");
    const bf_config& cfg = s->h->cfg;
    const int S = cfg.n_out_per_gemm * cfg.n_avg;
    if ((long long)n_units * S > 0x7fffffffLL)
        return fail(BF_ERR_INVALID, "bf_stokes_voltages_device: %d units of %d samples are a series of 2^31 samples or more", n_units, S);
    if (!s->n_sel) return fail(BF_ERR_STATE, "bf_stokes_voltages_device: bf_stokes_set_weights has not been called");
    ON_DEVICE(s->h);
    hipStream_t q = as_stream(hip_stream);
    HIP_TRY(s->gathers.wait(q));
    HIP_TRY(dsabf::launch_stokes_voltages(cfg.n_ant, cfg.n_freq, S, s->n_sel, d_packed, n_units, s->d_w, (float*)d_out, s->h->n_cus, q));
    return direct_launched(s, q);
}

int bf_stokes_push(bf_stokes* s, const void* d_packed, int n_units, void* hip_stream)
{
    if (!s || !d_packed) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if ((uintptr_t)d_packed & 15) return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned");
    if (int rc = check_push(s, d_packed, n_units, "bf_stokes_push")) return rc;
    ON_DEVICE(s->h);
    return push_impl(s, d_packed, n_units, as_stream(hip_stream));
}

int bf_stokes_push_block(bf_stokes* s, int stream_idx, int slot, int first_unit, int n_units)
{
    if (!s) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(s)) return rc;
    bf_handle* h = s->h;
    const uint8_t* in = nullptr;
    if (int rc = resident_units(h, stream_idx, slot, first_unit, n_units, &in)) return rc;
    // (a unit of a small geometry may start on any multiple of 4 bytes -- n_ant % 4 == 0 -- and the kernel then loads 4-byte words)
    if (int rc = check_push(s, in, n_units, "bf_stokes_push_block")) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);   // the push is ordered on queue stream_idx: nothing of the handle's may still be only queued
    return push_impl(s, in, n_units, h->streams[stream_idx]);
}

int bf_stokes_collect(bf_stokes* s, int64_t* out, int* n_units)
{
    if (!s || !out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (!s->ring.pending()) return fail(BF_ERR_STATE, "bf_stokes_collect: no push is pending");
    ON_DEVICE(s->h);
    HIP_TRY(s->ring.wait_oldest());
    const bf_stokes::result_set& r = s->ring.oldest();
    std::memcpy(out, r.h_out, (size_t)r.n_units * entries(s->h->cfg, r.n_sel, s->n_int) * 4 * sizeof(long long));
    if (n_units) *n_units = r.n_units;
    s->ring.collected();
    return BF_OK;
}

}  // extern "C"
