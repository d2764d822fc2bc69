// bf_sk.cpp -- voltage moments and spectral kurtosis (include/dsabf.h: bf_sk_device, bf_sk_select, bf_sk_*; contract and
// measurements: docs/SPECTRAL_KURTOSIS.md).  The device code is csrc/sk/bf_sk.hip; this file checks the bounds, owns a stage's
// accumulator and orders its pushes and dumps (a twin of bf_corr.cpp), and holds the host rule that turns moments into flags.
#include <cmath>
#include <cstring>
#include <new>

#include "bf_runtime_internal.h"
#include "sk/bf_sk_kernels.h"

struct bf_sk : bf_stage {
    bf_sk() : bf_stage("moments stage") {}
    int max_in_flight = 0;
    size_t n_int64 = 0;                // 2 * bf_sk_entries
    long long* d_acc = nullptr;        // the integration in progress: every push adds to it, a dump copies it out and zeroes it
    uint64_t columns = 0;              // columns per polarisation pushed since the last dump
    // Pushes and dumps share d_acc, so each waits for the one before it, whatever queue that was issued on (as in bf_corr).
    hipEvent_t push_done[2] = {nullptr, nullptr};
    hipEvent_t last = nullptr;
    uint64_t n_push = 0;
    struct result_set {
        long long* h_mom = nullptr;    // pinned
        hipEvent_t copied = nullptr;
        uint64_t columns = 0;
    };
    std::vector<result_set> sets;      // dump j leaves its snapshot in set j % max_in_flight
    hipStream_t copy_q = nullptr;
    uint64_t n_dump = 0, n_collected = 0;
};

// The bounds of one launch (include/dsabf.h): n_ant <= 2048, n_pol <= 64, fewer than 2^24 columns per polarisation.
static int check_launch(const bf_handle* h, int n_units, const char* who)
{
    if (n_units <= 0) return fail(BF_ERR_INVALID, "%s: n_units must be positive", who);
    if (h->cfg.n_ant > dsabf::kSkMaxAnt || h->cfg.n_ant % 4)
        return fail(BF_ERR_INVALID, "%s: %d antennas; the moments are defined for a multiple of 4 up to %d", who, h->cfg.n_ant, dsabf::kSkMaxAnt);
    if (h->cfg.n_pol > dsabf::kSkMaxPol)
        return fail(BF_ERR_INVALID, "%s: %d polarisations; the moments are defined up to %d", who, h->cfg.n_pol, dsabf::kSkMaxPol);
    const long long n = (long long)n_units * h->cfg.n_out_per_gemm * h->cfg.n_avg;
    if (n > dsabf::kSkMaxColumns)
        return fail(BF_ERR_INVALID, "%s: %lld columns per polarisation in one call; a call is defined below 2^24 (M1 <= 128 * N fits int32)", who, n);
    return BF_OK;
}

static int launch(bf_handle* h, const void* d_packed, int n_units, long long* d_mom, bool accumulate, hipStream_t q)
{
    HIP_TRY(dsabf::launch_moments(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_pol, h->cfg.n_out_per_gemm * h->cfg.n_avg, d_packed, n_units, d_mom,
                                  accumulate, h->n_cus, q));
    return BF_OK;
}

// One push of a stage, already checked: behind whatever used the accumulator last, and the new end of that chain.
static int push_impl(bf_sk* c, const void* d_packed, int n_units, hipStream_t q)
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

size_t bf_sk_entries(const bf_config* cfg)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_pol <= 0 || cfg->n_ant <= 0) return 0;
    return (size_t)cfg->n_freq * (size_t)cfg->n_pol * (size_t)cfg->n_ant;
}

int bf_sk_default_options(bf_sk_options* o)
{
    if (!o) return fail(BF_ERR_INVALID, "NULL argument");
    o->centre = 1.0;
    o->n_sigma = 5.0;
    o->max_bad_fraction_ant = 0.5;
    o->max_bad_fraction_chan = 0.5;
    return BF_OK;
}

// Host arithmetic in fp64, one rounding per operation (the library is built with -ffp-contract=off), in the order of include/dsabf.h.
int bf_sk_select(const int64_t* moments, uint64_t n_columns_per_pol, int n_freq, int n_pol, int n_ant, const bf_sk_options* opt, double* sk,
                 uint8_t* cell, uint8_t* ant_flags, uint8_t* chan_flags)
{
    if (!moments) return fail(BF_ERR_INVALID, "bf_sk_select: moments is NULL");
    if (n_columns_per_pol < 2) return fail(BF_ERR_INVALID, "bf_sk_select: the estimator needs at least 2 columns per polarisation");
    if (n_freq <= 0 || n_pol <= 0 || n_ant <= 0) return fail(BF_ERR_INVALID, "bf_sk_select: n_freq, n_pol and n_ant must be positive");
    bf_sk_options o;
    bf_sk_default_options(&o);
    if (opt) o = *opt;
    const double M = (double)n_columns_per_pol;
    const double scale = (double)(n_columns_per_pol + 1) / (double)(n_columns_per_pol - 1);
    const double half_width = o.n_sigma * 2.0 / std::sqrt(M);
    const double lo = o.centre - half_width, hi = o.centre + half_width;
    const size_t layers = (size_t)n_freq * (size_t)n_pol, n_cells = layers * (size_t)n_ant;
    std::vector<uint8_t> code(n_cells), bad_ant((size_t)n_ant);
    std::vector<size_t> bad((size_t)n_ant, 0);
    for (size_t l = 0; l < layers; l++)
        for (int a = 0; a < n_ant; a++) {
            const size_t i = l * (size_t)n_ant + (size_t)a;
            const int64_t m1 = moments[2 * i], m2 = moments[2 * i + 1];
            double v = 0.0;
            uint8_t c = 0;
            if (m1 == 0) {
                c = BF_SK_DEAD;
            } else {
                const double r = (M * (double)m2) / ((double)m1 * (double)m1);
                v = scale * (r - 1.0);
                if (v < lo) c |= BF_SK_LOW;
                if (v > hi) c |= BF_SK_HIGH;
            }
            code[i] = c;
            if (sk) sk[i] = v;
            if (cell) cell[i] = c;
            if (c) bad[(size_t)a]++;
        }
    int n_good = 0;
    for (int a = 0; a < n_ant; a++) {
        bad_ant[(size_t)a] = (double)bad[(size_t)a] > o.max_bad_fraction_ant * (double)layers ? 1 : 0;
        if (!bad_ant[(size_t)a]) n_good++;
        if (ant_flags) ant_flags[a] = bad_ant[(size_t)a];
    }
    if (chan_flags)
        for (int f = 0; f < n_freq; f++) {
            size_t bad_f = 0;
            for (int p = 0; p < n_pol; p++)
                for (int a = 0; a < n_ant; a++)
                    if (!bad_ant[(size_t)a] && code[((size_t)f * (size_t)n_pol + (size_t)p) * (size_t)n_ant + (size_t)a]) bad_f++;
            chan_flags[f] = (n_good == 0 || (double)bad_f > o.max_bad_fraction_chan * (double)((size_t)n_good * (size_t)n_pol)) ? 1 : 0;
        }
    return BF_OK;
}

int bf_sk_device(bf_handle* h, const void* d_packed, int n_units, int64_t* d_moments, int accumulate, void* hip_stream)
{
    if (!h || !d_packed || !d_moments) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_launch(h, n_units, "bf_sk_device")) return rc;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_moments & 7))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned, d_moments 8-byte aligned");
    ON_DEVICE(h);
    return launch(h, d_packed, n_units, (long long*)d_moments, accumulate != 0, as_stream(hip_stream));
}

int bf_sk_create(bf_handle* h, int max_in_flight, bf_sk** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h) return fail(BF_ERR_INVALID, "bf_sk_create: the handle is NULL");
    if (max_in_flight <= 0) return fail(BF_ERR_INVALID, "bf_sk_create: max_in_flight must be positive");
    if (int rc = check_launch(h, 1, "bf_sk_create")) return rc;
    ON_DEVICE(h);
    bf_sk* c = new (std::nothrow) bf_sk();
    if (!c) return fail(BF_ERR_DEVICE, "out of host memory");
    c->h = h;
    c->max_in_flight = max_in_flight;
    c->n_int64 = 2 * bf_sk_entries(&h->cfg);
    const size_t bytes = c->n_int64 * sizeof(long long);
    bf_resources& res = c->res;
    res.dev(&c->d_acc, bytes, true);
    res.queue(&c->copy_q);
    for (auto& ev : c->push_done) res.event(&ev);
    c->sets.resize((size_t)max_in_flight);
    for (auto& r : c->sets) {
        res.host(&r.h_mom, bytes);
        res.event(&r.copied);
    }
    res.device_sync();
    if (int rc = stage_adopt(c, "bf_sk_create")) return rc;
    *out = c;
    return BF_OK;
}

int bf_sk_destroy(bf_sk* c) { return stage_destroy(c); }

int bf_sk_pending(const bf_sk* c) { return c ? (int)(c->n_dump - c->n_collected) : fail(BF_ERR_INVALID, "the stage is NULL"); }

int bf_sk_push(bf_sk* c, const void* d_packed, int n_units, void* hip_stream)
{
    if (!c || !d_packed) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(c)) return rc;
    if (int rc = check_launch(c->h, n_units, "bf_sk_push")) return rc;
    if ((uintptr_t)d_packed & 15) return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned");
    ON_DEVICE(c->h);
    return push_impl(c, d_packed, n_units, as_stream(hip_stream));
}

int bf_sk_push_block(bf_sk* c, int stream_idx, int slot, int first_unit, int n_units)
{
    if (!c) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(c)) return rc;
    bf_handle* h = c->h;
    if (stream_idx < 0 || stream_idx >= h->cfg.n_streams) return fail(BF_ERR_INVALID, "stream %d out of range", stream_idx);
    if (slot < 0 || slot >= h->cfg.n_blocks_on_gpu) return fail(BF_ERR_INVALID, "slot %d out of range", slot);
    if (first_unit < 0 || n_units <= 0 || first_unit + n_units > h->cfg.n_gemms_per_block)
        return fail(BF_ERR_INVALID, "gemm-units [%d, %d) are not inside a block of %d", first_unit, first_unit + n_units, h->cfg.n_gemms_per_block);
    if (int rc = check_launch(h, n_units, "bf_sk_push_block")) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);   // the push is ordered on queue stream_idx: nothing of the handle's may still be only queued
    const uint8_t* in = h->d_data + bf_bytes_per_gemm(&h->cfg) * ((size_t)h->cfg.n_gemms_per_block * slot + first_unit);
    return push_impl(c, in, n_units, h->streams[stream_idx]);
}

int bf_sk_dump(bf_sk* c, void* hip_stream)
{
    (void)hip_stream;   // the dump never holds the caller's queue: it is ordered by the stage's own chain
    if (!c) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(c)) return rc;
    if (c->n_dump - c->n_collected >= (uint64_t)c->max_in_flight)
        return fail(BF_ERR_STATE, "bf_sk_dump: %d dumps are uncollected (max_in_flight): bf_sk_collect first", c->max_in_flight);
    ON_DEVICE(c->h);
    bf_sk::result_set& r = c->sets[c->n_dump % c->max_in_flight];
    if (c->last) HIP_TRY(hipStreamWaitEvent(c->copy_q, c->last, 0));
    const size_t bytes = c->n_int64 * sizeof(long long);
    HIP_TRY(hipMemcpyAsync(r.h_mom, c->d_acc, bytes, hipMemcpyDeviceToHost, c->copy_q));
    HIP_TRY(hipMemsetAsync(c->d_acc, 0, bytes, c->copy_q));
    HIP_TRY(hipEventRecord(r.copied, c->copy_q));
    c->last = r.copied;
    r.columns = c->columns;
    c->columns = 0;
    c->n_dump++;
    return BF_OK;
}

int bf_sk_collect(bf_sk* c, int64_t* out, uint64_t* n_columns_per_pol)
{
    if (!c || !out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(c)) return rc;
    if (c->n_collected == c->n_dump) return fail(BF_ERR_STATE, "bf_sk_collect: no dump is pending");
    ON_DEVICE(c->h);
    bf_sk::result_set& r = c->sets[c->n_collected % c->max_in_flight];
    HIP_TRY(hipEventSynchronize(r.copied));
    std::memcpy(out, r.h_mom, c->n_int64 * sizeof(long long));
    if (n_columns_per_pol) *n_columns_per_pol = r.columns;
    c->n_collected++;   // (the set is free from here on)
    return BF_OK;
}

}  // extern "C"
