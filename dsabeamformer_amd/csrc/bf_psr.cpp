// bf_psr.cpp -- the pulsar folder (include/dsabf.h: bf_psr_*; contract, ordering and measurements: docs/PULSAR_FOLDING.md).  The
// device code is csrc/psr/bf_psr.hip; this file folds the pushes into a bf_accumulator (bf_runtime_internal.h: it orders the pushes and
// dumps whatever queues they come on and keeps the snapshots), and holds the two host helpers (the model from a spin frequency, the
// per-beam S/N of a folded profile).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "bf_runtime_internal.h"
#include "psr/bf_psr_kernels.h"

struct bf_psr : bf_stage {
    bf_psr() : bf_stage("pulsar folder") {}
    int n_freq = 0, n_beams = 0, max_rows = 0, n_bins = 0, n_psr = 0;
    bf_psr_model model[dsabf::kPsrMaxPulsars] = {};
    int32_t delay_min[dsabf::kPsrMaxPulsars] = {}, delay_max[dsabf::kPsrMaxPulsars] = {};
    int32_t* d_delays = nullptr;       // [n_psr][n_freq]
    // The integration in progress, one allocation: n_prof doubles [k][f][bin][beam], then n_hits uint64 [k][f][bin].  A dump's record
    // is {first_row, n_rows}.
    bf_accumulator acc;
    size_t n_prof = 0, n_hits = 0;
    uint64_t pushed = 0;               // rows the stage has been given
    uint64_t first_row = 0;            // first row of the integration in progress
};

bf_stage* dsabf::rt::as_stage(bf_psr* p) { return p; }

int dsabf::rt::psr_check_attach(const bf_psr* p, const bf_handle* h, int n_freq_total, int max_rows)
{
    if (int rc = orphaned(p)) return rc;
    if (p->h != h) return fail(BF_ERR_INVALID, "bf_dm_stream_attach_folder: the two stages belong to different handles");
    if (p->n_freq != n_freq_total)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_folder: the folder has %d channels, the DM stage %d", p->n_freq, n_freq_total);
    if (p->max_rows < max_rows)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_folder: max_rows_per_push %d < the DM stage's %d", p->max_rows, max_rows);
    if (p->feeder) return fail(BF_ERR_STATE, "bf_dm_stream_attach_folder: the folder is attached to another DM stage");
    return BF_OK;
}

// What a push of n_rows rows is refused for, before anything is queued: the row count, and an oscillator index outside (-2^31, 2^31).
int dsabf::rt::psr_check_push(const bf_psr* p, int n_rows)
{
    if (n_rows < 1 || n_rows > p->max_rows) return fail(BF_ERR_INVALID, "n_rows must be 1 .. %d (max_rows_per_push)", p->max_rows);
    const __int128 lim = (__int128)1 << 31;
    for (int k = 0; k < p->n_psr; k++) {
        const __int128 base = (__int128)p->pushed - (__int128)p->model[k].epoch_row;
        const __int128 lo = base - p->delay_max[k], hi = base + (n_rows - 1) - p->delay_min[k];
        if (lo <= -lim || hi >= lim)
            return fail(BF_ERR_INVALID, "bf_psr_push: pulsar %d would reach |row - epoch_row - delay| >= 2^31: re-anchor epoch_row (a new folder at a "
                        "later epoch)", k);
    }
    return BF_OK;
}

static bool finite_all(std::initializer_list<double> v)
{
    for (double x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

// frac(x) * 2^64 as an integer; a frac that rounds up to 1.0 (x a hair below an integer) is phase 0 of the next turn
static uint64_t turns_to_u64(double x)
{
    const double fr = x - std::floor(x);
    return fr >= 1.0 ? 0 : (uint64_t)std::ldexp(fr, 64);
}

extern "C" {

int bf_psr_model_from_spin(double f0_hz, double f1_hz_s, double phase0_turns, double row_seconds, int64_t epoch_row, bf_psr_model* model)
{
    if (!model) return fail(BF_ERR_INVALID, "bf_psr_model_from_spin: model is NULL");
    if (!finite_all({f0_hz, f1_hz_s, phase0_turns, row_seconds}) || !(row_seconds > 0.0))
        return fail(BF_ERR_INVALID, "bf_psr_model_from_spin: the arguments must be finite and row_seconds > 0");
    const double x = f0_hz * row_seconds;
    const double dd = std::nearbyint(std::ldexp((f1_hz_s * row_seconds) * row_seconds, 64));
    if (!(std::fabs(dd) < 4611686018427387904.0))
        return fail(BF_ERR_INVALID, "bf_psr_model_from_spin: f1 * row_seconds^2 = %g turns per row^2 is outside (-1/4, 1/4)", (f1_hz_s * row_seconds) * row_seconds);
    model->ddphase = (int64_t)dd;
    model->dphase = turns_to_u64(x) + (uint64_t)(model->ddphase >> 1);
    model->phase0 = turns_to_u64(phase0_turns);
    model->epoch_row = epoch_row;
    return BF_OK;
}

size_t bf_psr_entries(int n_psr, int n_freq_total, int n_bins, int n_beams)
{
    if (n_psr < 1 || n_psr > dsabf::kPsrMaxPulsars || n_freq_total < 1 || n_beams < 1 || n_bins < dsabf::kPsrMinBins || n_bins > dsabf::kPsrMaxBins) return 0;
    return (size_t)n_psr * (size_t)n_freq_total * (size_t)n_bins * (size_t)n_beams;
}

int bf_psr_create(bf_handle* h, int n_freq_total, int max_rows_per_push, int n_bins, const bf_psr_model* models, const int32_t* delays, int n_psr,
                  int max_in_flight, bf_psr** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_freq_total < 1 || max_rows_per_push < 1 || max_in_flight < 1)
        return fail(BF_ERR_INVALID, "bf_psr_create: need n_freq_total, max_rows_per_push, max_in_flight >= 1");
    if (n_bins < dsabf::kPsrMinBins || n_bins > dsabf::kPsrMaxBins)
        return fail(BF_ERR_INVALID, "bf_psr_create: n_bins must be %d .. %d, not %d", dsabf::kPsrMinBins, dsabf::kPsrMaxBins, n_bins);
    if (n_psr < 1 || n_psr > dsabf::kPsrMaxPulsars) return fail(BF_ERR_INVALID, "bf_psr_create: n_psr must be 1 .. %d, not %d", dsabf::kPsrMaxPulsars, n_psr);
    if (!models || !delays) return fail(BF_ERR_INVALID, "bf_psr_create: NULL argument");
    for (size_t i = 0; i < (size_t)n_psr * n_freq_total; i++)
        if (delays[i] < 0) return fail(BF_ERR_INVALID, "bf_psr_create: delays must be >= 0 (delay[%zu] = %d)", i, delays[i]);
    if (!h) return fail(BF_ERR_INVALID, "bf_psr_create: the handle is NULL");
    ON_DEVICE(h);
    bf_psr* p = new (std::nothrow) bf_psr();
    if (!p) return fail(BF_ERR_DEVICE, "out of host memory");
    p->h = h;
    p->n_freq = n_freq_total;
    p->n_beams = h->cfg.n_beams;
    p->max_rows = max_rows_per_push;
    p->n_bins = n_bins;
    p->n_psr = n_psr;
    for (int k = 0; k < n_psr; k++) {
        p->model[k] = models[k];
        const int32_t* d = delays + (size_t)k * n_freq_total;
        p->delay_min[k] = *std::min_element(d, d + n_freq_total);
        p->delay_max[k] = *std::max_element(d, d + n_freq_total);
    }
    p->n_prof = bf_psr_entries(n_psr, n_freq_total, n_bins, p->n_beams);
    p->n_hits = p->n_prof / (size_t)p->n_beams;
    bf_resources& res = p->res;
    p->acc.create(res, p->n_prof * sizeof(double) + p->n_hits * sizeof(uint64_t), max_in_flight);
    res.dev(&p->d_delays, (size_t)n_psr * n_freq_total * sizeof(int32_t));
    if (res.err == hipSuccess) res.err = hipMemcpy(p->d_delays, delays, (size_t)n_psr * n_freq_total * sizeof(int32_t), hipMemcpyHostToDevice);
    res.device_sync();
    if (int rc = stage_adopt(p, "bf_psr_create")) return rc;
    *out = p;
    return BF_OK;
}

int bf_psr_destroy(bf_psr* p) { return stage_destroy(p); }

int bf_psr_push(bf_psr* p, const float* d_rows, int n_rows, void* hip_stream)
{
    if (!p || !d_rows) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(p)) return rc;
    if (int rc = psr_check_push(p, n_rows)) return rc;
    if ((uintptr_t)d_rows & 3) return fail(BF_ERR_INVALID, "misaligned device pointer: d_rows must be 4-byte aligned");
    ON_DEVICE(p->h);
    hipStream_t q = as_stream(hip_stream);
    dsabf::PsrFoldArgs a{};
    for (int k = 0; k < p->n_psr; k++) {
        const bf_psr_model& m = p->model[k];
        a.osc[k] = {m.phase0, m.dphase, m.ddphase, (int64_t)((__int128)p->pushed - (__int128)m.epoch_row)};
    }
    a.delays = p->d_delays;
    a.profile = reinterpret_cast<double*>(p->acc.d_acc);
    a.hits = reinterpret_cast<unsigned long long*>(p->acc.d_acc + p->n_prof * sizeof(double));
    a.n_psr = p->n_psr;
    a.n_freq = p->n_freq;
    a.n_bins = p->n_bins;
    a.n_beams = p->n_beams;
    // behind whatever used the accumulators last, and the new end of that chain
    HIP_TRY(p->acc.chain.wait(q));
    HIP_TRY(dsabf::launch_psr_fold(d_rows, n_rows, a, q));
    HIP_TRY(p->acc.chain.extend(q));
    p->pushed += (uint64_t)n_rows;
    return BF_OK;
}

// (the dump never holds the caller's queue: it is ordered by the stage's own chain)
int bf_psr_dump(bf_psr* p, void* hip_stream)
{
    (void)hip_stream;
    if (!p) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(p)) return rc;
    if (!p->acc.ring.room())
        return fail(BF_ERR_STATE, "bf_psr_dump: %d dumps are uncollected (max_in_flight): bf_psr_collect first", p->acc.ring.max_in_flight);
    ON_DEVICE(p->h);
    if (int rc = p->acc.dump(p->first_row, p->pushed - p->first_row)) return rc;
    p->first_row = p->pushed;
    return BF_OK;
}

int bf_psr_collect(bf_psr* p, double* profile, uint64_t* hits, uint64_t* first_row, uint64_t* n_rows)
{
    if (!p || !profile || !hits) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(p)) return rc;
    if (!p->acc.ring.pending()) return fail(BF_ERR_STATE, "bf_psr_collect: no dump is pending");
    ON_DEVICE(p->h);
    const char* h_acc = nullptr;
    uint64_t record[2];
    if (int rc = p->acc.collect(&h_acc, record)) return rc;
    std::memcpy(profile, h_acc, p->n_prof * sizeof(double));
    std::memcpy(hits, h_acc + p->n_prof * sizeof(double), p->n_hits * sizeof(uint64_t));
    if (first_row) *first_row = record[0];
    if (n_rows) *n_rows = record[1];
    return BF_OK;
}

int bf_psr_pending(const bf_psr* p) { return p ? p->acc.ring.pending() : fail(BF_ERR_INVALID, "the stage is NULL"); }

// median of v[0 .. n) (n >= 1), which it sorts ascending
static double median_sorted(std::vector<double>& v)
{
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) * 0.5;
}

int bf_psr_beam_snr(const double* profile_k, const uint64_t* hits_k, int n_freq_total, int n_bins, int n_beams, const uint8_t* chan_mask, double* snr,
                    int32_t* peak_bin)
{
    if (!profile_k || !hits_k || !snr || !peak_bin) return fail(BF_ERR_INVALID, "bf_psr_beam_snr: NULL argument");
    if (n_freq_total < 1 || n_bins < 1 || n_beams < 1) return fail(BF_ERR_INVALID, "bf_psr_beam_snr: need n_freq_total, n_bins, n_beams >= 1");
    std::vector<uint64_t> H((size_t)n_bins, 0);
    for (int f = 0; f < n_freq_total; f++)
        if (!chan_mask || !chan_mask[f])
            for (int j = 0; j < n_bins; j++) H[(size_t)j] += hits_k[(size_t)f * n_bins + j];
    std::vector<double> m, dev;
    std::vector<int> live;
    for (int j = 0; j < n_bins; j++)
        if (H[(size_t)j] > 0) live.push_back(j);
    for (int b = 0; b < n_beams; b++) {
        snr[b] = 0.0;
        peak_bin[b] = -1;
        if (live.size() < 4) continue;
        m.clear();
        for (int j : live) {
            double S = 0.0;
            for (int f = 0; f < n_freq_total; f++)
                if (!chan_mask || !chan_mask[f]) S = S + profile_k[((size_t)f * n_bins + j) * n_beams + b];
            m.push_back(S / (double)H[(size_t)j]);
        }
        size_t best = 0;
        for (size_t i = 1; i < m.size(); i++)
            if (m[i] > m[best]) best = i;
        const double top = m[best];
        dev = m;
        const double med = median_sorted(dev);
        for (size_t i = 0; i < m.size(); i++) dev[i] = std::fabs(m[i] - med);
        const double sigma = 1.4826 * median_sorted(dev);
        if (!(sigma > 0.0)) continue;
        snr[b] = (top - med) / sigma;
        peak_bin[b] = live[best];
    }
    return BF_OK;
}

}  // extern "C"
