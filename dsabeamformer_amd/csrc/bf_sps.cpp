// bf_sps.cpp -- single-pulse search behind the DM stage (include/dsabf.h: bf_sps_*; contract and measurements: docs/SINGLE_PULSE.md).
// The device code is csrc/sps/bf_sps.hip; this file owns the stage's memory, orders its pushes (each behind the kernels of the one
// before it), keeps the result sets (a bf_result_ring: bf_runtime_internal.h) and selects the candidates.
#include <cmath>
#include <cstring>
#include <deque>
#include <new>

#include "bf_runtime_internal.h"
#include "sps/bf_sps_kernels.h"

struct bf_sps : bf_stage {
    bf_sps() : bf_stage("search stage") {}
    int n_dm = 0, dm_first = 0, n_widths = 0, halo = 0, max_t = 0, baseline = 0, n_beams = 0;
    uint64_t min_samples = 0;
    double threshold = 0;
    // The last `halo` = 2^(K-1) - 1 samples of every (trial, beam), [n_dm][halo][n_beams], zeros where the stream had none yet.
    // Two of them: push j reads d_tail[j % 2] (all its tiles do) while its finishing pass writes d_tail[(j + 1) % 2].
    float* d_tail[2] = {nullptr, nullptr};
    bf_sps_peak* d_part_peaks = nullptr;   // per-tile records of the push that is running (pushes run one after the other)
    bf_sps_stat* d_part_stats = nullptr;
    // Push j = ring.n_issued leaves its records in set j % max_in_flight: on the device, then -- on the stage's own copy queue, so that the queue
    // the chunk came from goes on as soon as the kernels have read it -- in pinned host memory.
    struct result_set : bf_result_set {
        bf_sps_peak *d_peaks = nullptr, *h_peaks = nullptr;
        bf_sps_stat *d_stats = nullptr, *h_stats = nullptr;
        hipEvent_t kernels_done = nullptr;
        uint64_t first_t = 0;
        int n_t = 0;
    };
    bf_result_ring<result_set> ring;
    uint64_t seen = 0;                     // samples of the series in front of the next push
    // the push last collected (bf_sps_last_records) and the statistics of the last `baseline` collected pushes, oldest first
    std::vector<bf_sps_peak> last_peaks;
    std::vector<bf_sps_stat> last_stats, totals;
    uint64_t last_first_t = 0;
    int last_n_t = 0;
    std::deque<std::pair<int, std::vector<bf_sps_stat>>> window;
};

bf_stage* dsabf::rt::as_stage(bf_sps* s) { return s; }

int dsabf::rt::sps_check_attach(const bf_sps* s, const bf_handle* h, int n_dm, int max_rows)
{
    if (int rc = orphaned(s)) return rc;
    if (s->h != h) return fail(BF_ERR_INVALID, "bf_dm_stream_attach_search: the two stages belong to different handles");
    if (s->n_dm != n_dm) return fail(BF_ERR_INVALID, "bf_dm_stream_attach_search: the search stage has %d trials, the DM stage %d", s->n_dm, n_dm);
    if (s->max_t < max_rows)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_search: max_t_per_push %d < max_rows_per_push %d", s->max_t, max_rows);
    if (s->feeder) return fail(BF_ERR_STATE, "bf_dm_stream_attach_search: the search stage is attached to another DM stage");
    return BF_OK;
}

int dsabf::rt::sps_max_in_flight(const bf_sps* s) { return s->ring.max_in_flight; }

extern "C" {

int bf_sps_create(bf_handle* h, int n_dm, int dm_first, int n_widths, int max_t_per_push, int max_in_flight, int baseline_pushes,
                  int min_samples, double threshold, bf_sps** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_widths < 1 || n_widths > dsabf::kSpsMaxWidths)
        return fail(BF_ERR_INVALID, "bf_sps_create: n_widths must be 1 .. %d (boxcar widths 1 .. 2^(n_widths-1)), not %d", dsabf::kSpsMaxWidths, n_widths);
    if (!h) return fail(BF_ERR_INVALID, "bf_sps_create: the handle is NULL");
    if (n_dm <= 0 || n_dm > 65535 || dm_first < 0 || max_t_per_push <= 0 || max_in_flight <= 0 || baseline_pushes <= 0 || min_samples < 0)
        return fail(BF_ERR_INVALID, "bf_sps_create: need 0 < n_dm <= 65535, dm_first >= 0, max_t_per_push, max_in_flight, baseline_pushes > 0, min_samples >= 0");
    if (!(threshold == threshold)) return fail(BF_ERR_INVALID, "bf_sps_create: threshold is NaN");
    ON_DEVICE(h);
    bf_sps* s = new (std::nothrow) bf_sps();
    if (!s) return fail(BF_ERR_DEVICE, "out of host memory");
    s->h = h;
    s->n_dm = n_dm;
    s->dm_first = dm_first;
    s->n_widths = n_widths;
    s->halo = dsabf::sps_halo(n_widths);
    s->max_t = max_t_per_push;
    s->baseline = baseline_pushes;
    s->min_samples = (uint64_t)min_samples;
    s->threshold = threshold;
    s->n_beams = h->cfg.n_beams;
    const size_t n_db = (size_t)n_dm * s->n_beams, n_rec = (size_t)n_widths * n_db, tiles = (size_t)dsabf::sps_tiles(max_t_per_push);
    const size_t tail_bytes = n_db * s->halo * sizeof(float);
    bf_resources& res = s->res;
    for (int k = 0; k < 2 && tail_bytes; k++) res.dev(&s->d_tail[k], tail_bytes, true);
    res.dev(&s->d_part_peaks, tiles * n_rec * sizeof(bf_sps_peak));
    res.dev(&s->d_part_stats, tiles * n_db * sizeof(bf_sps_stat));
    s->ring.create(res, max_in_flight);
    for (auto& r : s->ring.sets) {
        res.dev(&r.d_peaks, n_rec * sizeof(bf_sps_peak));
        res.dev(&r.d_stats, n_db * sizeof(bf_sps_stat));
        res.host(&r.h_peaks, n_rec * sizeof(bf_sps_peak));
        res.host(&r.h_stats, n_db * sizeof(bf_sps_stat));
        res.event(&r.kernels_done);
    }
    res.device_sync();
    if (int rc = stage_adopt(s, "bf_sps_create")) return rc;
    *out = s;
    return BF_OK;
}

int bf_sps_destroy(bf_sps* s) { return stage_destroy(s); }

int bf_sps_pending(const bf_sps* s) { return s ? s->ring.pending() : BF_ERR_INVALID; }

int bf_sps_push(bf_sps* s, const float* d_chunk, int n_t, uint64_t first_t, void* hip_stream)
{
    if (!s || !d_chunk) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_t <= 0 || n_t > s->max_t) return fail(BF_ERR_INVALID, "n_t must be 1 .. %d (max_t_per_push)", s->max_t);
    if (int rc = orphaned(s)) return rc;
    if (!s->ring.room())
        return fail(BF_ERR_STATE, "bf_sps_push: %d pushes are uncollected (max_in_flight): bf_sps_collect first", s->ring.max_in_flight);
    bf_handle* h = s->h;
    ON_DEVICE(h);
    hipStream_t q = as_stream(hip_stream);
    const uint64_t j = s->ring.n_issued;
    bf_sps::result_set& r = s->ring.next();
    // behind the kernels of the push before this one, whatever queue they ran on: they wrote the tail this one reads, and the
    // per-tile records are shared
    if (j) HIP_TRY(hipStreamWaitEvent(q, s->ring.newest().kernels_done, 0));
    dsabf::SpsBuffers buf{s->d_tail[j % 2], s->d_tail[(j + 1) % 2], s->d_part_peaks, s->d_part_stats, r.d_peaks, r.d_stats};
    HIP_TRY(dsabf::launch_sps_push(d_chunk, s->n_dm, n_t, s->n_beams, s->n_widths, s->seen, buf, q));
    HIP_TRY(hipEventRecord(r.kernels_done, q));
    HIP_TRY(hipStreamWaitEvent(s->ring.copy_q, r.kernels_done, 0));
    const size_t n_db = (size_t)s->n_dm * s->n_beams;
    HIP_TRY(hipMemcpyAsync(r.h_peaks, r.d_peaks, s->n_widths * n_db * sizeof(bf_sps_peak), hipMemcpyDeviceToHost, s->ring.copy_q));
    HIP_TRY(hipMemcpyAsync(r.h_stats, r.d_stats, n_db * sizeof(bf_sps_stat), hipMemcpyDeviceToHost, s->ring.copy_q));
    HIP_TRY(hipEventRecord(r.copied, s->ring.copy_q));
    r.first_t = first_t;
    r.n_t = n_t;
    s->seen += (uint64_t)n_t;
    s->ring.issued();
    return BF_OK;
}

int bf_sps_collect(bf_sps* s, bf_sps_candidate* out, size_t max_out, size_t* n_out)
{
    if (!s || !out || !n_out) return fail(BF_ERR_INVALID, "NULL argument");
    *n_out = 0;
    const size_t n_db = (size_t)s->n_dm * s->n_beams;
    if (max_out < n_db) return fail(BF_ERR_INVALID, "bf_sps_collect: room for %zu candidates, a push can give n_dm * n_beams = %zu", max_out, n_db);
    if (int rc = orphaned(s)) return rc;
    if (!s->ring.pending()) return fail(BF_ERR_STATE, "bf_sps_collect: no push is pending");
    bf_handle* h = s->h;
    ON_DEVICE(h);
    HIP_TRY(s->ring.wait_oldest());
    const bf_sps::result_set& r = s->ring.oldest();
    s->last_peaks.assign(r.h_peaks, r.h_peaks + s->n_widths * n_db);
    s->last_stats.assign(r.h_stats, r.h_stats + n_db);
    s->last_first_t = r.first_t;
    s->last_n_t = r.n_t;
    s->ring.collected();
    s->window.emplace_back(r.n_t, s->last_stats);
    while (s->window.size() > (size_t)s->baseline) s->window.pop_front();
    uint64_t n = 0;
    s->totals.assign(n_db, bf_sps_stat{0.0, 0.0});
    for (const auto& w : s->window) {   // oldest first
        n += (uint64_t)w.first;
        for (size_t i = 0; i < n_db; i++) {
            s->totals[i].sum += w.second[i].sum;
            s->totals[i].sumsq += w.second[i].sumsq;
        }
    }
    return bf_sps_select(s->last_peaks.data(), s->totals.data(), n, s->n_widths, s->n_dm, s->n_beams, s->last_first_t, s->dm_first,
                         s->min_samples, s->threshold, out, max_out, n_out);
}

int bf_sps_last_records(const bf_sps* s, const bf_sps_peak** peaks, const bf_sps_stat** stats, uint64_t* first_t, int* n_t)
{
    if (!s) return fail(BF_ERR_INVALID, "NULL argument");
    if (s->last_peaks.empty()) return fail(BF_ERR_STATE, "bf_sps_last_records: nothing has been collected yet");
    if (peaks) *peaks = s->last_peaks.data();
    if (stats) *stats = s->last_stats.data();
    if (first_t) *first_t = s->last_first_t;
    if (n_t) *n_t = s->last_n_t;
    return BF_OK;
}

int bf_sps_select(const bf_sps_peak* peaks, const bf_sps_stat* totals, uint64_t n, int n_widths, int n_dm, int n_beams, uint64_t first_t,
                  int dm_first, uint64_t min_samples, double threshold, bf_sps_candidate* out, size_t max_out, size_t* n_out)
{
    if (!peaks || !totals || !n_out || (!out && max_out)) return fail(BF_ERR_INVALID, "NULL argument");
    *n_out = 0;
    if (n_widths < 1 || n_widths > dsabf::kSpsMaxWidths || n_dm <= 0 || n_beams <= 0)
        return fail(BF_ERR_INVALID, "bf_sps_select: need 1 <= n_widths <= %d, n_dm, n_beams > 0", dsabf::kSpsMaxWidths);
    if (n == 0 || n < min_samples) return BF_OK;
    const size_t n_db = (size_t)n_dm * n_beams;
    size_t m = 0;
    for (size_t i = 0; i < n_db; i++) {
        const double mu = totals[i].sum / (double)n;
        const double var = totals[i].sumsq / (double)n - mu * mu;
        const double sigma = std::sqrt(var > 0.0 ? var : 0.0);
        if (sigma == 0.0) continue;
        int best_k = -1;
        double best = 0.0;
        for (int k = 0; k < n_widths; k++) {
            const bf_sps_peak& p = peaks[(size_t)k * n_db + i];
            if (p.t_end < 0) continue;
            const double w = (double)(1 << k);
            const double snr = ((double)p.value - w * mu) / (sigma * std::sqrt(w));
            if (best_k < 0 || snr > best) {   // (strictly: the lowest k keeps a tie)
                best_k = k;
                best = snr;
            }
        }
        if (best_k < 0 || !(best >= threshold)) continue;
        if (m >= max_out) return fail(BF_ERR_INVALID, "bf_sps_select: more than max_out = %zu candidates", max_out);
        const bf_sps_peak& p = peaks[(size_t)best_k * n_db + i];
        bf_sps_candidate c;
        c.t_start = first_t + (uint64_t)p.t_end - (uint64_t)((1 << best_k) - 1);
        c.dm = dm_first + (int)(i / (size_t)n_beams);
        c.beam = (int)(i % (size_t)n_beams);
        c.width = 1 << best_k;
        c.peak = p.value;
        c.snr = best;
        out[m++] = c;
    }
    *n_out = m;
    return BF_OK;
}

}  // extern "C"
