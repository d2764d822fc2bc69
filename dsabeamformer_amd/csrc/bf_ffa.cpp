// bf_ffa.cpp -- the periodicity search behind the DM trials (include/dsabf.h: bf_ffa_*; contract, ordering and measurements:
// docs/PERIODICITY.md).  The device code is csrc/ffa/bf_ffa.hip; this file owns the series and the carried decimation state, cuts
// every push at the segment boundaries, orders the pushes whatever queues they come on (a bf_chain), keeps the result sets (a
// bf_result_ring: bf_runtime_internal.h) and selects the candidates.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "bf_runtime_internal.h"
#include "ffa/bf_ffa_kernels.h"

struct bf_ffa : bf_stage {
    bf_ffa() : bf_stage("periodicity stage") {}
    int n_dm = 0, dm_first = 0, tdec = 0, n_seg = 0, n_oct = 0, p_lo = 0, p_hi = 0, n_widths = 0, max_t = 0, n_beams = 0;
    double threshold = 0;
    int det_blk = 0, det_win = 0;   // bf_ffa_set_detrend: samples per block and blocks per median window; det_blk == 0: off
    // Two series slots: segment s is decimated into slot s % 2 and searched there while the samples behind it go to the other one.
    // A slot holds the octaves one behind the other, each [n_dm][n_beams][n_seg >> o].
    float* d_slot[2] = {nullptr, nullptr};
    // The decimation group in progress, [n_dm][n_beams]: push j reads d_carry[j % 2] and writes d_carry[(j + 1) % 2] (the thread
    // that closes the carried group and the one that leaves the next one open are different threads of one launch).
    float* d_carry[2] = {nullptr, nullptr};
    uint64_t n_in = 0;        // input samples the stage has been given
    uint64_t seg_first = 0;   // first_row of the segment in progress (set by the push that brings its first sample)
    bf_chain pushes;          // the pushes share the slots and the carry; pushes.n is j above
    struct result_set : bf_result_set {
        bf_ffa_peak *d_peaks = nullptr, *h_peaks = nullptr;
        bf_ffa_stat *d_stats = nullptr, *h_stats = nullptr;
        hipEvent_t kernels_done = nullptr;
        uint64_t first_row = 0;
    };
    bf_result_ring<result_set> ring;   // one issue per segment searched
    std::vector<bf_ffa_peak> last_peaks;
    std::vector<bf_ffa_stat> last_stats;
    uint64_t last_first_row = 0;
    size_t n_db() const { return (size_t)n_dm * n_beams; }
    size_t n_rec() const { return (size_t)n_oct * (p_hi - p_lo) * n_widths * n_db(); }
    uint64_t seg_rows() const { return (uint64_t)n_seg * (uint64_t)tdec; }
};

bf_stage* dsabf::rt::as_stage(bf_ffa* s) { return s; }

int dsabf::rt::ffa_check_attach(const bf_ffa* s, const bf_handle* h, int n_dm, int max_rows)
{
    if (int rc = orphaned(s)) return rc;
    if (s->h != h) return fail(BF_ERR_INVALID, "bf_dm_stream_attach_periodicity: the two stages belong to different handles");
    if (s->n_dm != n_dm) return fail(BF_ERR_INVALID, "bf_dm_stream_attach_periodicity: the periodicity stage has %d trials, the DM stage %d", s->n_dm, n_dm);
    if (s->max_t < max_rows)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_periodicity: max_t_per_push %d < max_rows_per_push %d", s->max_t, max_rows);
    if (s->feeder) return fail(BF_ERR_STATE, "bf_dm_stream_attach_periodicity: the periodicity stage is attached to another DM stage");
    return BF_OK;
}

// What a push of n_t times is refused for, before anything is queued: the count, and result sets for the segments it completes.
int dsabf::rt::ffa_check_push(const bf_ffa* s, int n_t)
{
    if (n_t < 1 || n_t > s->max_t) return fail(BF_ERR_INVALID, "n_t must be 1 .. %d (max_t_per_push)", s->max_t);
    const uint64_t completes = (s->n_in + (uint64_t)n_t) / s->seg_rows() - s->n_in / s->seg_rows();
    if (completes && !s->ring.room(completes))
        return fail(BF_ERR_STATE, "bf_ffa_push: %llu segments are uncollected and this push completes %llu more (max_in_flight %d): bf_ffa_collect first",
                    (unsigned long long)s->ring.pending(), (unsigned long long)completes, s->ring.max_in_flight);
    return BF_OK;
}

// The bounds of docs/PERIODICITY.md section 1 that need no device; `who` names the caller in the message.
static int ffa_check_shape(const char* who, int tdec, int n_seg, int n_oct, int p_lo, int p_hi, int n_widths)
{
    if (tdec < 1 || tdec > BF_FFA_MAX_DEC) return fail(BF_ERR_INVALID, "%s: tdec must be 1 .. %d, not %d", who, BF_FFA_MAX_DEC, tdec);
    if (n_oct < 1 || n_oct > BF_FFA_MAX_OCT) return fail(BF_ERR_INVALID, "%s: n_oct must be 1 .. %d, not %d", who, BF_FFA_MAX_OCT, n_oct);
    if (n_seg < 1 || n_seg > BF_FFA_MAX_SEG) return fail(BF_ERR_INVALID, "%s: n_seg must be 1 .. %d, not %d", who, BF_FFA_MAX_SEG, n_seg);
    if (n_seg % (1 << (n_oct - 1))) return fail(BF_ERR_INVALID, "%s: n_seg %d is no multiple of 2^(n_oct-1) = %d", who, n_seg, 1 << (n_oct - 1));
    if (p_lo < BF_FFA_MIN_PERIOD || p_hi <= p_lo || p_hi > BF_FFA_MAX_PERIOD)
        return fail(BF_ERR_INVALID, "%s: need %d <= p_lo < p_hi <= %d, not %d, %d", who, BF_FFA_MIN_PERIOD, BF_FFA_MAX_PERIOD, p_lo, p_hi);
    if (n_widths < 1 || n_widths > BF_FFA_MAX_WIDTHS || (1 << (n_widths - 1)) > p_lo / 2)
        return fail(BF_ERR_INVALID, "%s: n_widths must be 1 .. %d with 2^(n_widths-1) <= p_lo / 2, not %d at p_lo %d", who, BF_FFA_MAX_WIDTHS, n_widths, p_lo);
    for (int o = 0; o < n_oct; o++)
        for (int p = p_lo; p < p_hi; p++)
            if (dsabf::ffa_rows(n_seg >> o, p) < 2)
                return fail(BF_ERR_INVALID, "%s: octave %d (%d samples) holds fewer than 2 rows of period %d", who, o, n_seg >> o, p);
    return BF_OK;
}

extern "C" {

size_t bf_ffa_entries(int n_oct, int p_lo, int p_hi, int n_widths, int n_dm, int n_beams)
{
    if (n_oct < 1 || n_oct > BF_FFA_MAX_OCT || p_lo < BF_FFA_MIN_PERIOD || p_hi <= p_lo || p_hi > BF_FFA_MAX_PERIOD || n_widths < 1 ||
        n_widths > BF_FFA_MAX_WIDTHS || n_dm < 1 || n_beams < 1)
        return 0;
    return (size_t)n_oct * (size_t)(p_hi - p_lo) * (size_t)n_widths * (size_t)n_dm * (size_t)n_beams;
}

int bf_ffa_rows_of(int len, int p) { return dsabf::ffa_rows(len, p); }

int bf_ffa_create(bf_handle* h, int n_dm, int dm_first, int tdec, int n_seg, int n_oct, int p_lo, int p_hi, int n_widths, int max_t_per_push,
                  int max_in_flight, double threshold, bf_ffa** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = ffa_check_shape("bf_ffa_create", tdec, n_seg, n_oct, p_lo, p_hi, n_widths)) return rc;
    if (n_dm <= 0 || n_dm > 65535 || dm_first < 0 || max_t_per_push <= 0 || max_in_flight <= 0)
        return fail(BF_ERR_INVALID, "bf_ffa_create: need 0 < n_dm <= 65535, dm_first >= 0, max_t_per_push, max_in_flight > 0");
    if (!(threshold == threshold)) return fail(BF_ERR_INVALID, "bf_ffa_create: threshold is NaN");
    if (!h) return fail(BF_ERR_INVALID, "bf_ffa_create: the handle is NULL");
    if (h->cfg.n_beams % 4) return fail(BF_ERR_INVALID, "bf_ffa_create: n_beams %d is no multiple of 4", h->cfg.n_beams);
    ON_DEVICE(h);
    bf_ffa* s = new (std::nothrow) bf_ffa();
    if (!s) return fail(BF_ERR_DEVICE, "out of host memory");
    s->h = h;
    s->n_dm = n_dm;
    s->dm_first = dm_first;
    s->tdec = tdec;
    s->n_seg = n_seg;
    s->n_oct = n_oct;
    s->p_lo = p_lo;
    s->p_hi = p_hi;
    s->n_widths = n_widths;
    s->max_t = max_t_per_push;
    s->threshold = threshold;
    s->n_beams = h->cfg.n_beams;
    const size_t n_db = s->n_db(), n_rec = s->n_rec();
    const size_t slot_floats = dsabf::ffa_octave_offset(n_oct, n_seg, n_db);
    bf_resources& res = s->res;
    for (int k = 0; k < 2; k++) {
        res.dev(&s->d_slot[k], slot_floats * sizeof(float));
        res.dev(&s->d_carry[k], n_db * sizeof(float));
    }
    s->pushes.create(res);
    s->ring.create(res, max_in_flight);
    for (auto& r : s->ring.sets) {
        res.dev(&r.d_peaks, n_rec * sizeof(bf_ffa_peak));
        res.dev(&r.d_stats, n_db * sizeof(bf_ffa_stat));
        res.host(&r.h_peaks, n_rec * sizeof(bf_ffa_peak));
        res.host(&r.h_stats, n_db * sizeof(bf_ffa_stat));
        res.event(&r.kernels_done);
    }
    if (int rc = stage_adopt(s, "bf_ffa_create")) return rc;
    *out = s;
    return BF_OK;
}

int bf_ffa_destroy(bf_ffa* s) { return stage_destroy(s); }

int bf_ffa_set_detrend(bf_ffa* s, int blk, int win)
{
    if (blk != 0) {   // (the bounds that need no stage first, as bf_ffa_create checks its shape before its handle)
        if (blk < 1 || blk > BF_FFA_MAX_DETREND_BLK || (blk & (blk - 1)))
            return fail(BF_ERR_INVALID, "bf_ffa_set_detrend: blk must be 0 (off) or a power of two 1 .. %d, not %d", BF_FFA_MAX_DETREND_BLK, blk);
        if (win < 1 || win > BF_FFA_MAX_DETREND_WIN || !(win & 1))
            return fail(BF_ERR_INVALID, "bf_ffa_set_detrend: win must be odd, 1 .. %d, not %d", BF_FFA_MAX_DETREND_WIN, win);
    }
    if (!s) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (int rc = orphaned(s)) return rc;
    if (s->pushes.n) return fail(BF_ERR_STATE, "bf_ffa_set_detrend: the stage has taken a push; the detrend is set before the first");
    if (blk != 0 && s->n_seg % blk) return fail(BF_ERR_INVALID, "bf_ffa_set_detrend: n_seg %d is no multiple of blk %d", s->n_seg, blk);
    s->det_blk = blk;
    s->det_win = blk ? win : 0;
    return BF_OK;
}

int bf_ffa_detrend(const bf_ffa* s, int* blk, int* win)
{
    if (!s) return fail(BF_ERR_INVALID, "the stage is NULL");
    if (blk) *blk = s->det_blk;
    if (win) *win = s->det_win;
    return BF_OK;
}

int bf_ffa_pending(const bf_ffa* s) { return s ? s->ring.pending() : fail(BF_ERR_INVALID, "the stage is NULL"); }

int bf_ffa_push(bf_ffa* s, const float* d_chunk, int n_t, uint64_t first_t, void* hip_stream)
{
    if (!s || !d_chunk) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (int rc = ffa_check_push(s, n_t)) return rc;
    if ((uintptr_t)d_chunk & 15) return fail(BF_ERR_INVALID, "misaligned device pointer: d_chunk must be 16-byte aligned");
    ON_DEVICE(s->h);
    hipStream_t q = as_stream(hip_stream);
    HIP_TRY(s->pushes.wait(q));
    const float* carry_in = s->d_carry[s->pushes.n % 2];
    float* carry_out = s->d_carry[(s->pushes.n + 1) % 2];
    const int c0 = (int)(s->n_in % (uint64_t)s->tdec);                     // samples the group in progress already holds
    const uint64_t dec0 = s->n_in / (uint64_t)s->tdec;                     // decimated samples in front of this push
    const int n_complete = (int)(((uint64_t)c0 + (uint64_t)n_t) / (uint64_t)s->tdec);
    const bool open_end = ((uint64_t)c0 + (uint64_t)n_t) % (uint64_t)s->tdec != 0;   // the push leaves a group open
    // one launch per segment the push touches; the open group rides with the last of them (or is a launch of its own)
    int g = 0;
    while (g < n_complete || (open_end && g == n_complete)) {
        const uint64_t u = dec0 + (uint64_t)g;
        const uint64_t seg = u / (uint64_t)s->n_seg;
        const int pos = (int)(u % (uint64_t)s->n_seg);
        int cnt = n_complete - g < s->n_seg - pos ? n_complete - g : s->n_seg - pos;   // complete groups of this launch
        // (the segment's first sample may have come with an earlier push, as part of the carried group: then g == 0 and the offset is -c0)
        if (pos == 0 && cnt > 0) s->seg_first = first_t + (uint64_t)((int64_t)g * s->tdec - (int64_t)c0);
        const bool closes = cnt > 0 && pos + cnt == s->n_seg;
        const bool with_open = open_end && g + cnt == n_complete;
        float* slot = s->d_slot[seg % 2];
        HIP_TRY(dsabf::launch_ffa_decimate(d_chunk, s->n_dm, n_t, s->n_beams, s->tdec, c0, g, cnt + (with_open ? 1 : 0), carry_in, carry_out, slot, s->n_seg,
                                           pos, q));
        g += cnt + (with_open ? 1 : 0);
        if (closes) {
            if (s->det_blk) HIP_TRY(dsabf::launch_ffa_detrend(slot, s->n_dm, s->n_beams, s->n_seg, s->det_blk, s->det_win, q));
            bf_ffa::result_set& r = s->ring.next();
            HIP_TRY(dsabf::launch_ffa_search(slot, s->n_dm, s->n_beams, s->n_seg, s->n_oct, s->p_lo, s->p_hi, s->n_widths, r.d_peaks, r.d_stats, q));
            HIP_TRY(hipEventRecord(r.kernels_done, q));
            HIP_TRY(hipStreamWaitEvent(s->ring.copy_q, r.kernels_done, 0));
            HIP_TRY(hipMemcpyAsync(r.h_peaks, r.d_peaks, s->n_rec() * sizeof(bf_ffa_peak), hipMemcpyDeviceToHost, s->ring.copy_q));
            HIP_TRY(hipMemcpyAsync(r.h_stats, r.d_stats, s->n_db() * sizeof(bf_ffa_stat), hipMemcpyDeviceToHost, s->ring.copy_q));
            HIP_TRY(hipEventRecord(r.copied, s->ring.copy_q));
            r.first_row = s->seg_first;
            s->ring.issued();
        }
    }
    HIP_TRY(s->pushes.extend(q));
    s->n_in += (uint64_t)n_t;
    return BF_OK;
}

int bf_ffa_collect(bf_ffa* s, bf_ffa_candidate* out, size_t max_out, size_t* n_out)
{
    if (!s || !out || !n_out) return fail(BF_ERR_INVALID, "NULL argument");
    *n_out = 0;
    if (max_out < s->n_db())
        return fail(BF_ERR_INVALID, "bf_ffa_collect: room for %zu candidates, a segment can give n_dm * n_beams = %zu", max_out, s->n_db());
    if (int rc = orphaned(s)) return rc;
    if (!s->ring.pending()) return fail(BF_ERR_STATE, "bf_ffa_collect: no segment is pending");
    ON_DEVICE(s->h);
    HIP_TRY(s->ring.wait_oldest());
    const bf_ffa::result_set& r = s->ring.oldest();
    s->last_peaks.assign(r.h_peaks, r.h_peaks + s->n_rec());
    s->last_stats.assign(r.h_stats, r.h_stats + s->n_db());
    s->last_first_row = r.first_row;
    s->ring.collected();
    return bf_ffa_select(s->last_peaks.data(), s->last_stats.data(), s->tdec, s->n_seg, s->n_oct, s->p_lo, s->p_hi, s->n_widths, s->n_dm, s->n_beams,
                         s->last_first_row, s->seg_rows(), s->dm_first, s->threshold, out, max_out, n_out);
}

int bf_ffa_last_records(const bf_ffa* s, const bf_ffa_peak** peaks, const bf_ffa_stat** stats, uint64_t* first_row, uint64_t* n_rows)
{
    if (!s) return fail(BF_ERR_INVALID, "NULL argument");
    if (s->last_peaks.empty()) return fail(BF_ERR_STATE, "bf_ffa_last_records: nothing has been collected yet");
    if (peaks) *peaks = s->last_peaks.data();
    if (stats) *stats = s->last_stats.data();
    if (first_row) *first_row = s->last_first_row;
    if (n_rows) *n_rows = s->seg_rows();
    return BF_OK;
}

int bf_ffa_select(const bf_ffa_peak* peaks, const bf_ffa_stat* stats, int tdec, int n_seg, int n_oct, int p_lo, int p_hi, int n_widths, int n_dm,
                  int n_beams, uint64_t first_row, uint64_t n_rows, int dm_first, double threshold, bf_ffa_candidate* out, size_t max_out,
                  size_t* n_out)
{
    if (!peaks || !stats || !n_out || (!out && max_out)) return fail(BF_ERR_INVALID, "NULL argument");
    *n_out = 0;
    if (int rc = ffa_check_shape("bf_ffa_select", tdec, n_seg, n_oct, p_lo, p_hi, n_widths)) return rc;
    if (n_dm <= 0 || n_beams <= 0) return fail(BF_ERR_INVALID, "bf_ffa_select: need n_dm, n_beams > 0");
    const size_t n_db = (size_t)n_dm * n_beams;
    const int n_p = p_hi - p_lo;
    size_t m = 0;
    for (size_t i = 0; i < n_db; i++) {
        const double mu = stats[i].sum / (double)n_seg;
        const double var = stats[i].sumsq / (double)n_seg - mu * mu;
        const double sigma = std::sqrt(var > 0.0 ? var : 0.0);
        if (sigma == 0.0) continue;
        bool have = false;
        double best = 0.0;
        int bo = 0, bp = 0, bk = 0, bM = 0;
        for (int o = 0; o < n_oct; o++) {
            const double o2 = (double)(1 << o);
            const double mu_o = o2 * mu, sigma_o = sigma * std::sqrt(o2);
            for (int p = p_lo; p < p_hi; p++) {
                const int M = dsabf::ffa_rows(n_seg >> o, p);
                for (int k = 0; k < n_widths; k++) {
                    const bf_ffa_peak& r = peaks[(((size_t)o * n_p + (p - p_lo)) * n_widths + k) * n_db + i];
                    const double wM = (double)(1 << k) * (double)M;
                    const double snr = ((double)r.value - wM * mu_o) / (sigma_o * std::sqrt(wM));
                    if (!have || snr > best) {   // (strictly: the lowest o, then p, then k keeps a tie)
                        have = true;
                        best = snr;
                        bo = o;
                        bp = p;
                        bk = k;
                        bM = M;
                    }
                }
            }
        }
        if (!have || !(best >= threshold)) continue;
        if (m >= max_out) return fail(BF_ERR_INVALID, "bf_ffa_select: more than max_out = %zu candidates", max_out);
        const bf_ffa_peak& r = peaks[(((size_t)bo * n_p + (bp - p_lo)) * n_widths + bk) * n_db + i];
        bf_ffa_candidate c;
        std::memset(&c, 0, sizeof c);
        c.first_row = first_row;
        c.n_rows = n_rows;
        c.period_rows = ((double)tdec * (double)(1 << bo)) * ((double)bp + (double)r.shift / (double)(bM - 1));
        c.dm = dm_first + (int)(i / (size_t)n_beams);
        c.beam = (int)(i % (size_t)n_beams);
        c.octave = bo;
        c.p = bp;
        c.shift = r.shift;
        c.bin = r.bin;
        c.width = 1 << bk;
        c.snr = best;
        c.value = r.value;
        std::memcpy(&out[m++], &c, sizeof c);   // (the padding bytes too: zero)
    }
    *n_out = m;
    return BF_OK;
}

int bf_ffa_sift(const bf_ffa_candidate* in, size_t n, double tol, int max_harm, int dm_tol, bf_ffa_group* out, size_t max_out, size_t* n_out)
{
    if (!n_out) return fail(BF_ERR_INVALID, "NULL argument");
    *n_out = 0;
    if (!(tol >= 0.0 && tol < 1.0)) return fail(BF_ERR_INVALID, "bf_ffa_sift: tol must be in [0, 1)");
    if (max_harm < 1 || max_harm > BF_FFA_MAX_HARM) return fail(BF_ERR_INVALID, "bf_ffa_sift: max_harm must be 1 .. %d, not %d", BF_FFA_MAX_HARM, max_harm);
    if (dm_tol < 0) return fail(BF_ERR_INVALID, "bf_ffa_sift: dm_tol must be >= 0, not %d", dm_tol);
    if (n == 0) return BF_OK;
    if (!in || !out) return fail(BF_ERR_INVALID, "NULL argument");
    for (size_t i = 0; i < n; i++) {
        if (!(in[i].snr == in[i].snr)) return fail(BF_ERR_INVALID, "bf_ffa_sift: candidate %zu has a NaN snr", i);
        if (!(in[i].period_rows > 0.0)) return fail(BF_ERR_INVALID, "bf_ffa_sift: candidate %zu has a period_rows that is not > 0", i);
    }
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [in](size_t a, size_t b) { return in[a].snr > in[b].snr; });   // ties: the lower index first
    std::vector<bf_ffa_group> groups;
    std::vector<std::vector<int32_t>> beams;   // the distinct beams of a group
    for (size_t idx : order) {
        const bf_ffa_candidate& c = in[idx];
        bool joined = false;
        for (size_t g = 0; g < groups.size() && !joined; g++) {
            bf_ffa_group& grp = groups[g];
            const bf_ffa_candidate& hd = grp.head;
            if (c.first_row != hd.first_row || c.n_rows != hd.n_rows) continue;
            const int64_t ddm = (int64_t)c.dm - (int64_t)hd.dm;
            if (ddm > dm_tol || -ddm > dm_tol) continue;
            for (int a = 1; a <= max_harm && !joined; a++)
                for (int b = 1; b <= max_harm; b++)
                    if (std::fabs((c.period_rows * (double)b) / (hd.period_rows * (double)a) - 1.0) <= tol) {
                        grp.n_members++;
                        if (std::find(beams[g].begin(), beams[g].end(), c.beam) == beams[g].end()) beams[g].push_back(c.beam);
                        grp.dm_lo = std::min(grp.dm_lo, c.dm);
                        grp.dm_hi = std::max(grp.dm_hi, c.dm);
                        if (a != 1 || b != 1) grp.n_harmonic++;
                        joined = true;
                        break;
                    }
        }
        if (joined) continue;
        bf_ffa_group grp;
        std::memset(&grp, 0, sizeof grp);
        std::memcpy(&grp.head, &c, sizeof c);
        grp.n_members = 1;
        grp.dm_lo = grp.dm_hi = c.dm;
        groups.push_back(grp);
        beams.push_back(std::vector<int32_t>(1, c.beam));
    }
    if (groups.size() > max_out) return fail(BF_ERR_INVALID, "bf_ffa_sift: %zu groups, room for max_out = %zu", groups.size(), max_out);
    for (size_t g = 0; g < groups.size(); g++) {
        groups[g].n_beams = (int32_t)beams[g].size();
        std::memcpy(&out[g], &groups[g], sizeof(bf_ffa_group));
    }
    *n_out = groups.size();
    return BF_OK;
}

}  // extern "C"
