// bf_inj.cpp -- the pulse injector (include/dsabf.h: bf_inj_*; contract, ordering and measurements: docs/INJECTION.md).  The device
// code is csrc/inj/bf_inj.hip; this file keeps the live pulses and their windows in host arithmetic, decides per apply what is
// launched, owns the pulses' device tables, and holds the three host helpers (a burst's profile, the nearest trial of a delay row,
// the recovery bookkeeping).
//
// Device memory and the applies in flight.  A pulse's tables (response, delay, profile) are ONE device allocation, written once inside
// the add, on a queue of the stage's own that the add waits for, before the pulse is in the list any apply launches from.  No queued
// kernel can read that allocation: it belongs to no live pulse.  It goes back to the stage when the pulse is spent, stamped with the
// number of the last apply that launched; an add takes it again only once the event behind that apply, and behind every apply before
// it, has completed (hipEventQuery, never a wait).  An add whose size no idle allocation fits takes fresh memory.  The applies
// themselves carry everything else by value in their kernel arguments: nothing on the device changes from one apply to the next.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <new>
#include <vector>

#include "bf_runtime_internal.h"
#include "inj/bf_inj_kernels.h"

struct bf_inj : bf_stage {
    bf_inj() : bf_stage("injector") {}
    int n_freq = 0, n_beams = 0, max_rows = 0, max_pulses = 0, max_width = 0;
    uint64_t next_row = 0;             // rows applied so far
    uint64_t launches = 0;             // kernels launched so far
    uint64_t next_id = 0;
    struct pulse {
        uint64_t id = 0;
        bool train = false;
        int64_t t0 = 0;                // burst
        int width = 0;                 // burst: W; train: n_bins
        bf_psr_model model{};          // train
        uint64_t first_row = 0, end_row = 0;   // train: rows [first_row, end_row), end_row saturated at UINT64_MAX
        int32_t delay_min = 0, delay_max = 0;
        std::vector<int32_t> delay;    // [n_freq]
        char* d_tables = nullptr;      // response float [n_beams] | delay int32 [n_freq] | profile float [n_freq][width]
        size_t bytes = 0;
    };
    std::vector<pulse> live;           // ascending id
    int n_trains = 0;
    // applies that launched, oldest first, and the event behind each; `completed`: every apply up to that number has ended
    struct launched {
        hipEvent_t ev;
        uint64_t seq;
    };
    std::deque<launched> in_flight;
    std::vector<hipEvent_t> spare_events;
    uint64_t seq = 0, completed = 0;
    struct idle_tables {
        char* d;
        size_t bytes;
        uint64_t seq;                  // free once completed >= seq
    };
    std::vector<idle_tables> idle;
    hipStream_t copy_q = nullptr;
    std::vector<char> staging;

    size_t table_bytes(int width) const { return ((size_t)n_beams + (size_t)n_freq + (size_t)n_freq * (size_t)width) * 4; }
    const float* d_response(const pulse& p) const { return reinterpret_cast<const float*>(p.d_tables); }
    const int32_t* d_delay(const pulse& p) const { return reinterpret_cast<const int32_t*>(p.d_tables + (size_t)n_beams * 4); }
    const float* d_profile(const pulse& p) const { return reinterpret_cast<const float*>(p.d_tables + ((size_t)n_beams + (size_t)n_freq) * 4); }
};

bf_stage* dsabf::rt::as_stage(bf_inj* s) { return s; }

int dsabf::rt::inj_check_attach(const bf_inj* s, const bf_handle* h, int n_freq_total, int max_rows, uint64_t pushed)
{
    if (int rc = orphaned(s)) return rc;
    if (s->h != h) return fail(BF_ERR_INVALID, "bf_dm_stream_attach_injector: the two stages belong to different handles");
    if (s->n_freq != n_freq_total)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_injector: the injector has %d channels, the DM stage %d", s->n_freq, n_freq_total);
    if (s->max_rows < max_rows)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_injector: max_rows_per_push %d < the DM stage's %d", s->max_rows, max_rows);
    if (s->feeder) return fail(BF_ERR_STATE, "bf_dm_stream_attach_injector: the injector is attached to another DM stage");
    if (s->next_row != pushed)
        return fail(BF_ERR_STATE, "bf_dm_stream_attach_injector: the injector has applied %llu rows, the DM stage has been pushed %llu",
                    (unsigned long long)s->next_row, (unsigned long long)pushed);
    return BF_OK;
}

// the rows [lo, hi) of an apply over [first, first + n) that lie inside a train's gate; lo >= hi: none
static void train_rows(const bf_inj::pulse& p, uint64_t first, int n, int* lo, int* hi)
{
    const uint64_t a = std::max(first, p.first_row), b = std::min(first + (uint64_t)n, p.end_row);
    *lo = a < b ? (int)(a - first) : 0;
    *hi = a < b ? (int)(b - first) : 0;
}

// What an apply of n_rows rows is refused for, before anything is queued: the row count, and a train's oscillator index outside
// (-2^31, 2^31) on the rows it covers (the folder's rule, psr_check_push).
int dsabf::rt::inj_check_apply(const bf_inj* s, int n_rows)
{
    if (n_rows < 1 || n_rows > s->max_rows) return fail(BF_ERR_INVALID, "n_rows must be 1 .. %d (max_rows_per_push)", s->max_rows);
    const __int128 lim = (__int128)1 << 31;
    for (const bf_inj::pulse& p : s->live) {
        if (!p.train) continue;
        int lo = 0, hi = 0;
        train_rows(p, s->next_row, n_rows, &lo, &hi);
        if (lo >= hi) continue;
        const __int128 base = (__int128)s->next_row - (__int128)p.model.epoch_row;
        if (base + lo - p.delay_max <= -lim || base + (hi - 1) - p.delay_min >= lim)
            return fail(BF_ERR_INVALID, "bf_inj_apply: train %llu would reach |row - epoch_row - delay| >= 2^31: re-anchor epoch_row",
                        (unsigned long long)p.id);
    }
    return BF_OK;
}

// the events of applies that have ended go back to the spares, in order; `completed` follows
static void inj_reap(bf_inj* s)
{
    while (!s->in_flight.empty() && hipEventQuery(s->in_flight.front().ev) == hipSuccess) {
        s->completed = s->in_flight.front().seq;
        s->spare_events.push_back(s->in_flight.front().ev);
        s->in_flight.pop_front();
    }
    (void)hipGetLastError();   // (hipErrorNotReady is no error of ours)
}

// Device tables for a new pulse: the smallest idle allocation that fits and that no apply in flight can read; else fresh memory,
// after giving back the idle ones that are too small and equally unread.
static int inj_tables(bf_inj* s, size_t bytes, char** out, size_t* out_bytes)
{
    inj_reap(s);
    int best = -1;
    for (int i = 0; i < (int)s->idle.size(); i++)
        if (s->idle[i].seq <= s->completed && s->idle[i].bytes >= bytes && (best < 0 || s->idle[i].bytes < s->idle[best].bytes)) best = i;
    if (best >= 0) {
        *out = s->idle[best].d;
        *out_bytes = s->idle[best].bytes;
        s->idle.erase(s->idle.begin() + best);
        return BF_OK;
    }
    for (size_t i = 0; i < s->idle.size();) {
        if (s->idle[i].seq > s->completed) {
            i++;
            continue;
        }
        std::vector<void*>& dev = s->res.device;
        dev.erase(std::remove(dev.begin(), dev.end(), (void*)s->idle[i].d), dev.end());
        (void)hipFree(s->idle[i].d);
        s->idle.erase(s->idle.begin() + (long)i);
    }
    char* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, bytes));
    s->res.device.push_back(d);
    *out = d;
    *out_bytes = bytes;
    return BF_OK;
}

// what both adds check of their tables, without a device
static int inj_check_tables(const bf_inj* s, const char* who, const int32_t* delay, const float* profile, const float* response)
{
    if (!delay || !profile || !response) return fail(BF_ERR_INVALID, "%s: NULL argument", who);
    for (int f = 0; f < s->n_freq; f++)
        if (delay[f] < 0) return fail(BF_ERR_INVALID, "%s: delays must be >= 0 (delay[%d] = %d)", who, f, delay[f]);
    return BF_OK;
}

// the tables go to the device and the pulse into the list; *p is complete but for d_tables / bytes / id
static int inj_store(bf_inj* s, bf_inj::pulse& p, const int32_t* delay, const float* profile, const float* response, uint64_t* id)
{
    ON_DEVICE(s->h);
    const size_t bytes = s->table_bytes(p.width);
    if (int rc = inj_tables(s, bytes, &p.d_tables, &p.bytes)) return rc;
    s->staging.resize(bytes);
    char* st = s->staging.data();
    std::memcpy(st, response, (size_t)s->n_beams * 4);
    std::memcpy(st + (size_t)s->n_beams * 4, delay, (size_t)s->n_freq * 4);
    std::memcpy(st + ((size_t)s->n_beams + (size_t)s->n_freq) * 4, profile, (size_t)s->n_freq * (size_t)p.width * 4);
    hipError_t e = hipMemcpyAsync(p.d_tables, st, bytes, hipMemcpyHostToDevice, s->copy_q);
    if (e == hipSuccess) e = hipStreamSynchronize(s->copy_q);
    if (e != hipSuccess) {
        s->idle.push_back({p.d_tables, p.bytes, 0});   // (nothing launched from it)
        return fail(BF_ERR_DEVICE, "bf_inj_add: the copy of the tables failed: %s", hipGetErrorString(e));
    }
    p.delay.assign(delay, delay + s->n_freq);
    p.delay_min = *std::min_element(p.delay.begin(), p.delay.end());
    p.delay_max = *std::max_element(p.delay.begin(), p.delay.end());
    p.id = s->next_id++;
    if (id) *id = p.id;
    s->n_trains += p.train;
    s->live.push_back(std::move(p));
    return BF_OK;
}

// does burst p touch a row of [first, first + n) in some channel?
static bool burst_overlaps(const bf_inj::pulse& p, uint64_t first, int n)
{
    const __int128 a = first, b = (__int128)first + n;
    if ((__int128)p.t0 + p.delay_max + p.width <= a || (__int128)p.t0 + p.delay_min >= b) return false;
    for (int32_t d : p.delay) {
        const __int128 lo = (__int128)p.t0 + d;
        if (lo < b && lo + p.width > a) return true;
    }
    return false;
}

// The apply itself (bf_inj_apply, and bf_dm_stream_push for an attached injector); inj_check_apply has passed.
int dsabf::rt::inj_apply(bf_inj* s, float* d_rows, int n_rows, hipStream_t q)
{
    if ((uintptr_t)d_rows & 15) return fail(BF_ERR_INVALID, "misaligned device pointer: d_rows must be 16-byte aligned");
    const uint64_t first = s->next_row;
    std::vector<const bf_inj::pulse*> bursts, trains;
    for (const bf_inj::pulse& p : s->live) {
        int lo = 0, hi = 0;
        if (p.train)
            train_rows(p, first, n_rows, &lo, &hi);
        if (p.train ? lo < hi : burst_overlaps(p, first, n_rows)) (p.train ? trains : bursts).push_back(&p);
    }
    if (!bursts.empty() || !trains.empty()) {
        ON_DEVICE(s->h);
        for (size_t at = 0; at < bursts.size(); at += dsabf::kInjBatch) {
            dsabf::InjBurstArgs a{};
            a.n = (int)std::min<size_t>(dsabf::kInjBatch, bursts.size() - at);
            a.n_freq = s->n_freq;
            a.n_beams = s->n_beams;
            for (int k = 0; k < a.n; k++) {
                const bf_inj::pulse& p = *bursts[at + k];
                a.b[k] = {s->d_profile(p), s->d_response(p), s->d_delay(p), (int64_t)((__int128)p.t0 - (__int128)first), p.width};
            }
            // the kernel's [lo, hi) of every channel, restated: the grid covers the longest
            int64_t span = 0;
            for (int f = 0; f < s->n_freq; f++) {
                int64_t lo = INT64_MAX, hi = INT64_MIN;
                for (int k = 0; k < a.n; k++) {
                    const int64_t start = a.b[k].rel + bursts[at + k]->delay[(size_t)f];
                    lo = std::min(lo, start);
                    hi = std::max(hi, start + a.b[k].W);
                }
                span = std::max(span, std::min<int64_t>(hi, n_rows) - std::max<int64_t>(lo, 0));
            }
            HIP_TRY(dsabf::launch_inj_bursts(d_rows, n_rows, a, (int)span, q));
            s->launches++;
        }
        if (!trains.empty()) {
            dsabf::InjTrainArgs a{};
            a.n = (int)trains.size();
            a.n_freq = s->n_freq;
            a.n_beams = s->n_beams;
            a.row_lo = n_rows;
            a.row_hi = 0;
            for (int k = 0; k < a.n; k++) {
                const bf_inj::pulse& p = *trains[(size_t)k];
                dsabf::InjTrain& t = a.t[k];
                t = {s->d_profile(p), s->d_response(p), s->d_delay(p), p.model.phase0, p.model.dphase, p.model.ddphase,
                     (int64_t)((__int128)first - (__int128)p.model.epoch_row), 0, 0, p.width};
                train_rows(p, first, n_rows, &t.lo, &t.hi);
                a.row_lo = std::min(a.row_lo, t.lo);
                a.row_hi = std::max(a.row_hi, t.hi);
            }
            HIP_TRY(dsabf::launch_inj_trains(d_rows, a, q));
            s->launches++;
        }
        // the event behind this apply: what an add asks before it takes a spent pulse's tables again
        hipEvent_t ev = nullptr;
        if (!s->spare_events.empty()) {
            ev = s->spare_events.back();
            s->spare_events.pop_back();
        } else {
            s->res.event(&ev);
            if (s->res.err != hipSuccess) {   // (no event to be had: not this apply's failure)
                s->res.err = hipSuccess;
                ev = nullptr;
            }
        }
        s->seq++;
        if (ev) {
            HIP_TRY(hipEventRecord(ev, q));
            s->in_flight.push_back({ev, s->seq});
        } else {
            HIP_TRY(hipStreamSynchronize(q));   // without an event the apply ends here, on the host
            if (s->in_flight.empty()) s->completed = s->seq;
        }
    }
    s->next_row = first + (uint64_t)n_rows;
    // spent pulses give their slot back, and their tables -- behind the applies issued so far
    for (size_t i = 0; i < s->live.size();) {
        const bf_inj::pulse& p = s->live[i];
        const bool spent = p.train ? p.end_row <= s->next_row : (__int128)s->next_row >= (__int128)p.t0 + p.delay_max + p.width;
        if (!spent) {
            i++;
            continue;
        }
        s->idle.push_back({p.d_tables, p.bytes, s->seq});
        s->n_trains -= p.train;
        s->live.erase(s->live.begin() + (long)i);
    }
    return BF_OK;
}

extern "C" {

int bf_inj_create(bf_handle* h, int n_freq_total, int max_rows_per_push, int max_pulses, int max_width, bf_inj** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_freq_total < 1 || n_freq_total > 65535) return fail(BF_ERR_INVALID, "bf_inj_create: n_freq_total must be 1 .. 65535, not %d", n_freq_total);
    if (max_rows_per_push < 1 || max_rows_per_push > dsabf::kInjMaxRows)
        return fail(BF_ERR_INVALID, "bf_inj_create: max_rows_per_push must be 1 .. %d, not %d", dsabf::kInjMaxRows, max_rows_per_push);
    if (max_pulses < 1 || max_pulses > dsabf::kInjMaxPulses)
        return fail(BF_ERR_INVALID, "bf_inj_create: max_pulses must be 1 .. %d, not %d", dsabf::kInjMaxPulses, max_pulses);
    if (max_width < 1 || max_width > dsabf::kInjMaxWidth)
        return fail(BF_ERR_INVALID, "bf_inj_create: max_width must be 1 .. %d, not %d", dsabf::kInjMaxWidth, max_width);
    if (!h) return fail(BF_ERR_INVALID, "bf_inj_create: the handle is NULL");
    if (h->cfg.n_beams % 4) return fail(BF_ERR_INVALID, "bf_inj_create: n_beams (%d) must be a multiple of 4", h->cfg.n_beams);
    ON_DEVICE(h);
    bf_inj* s = new (std::nothrow) bf_inj();
    if (!s) return fail(BF_ERR_DEVICE, "out of host memory");
    s->h = h;
    s->n_freq = n_freq_total;
    s->n_beams = h->cfg.n_beams;
    s->max_rows = max_rows_per_push;
    s->max_pulses = max_pulses;
    s->max_width = max_width;
    s->res.queue(&s->copy_q);
    for (int i = 0; i < 4; i++) {   // events for the applies in flight (a DM stage keeps three pushes): an apply makes one only beyond these
        hipEvent_t ev = nullptr;
        s->res.event(&ev);
        if (ev) s->spare_events.push_back(ev);
    }
    if (int rc = stage_adopt(s, "bf_inj_create")) return rc;
    *out = s;
    return BF_OK;
}

int bf_inj_destroy(bf_inj* s) { return stage_destroy(s); }

int bf_inj_add_burst(bf_inj* s, int64_t t0, int W, const int32_t* delay, const float* profile, const float* response, uint64_t* id)
{
    if (!s) return fail(BF_ERR_INVALID, "bf_inj_add_burst: the stage is NULL");
    if (t0 < 0) return fail(BF_ERR_INVALID, "bf_inj_add_burst: t0 must be >= 0");
    if (W < 1 || W > s->max_width) return fail(BF_ERR_INVALID, "bf_inj_add_burst: W must be 1 .. %d (max_width), not %d", s->max_width, W);
    if (int rc = inj_check_tables(s, "bf_inj_add_burst", delay, profile, response)) return rc;
    if (int rc = orphaned(s)) return rc;
    if ((uint64_t)t0 + (uint64_t)*std::min_element(delay, delay + s->n_freq) < s->next_row)
        return fail(BF_ERR_STATE, "bf_inj_add_burst: the burst's first row %llu lies before the %llu rows already applied",
                    (unsigned long long)((uint64_t)t0 + (uint64_t)*std::min_element(delay, delay + s->n_freq)), (unsigned long long)s->next_row);
    if ((int)s->live.size() >= s->max_pulses) return fail(BF_ERR_STATE, "bf_inj_add_burst: %d pulses are alive (max_pulses)", s->max_pulses);
    bf_inj::pulse p;
    p.t0 = t0;
    p.width = W;
    return inj_store(s, p, delay, profile, response, id);
}

int bf_inj_add_train(bf_inj* s, const bf_psr_model* model, uint64_t first_row, uint64_t n_rows, int n_bins, const int32_t* delay,
                     const float* profile, const float* response, uint64_t* id)
{
    if (!s || !model) return fail(BF_ERR_INVALID, "bf_inj_add_train: NULL argument");
    const int max_bins = std::min(s->max_width, dsabf::kPsrMaxBins);
    if (n_bins < dsabf::kPsrMinBins || n_bins > max_bins)
        return fail(BF_ERR_INVALID, "bf_inj_add_train: n_bins must be %d .. %d (max_width), not %d", dsabf::kPsrMinBins, max_bins, n_bins);
    if (n_rows < 1) return fail(BF_ERR_INVALID, "bf_inj_add_train: n_rows must be >= 1 (UINT64_MAX: until the end)");
    if (int rc = inj_check_tables(s, "bf_inj_add_train", delay, profile, response)) return rc;
    if (int rc = orphaned(s)) return rc;
    if (first_row < s->next_row)
        return fail(BF_ERR_STATE, "bf_inj_add_train: first_row %llu lies before the %llu rows already applied", (unsigned long long)first_row,
                    (unsigned long long)s->next_row);
    if ((int)s->live.size() >= s->max_pulses) return fail(BF_ERR_STATE, "bf_inj_add_train: %d pulses are alive (max_pulses)", s->max_pulses);
    if (s->n_trains >= dsabf::kInjMaxTrains) return fail(BF_ERR_STATE, "bf_inj_add_train: %d trains are alive", dsabf::kInjMaxTrains);
    bf_inj::pulse p;
    p.train = true;
    p.width = n_bins;
    p.model = *model;
    p.first_row = first_row;
    p.end_row = n_rows > UINT64_MAX - first_row ? UINT64_MAX : first_row + n_rows;
    return inj_store(s, p, delay, profile, response, id);
}

int bf_inj_apply(bf_inj* s, float* d_rows, int n_rows, void* hip_stream)
{
    if (!s || !d_rows) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (s->feeder) return fail(BF_ERR_STATE, "bf_inj_apply: the injector is attached to a DM stage, whose pushes apply it");
    if (int rc = inj_check_apply(s, n_rows)) return rc;
    return inj_apply(s, d_rows, n_rows, as_stream(hip_stream));
}

uint64_t bf_inj_next_row(const bf_inj* s) { return s ? s->next_row : 0; }
uint64_t bf_inj_launches(const bf_inj* s) { return s ? s->launches : 0; }

int bf_inj_burst_profile(int n_freq_total, int W, double centre, double sigma, const int32_t* smear, const double* fluence, float* profile)
{
    if (!fluence || !profile) return fail(BF_ERR_INVALID, "bf_inj_burst_profile: NULL argument");
    if (n_freq_total < 1 || W < 1) return fail(BF_ERR_INVALID, "bf_inj_burst_profile: need n_freq_total, W >= 1");
    if (!(sigma > 0.0) || !std::isfinite(sigma) || !std::isfinite(centre))
        return fail(BF_ERR_INVALID, "bf_inj_burst_profile: sigma must be > 0, and sigma and centre finite");
    std::vector<double> g((size_t)W);
    const double two_var = 2.0 * sigma * sigma;
    for (int f = 0; f < n_freq_total; f++) {
        const int s = smear ? smear[f] : 1;
        if (s < 1) return fail(BF_ERR_INVALID, "bf_inj_burst_profile: smear must be >= 1 (smear[%d] = %d)", f, s);
        const double half = (double)(s - 1) / 2.0;
        double N = 0.0;
        for (int i = 0; i < W; i++) {
            double sum = 0.0;
            for (int j = 0; j < s; j++) {
                const double d = (((double)i - centre) - (double)j) + half;
                sum = sum + std::exp(-(d * d) / two_var);
            }
            g[(size_t)i] = (1.0 / (double)s) * sum;
            N = N + g[(size_t)i];
        }
        if (!(N > 0.0) || !std::isfinite(N) || !std::isfinite(fluence[f]))
            return fail(BF_ERR_INVALID, "bf_inj_burst_profile: channel %d: the window holds none of the pulse, or a value is not finite", f);
        for (int i = 0; i < W; i++) profile[(size_t)f * (size_t)W + (size_t)i] = (float)(fluence[f] * (g[(size_t)i] / N));
    }
    return BF_OK;
}

int bf_inj_nearest_trial(const int32_t* ladder, int n_dm, int n_freq_total, const int32_t* delay, int* trial)
{
    if (!ladder || !delay || !trial) return fail(BF_ERR_INVALID, "bf_inj_nearest_trial: NULL argument");
    if (n_dm < 1 || n_freq_total < 1) return fail(BF_ERR_INVALID, "bf_inj_nearest_trial: need n_dm, n_freq_total >= 1");
    int64_t best = INT64_MAX;
    for (int d = 0; d < n_dm; d++) {
        int64_t sum = 0;
        for (int f = 0; f < n_freq_total; f++) {
            const int64_t diff = (int64_t)ladder[(size_t)d * (size_t)n_freq_total + (size_t)f] - (int64_t)delay[f];
            sum += diff < 0 ? -diff : diff;
        }
        if (sum < best) {
            best = sum;
            *trial = d;
        }
    }
    return BF_OK;
}

int bf_inj_match(const bf_inj_truth* truth, size_t n, const bf_sps_candidate* cands, size_t m, uint64_t t_tol, int32_t dm_tol, int32_t* best)
{
    if ((n && (!truth || !best)) || (m && !cands)) return fail(BF_ERR_INVALID, "bf_inj_match: NULL argument");
    if (dm_tol < 0) return fail(BF_ERR_INVALID, "bf_inj_match: dm_tol must be >= 0");
    if (m > (size_t)INT32_MAX) return fail(BF_ERR_INVALID, "bf_inj_match: more than 2^31 - 1 candidates");
    for (size_t k = 0; k < n; k++) {
        best[k] = -1;
        const __int128 lo = (__int128)truth[k].t_lo - (__int128)t_tol, hi = (__int128)truth[k].t_hi + (__int128)t_tol;
        for (size_t c = 0; c < m; c++) {
            const bf_sps_candidate& cd = cands[c];
            const int64_t ddm = (int64_t)cd.dm - (int64_t)truth[k].trial;
            const __int128 c_lo = cd.t_start, c_hi = (__int128)cd.t_start + cd.width - 1;
            if (cd.beam != truth[k].beam || ddm > dm_tol || ddm < -(int64_t)dm_tol || c_lo > hi || c_hi < lo) continue;
            if (best[k] < 0 || cd.snr > cands[best[k]].snr) best[k] = (int32_t)c;
        }
    }
    return BF_OK;
}

}  // extern "C"
