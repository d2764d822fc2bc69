// bf_dm_stream.cpp -- DM-trial dedispersion (include/dsabf.h): the caller-stream calls and the stage of the observation loop
// (bf_dm_stream_*) with its twice-mapped ring.
#include <mutex>
#include <new>
#include <numeric>

#include "bf_runtime_internal.h"
#include "stamp/bf_stamp_kernels.h"

// ---- DM-trial dedispersion as a stage of the observation loop (include/dsabf.h) ---------------------------
// The detected stream arrives block by block; out[dm][t][b] needs rows t .. t + max_delay.  The stream keeps the last
// max_delay rows of what it has seen in front of the rows of the next push (one device buffer, slid back to its start when its
// end is reached), so every push runs the SAME kernels over [carry | new rows] that bf_dedisperse_dm_device runs over a
// whole series -- and emits exactly the output times that became complete.  Every (trial, time, beam) sum still runs over
// ascending f in one register from +0: the concatenated chunks are bit-identical to one call over the whole series.
struct bf_dm_stream : bf_stage {
    bf_dm_stream() : bf_stage("DM stage") {}
    void release_device() override;
    int n_dm = 0, n_freq = 0, max_delay = 0, max_rows = 0;
    size_t row_floats = 0;
    // The rows live in a RING of cap_rows rows whose physical memory is mapped TWICE, back to back, into one virtual range (HIP's
    // virtual-memory API): row i is also row i + cap_rows, so every window of <= cap_rows consecutive rows -- the carried-over
    // delay window in front of a push's rows -- is contiguous for the kernels wherever it starts, and nothing ever moves.  (Rounds
    // 5's linear buffer slid the carry back to its start every few pushes: at the production block, 31 MiB read and written again
    // every 2.5 blocks.)  ring (bf_stage) == false: that linear buffer -- for a device without VMM support, and bf_set_switch("dm_ring", 0).
    size_t cap_rows = 0;          // ring: rows of physical memory (>= max_delay + 3 max_rows); linear: 2 (max_delay + max_rows)
    size_t wpos = 0;              // ring: physical row the next pushed row goes to (< cap_rows)
    size_t fill = 0;              // linear: rows of d_buf in use, [fill - carry, fill) are the newest rows of the series
    hipMemGenericAllocationHandle_t phys{};
    size_t phys_bytes = 0;
    bool phys_created = false, mapped0 = false, mapped1 = false;
    uint64_t pushed = 0;          // rows the stream has been given
    uint64_t n_push = 0;          // pushes so far
    float* d_buf = nullptr;       // ring: the double mapping (2 x phys_bytes of address space); linear: cap_rows x [freq][beam]
    int32_t* d_delays = nullptr;  // [n_dm][freq]
    // Three pushes may be in flight at once (a caller that alternates queues, as run_observation does: a production block is 64
    // tiles of the shared-window kernel, a quarter of the chip -- the tiles of consecutive blocks run side by side).  Push j works
    // in set j % 3: its chunk [n_dm][max_rows][beam] and the wide kernel's scratch (dsabf::kDmScratchBytes).
    //   rows_ready[j % 3]: the rows of push j -- and of every push before it -- are in the buffer (recorded on push j's queue behind
    //                      its producer and behind rows_ready of push j - 1): what push j + 1's kernels wait for, not push j's END;
    //   done[j % 3]:       push j and every push before it are complete, host copy included (recorded behind done of push j - 1).
    // Push j waits for done of push j - 3 (its set's previous user); so does the producer of push j's rows, which overwrites what
    // only pushes <= j - 3 can still be reading (cap_rows >= max_delay + 3 max_rows).  The linear buffer keeps one push at a time.
    float* d_out[3] = {nullptr, nullptr, nullptr};
    int* d_flags[3] = {nullptr, nullptr, nullptr};
    bool flags_zeroed[3] = {false, false, false};
    hipEvent_t done[3] = {nullptr, nullptr, nullptr}, rows_ready[3] = {nullptr, nullptr, nullptr};
    bool done_recorded[3] = {false, false, false}, rows_recorded[3] = {false, false, false};
    float* reserved = nullptr;    // bf_dm_stream_reserve: where the NEXT push's rows are being written by their producer ...
    int reserved_rows = 0;        // ... and how many (0: no reservation outstanding)
    bf_sps* search = nullptr;     // bf_dm_stream_attach_search: every chunk is also pushed into this stage, before `done` is recorded
    bf_cond* cond = nullptr;      // bf_dm_stream_attach_conditioner: every push's new rows are conditioned in place, before `rows_ready` is recorded
    bf_psr* fold = nullptr;       // bf_dm_stream_attach_folder: every push's new rows are also folded where they lie, before `done` is recorded
    bf_ffa* ffa = nullptr;        // bf_dm_stream_attach_periodicity: every chunk is also pushed into this stage, before `done` is recorded
    bf_inj* inj = nullptr;        // bf_dm_stream_attach_injector: every push's new rows get the live pulses added in place, in front of the conditioner
    // bf_dm_stream_cut (docs/EVENTS.md section 2): the end of the most recent cut, recorded behind the cut before it.  The producer of
    // the rows of a later push waits for it wherever it waits for done[old]: it cannot overwrite what a cut queued before it reads.
    hipEvent_t cut_done = nullptr;
    bool cut_recorded = false;    // false: no cut has ever been issued, and nothing waits for the event
    hipStream_t cut_q = nullptr;  // bf_dm_stream_cut_host: a queue of the stage's own, made at the first call ...
    float* d_cut = nullptr;       // ... and the device buffer its stamps land in, grown as needed
    size_t cut_floats = 0;
    std::vector<int32_t> trial_delay;   // [n_dm]: max over f of delay[dm][f] -- the rows a stamp of that trial needs beyond its times
};

// One link to an attached stage: the member of the DM stage (search, cond, fold, ffa, inj) and that stage's feeder, set and cleared together.
template <class T>
static void set_link(bf_dm_stream* dm, T*& member, T* to)
{
    if (member) as_stage(member)->feeder = nullptr;
    member = to;
    if (!to) return;
    as_stage(to)->feeder = dm;
    as_stage(to)->attached();
}

void dsabf::rt::dm_stream_drop(bf_dm_stream* dm, bf_stage* attached)
{
    if (dm->search && as_stage(dm->search) == attached) set_link<bf_sps>(dm, dm->search, nullptr);
    if (dm->cond && as_stage(dm->cond) == attached) set_link<bf_cond>(dm, dm->cond, nullptr);
    if (dm->fold && as_stage(dm->fold) == attached) set_link<bf_psr>(dm, dm->fold, nullptr);
    if (dm->ffa && as_stage(dm->ffa) == attached) set_link<bf_ffa>(dm, dm->ffa, nullptr);
    if (dm->inj && as_stage(dm->inj) == attached) set_link<bf_inj>(dm, dm->inj, nullptr);
}

// The ring is no hipMalloc: it is unmapped and released here, behind the wait for everything in flight, and the stage's resource
// list (events, chunks, scratch, delays, the linear buffer) goes after it.
void bf_dm_stream::release_device()
{
    set_link<bf_sps>(this, search, nullptr);
    set_link<bf_cond>(this, cond, nullptr);
    set_link<bf_psr>(this, fold, nullptr);
    set_link<bf_ffa>(this, ffa, nullptr);
    set_link<bf_inj>(this, inj, nullptr);
    res.wait();
    if (h && h->dm_last.owner == this) h->dm_last = {};   // (the scratch of the handle's most recent DM launch goes with res)
    if (mapped0) (void)hipMemUnmap(d_buf, phys_bytes);
    if (mapped1) (void)hipMemUnmap(reinterpret_cast<char*>(d_buf) + phys_bytes, phys_bytes);
    if (phys_created) (void)hipMemRelease(phys);   // (the addresses go back to nobody: ring_address_space)
    mapped0 = mapped1 = phys_created = false;
    res.release();
}

// Address space for the rings: taken from arenas that are reserved once per process and NEVER given back or handed out twice.
// On this stack (ROCm 7.2, gfx950) a virtual range that is unmapped and mapped again to other physical memory keeps stale
// translations: kernels and copies then disagree about where the rows are (tools/vmm_probe.cpp modes 0-4: wrong from the second
// ring on, whatever is freed, synchronised or allocated in between; modes 5-6, fresh addresses every time: always right --
// profiles/r06_vmm_probe.txt).  Addresses cost nothing (47 bits of them); a stage takes 2 x its ring's bytes.
static void* ring_address_space(size_t bytes, size_t gran)
{
    static std::mutex mu;
    static char* base = nullptr;
    static size_t size = 0, used = 0;
    std::lock_guard<std::mutex> lock(mu);
    used = (used + gran - 1) / gran * gran;
    if (!base || used + bytes > size) {
        void* va = nullptr;
        for (size_t want : {(size_t)256 << 30, (size_t)32 << 30, (size_t)4 << 30, bytes}) {
            if (want < bytes) continue;
            if (hipMemAddressReserve(&va, want, gran, nullptr, 0) == hipSuccess && va) {
                base = static_cast<char*>(va);
                size = want;
                used = 0;
                break;
            }
            (void)hipGetLastError();
            va = nullptr;
        }
        if (!va) return nullptr;
    }
    void* out = base + used;
    used += bytes;
    return out;
}

// The ring: one physical allocation, mapped at va and at va + phys_bytes.  False (and nothing left behind): no VMM here.
static bool dm_ring_create(bf_dm_stream* s, int device, size_t want_rows)
{
    int vmm = 0;
    if (hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, device) != hipSuccess || !vmm) return false;
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) return false;
    const size_t row_bytes = s->row_floats * sizeof(float);
    const size_t step = gran / std::gcd(row_bytes, gran);   // rows per granule-aligned stretch
    const size_t rows = (want_rows + step - 1) / step * step;
    s->phys_bytes = rows * row_bytes;
    void* va = ring_address_space(2 * s->phys_bytes, gran);
    bool ok = va != nullptr && hipMemCreate(&s->phys, s->phys_bytes, &prop, 0) == hipSuccess;
    s->phys_created = ok;
    s->d_buf = static_cast<float*>(va);
    ok = ok && (s->mapped0 = hipMemMap(va, s->phys_bytes, 0, s->phys, 0) == hipSuccess);
    ok = ok && (s->mapped1 = hipMemMap(static_cast<char*>(va) + s->phys_bytes, s->phys_bytes, 0, s->phys, 0) == hipSuccess);
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    ok = ok && hipMemSetAccess(va, 2 * s->phys_bytes, &acc, 1) == hipSuccess;
    if (!ok) {
        if (s->mapped0) (void)hipMemUnmap(va, s->phys_bytes);
        if (s->mapped1) (void)hipMemUnmap(static_cast<char*>(va) + s->phys_bytes, s->phys_bytes);
        if (s->phys_created) (void)hipMemRelease(s->phys);
        s->mapped0 = s->mapped1 = s->phys_created = false;
        s->d_buf = nullptr;
        (void)hipGetLastError();
        return false;
    }
    s->ring = true;
    s->cap_rows = rows;
    return true;
}

// Scratch of the DM-trial dedispersion for calls on stream `s`: kDwMaxGroups flag ints + one 512-byte row of zeros
// (dsabf::kDmScratchBytes), zeroed ON THAT STREAM when it is first used -- ordered before the kernels that read it, also on a
// non-blocking stream (a memset on the null stream would not be).
static hipError_t dm_scratch(bf_handle* h, hipStream_t s, int** out)
{
    for (auto& sc : h->dm_scratch)
        if (sc.first == s) {
            *out = sc.second;
            return hipSuccess;
        }
    if (h->dm_scratch.size() >= 64) {   // a caller that keeps creating streams: nothing of ours may still be in flight
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
        for (auto& sc : h->dm_scratch) (void)hipFree(sc.second);   // (the handle's bf_dm_streams own their scratch: untouched)
        h->dm_scratch.clear();
        if (!h->dm_last.owner) h->dm_last = {};
    }
    int* p = nullptr;
    hipError_t e = hipMalloc((void**)&p, dsabf::kDmScratchBytes);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(p, 0, dsabf::kDmScratchBytes, s);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return e;
    }
    h->dm_scratch.emplace_back(s, p);
    *out = p;
    return hipSuccess;
}

// Which kernel ran.  The shared-window kernel decides per trial group ON THE DEVICE whether it takes it, and leaves the verdicts in
// the launch's scratch for dedisperse_dm_kernel; both give the same bits, so nothing else shows which of them computed a group.
// This notes, behind a launch_dedisperse_dm that succeeded, what bf_get_counter needs to read the verdicts later.  `wide` restates the gate of
// launch_dedisperse_dm (bf_kernels.hip: the switch, dm_wide_supported, 16-byte alignment of series and output, a series below
// 4 GiB): a launch that fails it never writes the flags, and what the scratch then holds belongs to an earlier launch.
// TWO COPIES OF ONE CONDITION: whoever changes the gate in bf_kernels.hip changes it here.  (The launcher is device code under the
// kernel build id and does not say what it launched; having it return that is the follow-up that removes this copy.  Until then
// tests/test_gpu_dm_paths.py holds the two together gate by gate: the switch in every case, the channel limit in
// test_cap_by_channels[1025], both alignments in test_gates against flags an aligned call left behind; the 4 GiB gate is untested.)
static void dm_note_launch(bf_handle* h, const dsabf::Geometry& g, const float* d_series, int n_t, int n_dm, int n_t_out, const float* d_out,
                           const int* flags, hipStream_t s, const bf_stage* owner)
{
    bf_handle::dm_launch& r = h->dm_last;
    r.flags = flags;
    r.n_g = n_dm > 0 ? (n_dm + dsabf::kDwTrials - 1) / dsabf::kDwTrials : 0;
    r.stream = s;
    r.owner = owner;
    r.wide = n_dm > 0 && n_t_out > 0 && flags && dsabf::dm_wide_supported(g, n_dm) && g.dm_wide && !((uintptr_t)d_series & 15) &&
             !((uintptr_t)d_out & 15) && (size_t)n_t * g.n_freq * g.n_beams * sizeof(float) < ((size_t)1 << 32);
}

// The counters "dm_wide_groups" and "dm_wide_mask": waits for the stream of the handle's most recent DM launch and reads that
// launch's flags.  A launch the wide kernel was no part of reports 0 without touching the device.
int dsabf::rt::dm_wide_taken(const bf_handle* h, uint64_t* groups, uint64_t* mask)
{
    *groups = *mask = 0;
    const bf_handle::dm_launch& r = h->dm_last;
    if (!r.wide || r.n_g <= 0) return BF_OK;
    ON_DEVICE(h);
    std::vector<int> taken((size_t)r.n_g, 0);
    HIP_TRY(hipStreamSynchronize(r.stream));
    HIP_TRY(hipMemcpy(taken.data(), r.flags, taken.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int g = 0; g < r.n_g; g++) {
        if (!taken[(size_t)g]) continue;
        ++*groups;
        if (g < 64) *mask |= (uint64_t)1 << g;
    }
    return BF_OK;
}

extern "C" {

int bf_dedisperse_dm_device(bf_handle* h, const float* d_series, int n_t, const int32_t* d_delays, int n_dm, int n_t_out,
                            float* d_out, void* hip_stream)
{
    if (!h || !d_series || !d_delays || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_t <= 0 || n_dm < 0 || n_t_out < 0 || n_t_out > n_t) return fail(BF_ERR_INVALID, "need 0 <= n_t_out <= n_t, n_dm >= 0");
    return bf_dedisperse_dm_band_device(h, d_series, n_t, h->geom.n_freq, d_delays, n_dm, n_t_out, d_out, hip_stream);
}

int bf_dedisperse_dm_band_device(bf_handle* h, const float* d_series, int n_t, int n_freq_total, const int32_t* d_delays,
                                 int n_dm, int n_t_out, float* d_out, void* hip_stream)
{
    if (!h || !d_series || !d_delays || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_freq_total <= 0 || n_t <= 0 || n_dm < 0 || n_t_out < 0 || n_t_out > n_t)
        return fail(BF_ERR_INVALID, "need n_freq_total > 0, 0 <= n_t_out <= n_t, n_dm >= 0");
    ON_DEVICE(h);
    dsabf::Geometry g = h->geom;
    g.n_freq = n_freq_total;
    int* flags = nullptr;
    HIP_TRY(dm_scratch(h, as_stream(hip_stream), &flags));
    h->dm_last = {};   // (a launch that fails half-way leaves nothing to report)
    HIP_TRY(dsabf::launch_dedisperse_dm(g, d_series, n_t, d_delays, n_dm, n_t_out, d_out, flags, as_stream(hip_stream)));
    dm_note_launch(h, g, d_series, n_t, n_dm, n_t_out, d_out, flags, as_stream(hip_stream), nullptr);
    return BF_OK;
}

int bf_dm_stream_create(bf_handle* h, const int32_t* delays, int n_dm, int n_freq_total, int max_rows_per_push, bf_dm_stream** out)
{
    return bf_dm_stream_create_history(h, delays, n_dm, n_freq_total, max_rows_per_push, 0, out);
}

int bf_dm_stream_create_history(bf_handle* h, const int32_t* delays, int n_dm, int n_freq_total, int max_rows_per_push, int history_rows,
                                bf_dm_stream** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h || !delays) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_dm <= 0 || n_freq_total <= 0 || max_rows_per_push <= 0) return fail(BF_ERR_INVALID, "need n_dm, n_freq_total, max_rows_per_push > 0");
    if (history_rows < 0) return fail(BF_ERR_INVALID, "history_rows must be >= 0");
    int dmax = 0;
    std::vector<int32_t> trial_delay((size_t)n_dm, 0);
    for (size_t i = 0; i < (size_t)n_dm * n_freq_total; i++) {
        if (delays[i] < 0) return fail(BF_ERR_INVALID, "a streamed dedispersion needs delays >= 0 (delay[%zu] = %d)", i, delays[i]);
        if (delays[i] > dmax) dmax = delays[i];
        if (delays[i] > trial_delay[i / (size_t)n_freq_total]) trial_delay[i / (size_t)n_freq_total] = delays[i];
    }
    ON_DEVICE(h);
    bf_dm_stream* s = new (std::nothrow) bf_dm_stream();
    if (!s) return fail(BF_ERR_DEVICE, "out of host memory");
    s->h = h;
    s->n_dm = n_dm;
    s->n_freq = n_freq_total;
    s->max_delay = dmax;
    s->max_rows = max_rows_per_push;
    s->row_floats = (size_t)n_freq_total * h->cfg.n_beams;
    s->trial_delay.swap(trial_delay);
    bf_resources& res = s->res;
    // the ring: the window of a push (<= max_delay + max_rows rows) + two more pushes' rows that may be written while it is read
    // (+ the rows kept for bf_dm_stream_cut: the linear buffer keeps none)
    if (!h->dm_ring || !dm_ring_create(s, h->device, (size_t)dmax + 3 * (size_t)max_rows_per_push + (size_t)history_rows)) {
        // linear: room for the carry and a push twice over -- when the end is reached the carry moves to the start without overlapping itself
        s->cap_rows = 2 * ((size_t)dmax + (size_t)max_rows_per_push);
        res.dev(&s->d_buf, s->cap_rows * s->row_floats * sizeof(float));
    }
    const int n_sets = s->ring ? 3 : 1;   // (the linear buffer keeps one push at a time: one chunk, one scratch)
    for (int k = 0; k < n_sets; k++) {
        res.dev(&s->d_out[k], (size_t)n_dm * max_rows_per_push * h->cfg.n_beams * sizeof(float));
        res.dev(&s->d_flags[k], dsabf::kDmScratchBytes);
    }
    res.dev(&s->d_delays, (size_t)n_dm * n_freq_total * sizeof(int32_t));
    if (res.err == hipSuccess) res.err = hipMemcpy(s->d_delays, delays, (size_t)n_dm * n_freq_total * sizeof(int32_t), hipMemcpyHostToDevice);
    for (int k = 0; k < 3; k++) {
        res.event(&s->done[k]);
        res.event(&s->rows_ready[k]);
    }
    res.event(&s->cut_done);
    if (int rc = stage_adopt(s, "bf_dm_stream_create")) return rc;
    *out = s;
    return BF_OK;
}

// (a stage whose handle went first lost its links then; one that still has its handle loses them in release_device)
int bf_dm_stream_destroy(bf_dm_stream* s) { return stage_destroy(s); }

int bf_dm_stream_max_delay(const bf_dm_stream* s) { return s ? s->max_delay : BF_ERR_INVALID; }

int bf_dm_stream_attach_search(bf_dm_stream* dm, bf_sps* sps)
{
    if (!dm) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(dm)) return rc;
    if (sps == dm->search) return BF_OK;
    if (sps)
        if (int rc = sps_check_attach(sps, dm->h, dm->n_dm, dm->max_rows)) return rc;
    set_link(dm, dm->search, sps);
    return BF_OK;
}

int bf_dm_stream_attach_conditioner(bf_dm_stream* dm, bf_cond* c)
{
    if (!dm) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(dm)) return rc;
    if (c == dm->cond) return BF_OK;
    if (c)
        if (int rc = cond_check_attach(c, dm->h, dm->n_freq, dm->max_rows)) return rc;
    set_link(dm, dm->cond, c);
    return BF_OK;
}

int bf_dm_stream_attach_folder(bf_dm_stream* dm, bf_psr* p)
{
    if (!dm) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(dm)) return rc;
    if (p == dm->fold) return BF_OK;
    if (p)
        if (int rc = psr_check_attach(p, dm->h, dm->n_freq, dm->max_rows)) return rc;
    set_link(dm, dm->fold, p);
    return BF_OK;
}

int bf_dm_stream_attach_periodicity(bf_dm_stream* dm, bf_ffa* f)
{
    if (!dm) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(dm)) return rc;
    if (f == dm->ffa) return BF_OK;
    if (f)
        if (int rc = ffa_check_attach(f, dm->h, dm->n_dm, dm->max_rows)) return rc;
    set_link(dm, dm->ffa, f);
    return BF_OK;
}

int bf_dm_stream_attach_injector(bf_dm_stream* dm, bf_inj* inj)
{
    if (!dm) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(dm)) return rc;
    if (inj == dm->inj) return BF_OK;
    if (inj)
        if (int rc = inj_check_attach(inj, dm->h, dm->n_freq, dm->max_rows, dm->pushed)) return rc;
    set_link(dm, dm->inj, inj);
    return BF_OK;
}

int bf_dm_stream_output_device(bf_dm_stream* s, float** d_out)
{
    if (!s || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    *d_out = s->d_out[s->ring && s->n_push ? (s->n_push - 1) % 3 : 0];   // the most recent push's chunk
    return BF_OK;
}

// Where the next n_rows rows go, with everything the writer of those rows must wait for queued on q first.
//   ring: behind the previous rows, wherever that is -- they overwrite rows that only pushes <= j - 3 can still be reading;
//   linear: behind the previous push, then behind the previous rows -- unless the buffer's end is reached: then the carry slides
//           back to the start first.
static int dm_place_rows(bf_dm_stream* s, int n_rows, hipStream_t q, float** dst)
{
    const size_t D = (size_t)s->max_delay;
    const size_t carry = s->pushed < D ? (size_t)s->pushed : D;
    if (s->ring) {
        const int old = (int)(s->n_push % 3);        // the slot push j will record into: last recorded by push j - 3
        if (s->done_recorded[old]) HIP_TRY(hipStreamWaitEvent(q, s->done[old], 0));
        if (s->cut_recorded) HIP_TRY(hipStreamWaitEvent(q, s->cut_done, 0));   // a cut queued before this producer may read the rows it overwrites
        *dst = s->d_buf + s->wpos * s->row_floats;   // (wpos + n_rows may pass cap_rows: the second mapping continues the first)
        return BF_OK;
    }
    // linear: the writer of the new rows runs behind the previous push, always -- after a slide the new rows walk into the area the
    // pushes before it read (and an earlier, still pending slide copies from), and only the chain of pushes orders those
    // (tools/fuzz_dm_stream.py without synchronisation between pushes found the version that waited only when sliding)
    const int prev = (int)((s->n_push + 2) % 3);
    if (s->n_push && s->done_recorded[prev]) HIP_TRY(hipStreamWaitEvent(q, s->done[prev], 0));
    if (s->fill + (size_t)n_rows > s->cap_rows) {    // slide: fill - carry >= carry here (cap = 2 (D + max_rows))
        if (carry)
            HIP_TRY(hipMemcpyAsync(s->d_buf, s->d_buf + (s->fill - carry) * s->row_floats, carry * s->row_floats * sizeof(float),
                                   hipMemcpyDeviceToDevice, q));
        s->fill = carry;                              // (the carry HAS moved: committed here, not at the push)
    }
    *dst = s->d_buf + s->fill * s->row_floats;
    return BF_OK;
}

// Zero-copy feed (round 6): the place of the next n_rows rows in the stage's own buffer, directly behind the carried-over window.
// The producer -- bf_enqueue_block_to, bf_gather_detected -- writes them there, ordered on (or behind) hip_stream; the push that
// follows finds them in place and only launches.  The reference's collapse sits directly behind detect, no copy in between
// (src/beamformer.cu:492-511); round 5's push copied every row device-to-device first (64 MiB read + 64 MiB written per production
// block).
int bf_dm_stream_reserve(bf_dm_stream* s, int n_rows, float** d_dst, void* hip_stream)
{
    if (!s || !d_dst) return fail(BF_ERR_INVALID, "NULL argument");
    *d_dst = nullptr;
    if (n_rows <= 0 || n_rows > s->max_rows) return fail(BF_ERR_INVALID, "n_rows must be 1 .. %d (max_rows_per_push)", s->max_rows);
    if (int rc = orphaned(s)) return rc;
    if (s->reserved_rows) return fail(BF_ERR_STATE, "bf_dm_stream_reserve: the previous reservation has not been pushed");
    bf_handle* h = s->h;
    ON_DEVICE(h);
    float* dst = nullptr;
    if (int rc = dm_place_rows(s, n_rows, as_stream(hip_stream), &dst)) return rc;
    s->reserved = dst;
    s->reserved_rows = n_rows;
    *d_dst = dst;
    return BF_OK;
}

int bf_dm_stream_push(bf_dm_stream* s, const float* d_rows, int n_rows, float* host_out, uint64_t* first_t, int* n_t_out,
                      void* hip_stream)
{
    if (!s || !d_rows) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_rows <= 0 || n_rows > s->max_rows) return fail(BF_ERR_INVALID, "n_rows must be 1 .. %d (max_rows_per_push)", s->max_rows);
    if (int rc = orphaned(s)) return rc;
    const bool in_place = s->reserved_rows != 0;
    if (in_place && (d_rows != s->reserved || n_rows != s->reserved_rows))
        return fail(BF_ERR_STATE, "bf_dm_stream_push: %d rows are reserved at %p (bf_dm_stream_reserve); push exactly those", s->reserved_rows,
                    (void*)s->reserved);
    // a push that will emit a chunk hands it to the attached search stage: refused HERE, before anything is queued, if that has no room
    if (s->search && s->pushed + (uint64_t)n_rows > (uint64_t)s->max_delay && bf_sps_pending(s->search) >= sps_max_in_flight(s->search))
        return fail(BF_ERR_STATE, "bf_dm_stream_push: the attached search stage has %d uncollected pushes (max_in_flight): bf_sps_collect first",
                    bf_sps_pending(s->search));
    // an attached folder refuses what it would refuse of these rows (its oscillator's range) HERE too
    if (s->fold)
        if (int rc = psr_check_push(s->fold, n_rows)) return rc;
    // an attached periodicity stage takes the chunk this push emits: what it would refuse of it (no free result set for the
    // segments the chunk completes) is refused HERE too
    if (s->ffa) {
        const uint64_t D = (uint64_t)s->max_delay, after = s->pushed + (uint64_t)n_rows;
        const uint64_t emits = (after > D ? after - D : 0) - (s->pushed > D ? s->pushed - D : 0);   // the chunk's times: n_out below
        if (emits)
            if (int rc = ffa_check_push(s->ffa, (int)emits)) return rc;
    }
    // an attached injector refuses what it would refuse of these rows (a train's oscillator range) HERE too
    if (s->inj)
        if (int rc = inj_check_apply(s->inj, n_rows)) return rc;
    bf_handle* h = s->h;
    ON_DEVICE(h);
    hipStream_t q = as_stream(hip_stream);
    const int prev = (int)((s->n_push + 2) % 3), mine = (int)(s->n_push % 3);
    const int set = s->ring ? mine : 0;                                   // chunk + scratch this push works in
    if (s->ring) {
        // this set's previous user is push j - 3 (the producer of in-place rows waited for it too, on the stream it was given)
        if (s->done_recorded[mine]) HIP_TRY(hipStreamWaitEvent(q, s->done[mine], 0));
    } else if (s->n_push && s->done_recorded[prev]) {
        HIP_TRY(hipStreamWaitEvent(q, s->done[prev], 0));                 // linear: behind the previous push, whatever queue that ran on
    }
    if (!s->flags_zeroed[set]) {
        HIP_TRY(hipMemsetAsync(s->d_flags[set], 0, dsabf::kDmScratchBytes, q));
        s->flags_zeroed[set] = true;
    }
    // (the stream's bookkeeping -- wpos / fill, pushed -- is committed at the end: a call that fails on the way leaves it as it found it.
    //  One exception: an attached conditioner.  Once bf_cond_push below has been issued the rows are rewritten and the push is in its
    //  window; if a LATER step of this call fails, do not push the same rows again -- detach, or destroy the stages.)
    const size_t D = (size_t)s->max_delay;
    const size_t carry = s->pushed < D ? (size_t)s->pushed : D;          // the rows in front of the new ones = series rows [pushed - carry, pushed)
    float* new_rows = s->reserved;                                        // where this push's rows lie in the stage's buffer
    if (!in_place) {                                                      // rows that live elsewhere: brought behind the carry first
        if (int rc = dm_place_rows(s, n_rows, q, &new_rows)) return rc;
        HIP_TRY(hipMemcpyAsync(new_rows, d_rows, (size_t)n_rows * s->row_floats * sizeof(float), hipMemcpyDeviceToDevice, q));
    }
    // the kernels read [carry | new rows]: the carry was written by the producers of the pushes before this one, possibly on
    // other queues -- wait until THEIR rows are in place (not for their dedispersion), then say that ours are
    if (s->ring && s->n_push && s->rows_recorded[prev]) HIP_TRY(hipStreamWaitEvent(q, s->rows_ready[prev], 0));
    // The conditioner's hook (docs/CONDITIONING.md section 3): the new rows are rewritten where they lie -- behind the copy-in (the
    // caller's source rows stay raw; host copies that bf_enqueue_block_to queued are in front of this push on q and carry raw rows
    // too), behind rows_ready of the push before this one, and BEFORE rows_ready of this push is recorded.  That one placement is
    // the whole ordering argument for the three pushes in flight: push j + 1's kernels read push j's rows as carry only behind that
    // event, so they see them conditioned; and conditioner j + 1 runs behind conditioner j (the stage's own event chain, and this
    // wait).  In the ring the rows may run past cap_rows into the second mapping: one contiguous range, taken as such.  The linear
    // buffer has no rows_ready: there the whole push already runs behind the previous one.
    // The injector's hook (docs/INJECTION.md section 2) stands in the same place, one step earlier: the live pulses are added to the
    // new rows where they lie, so the conditioner -- and through rows_ready everything else -- sees them as it would see real ones.
    // The argument above covers it word for word; the injector needs no chain of its own, it carries nothing from push to push.
    // (Like the conditioner it has rewritten the rows once issued: if a LATER step of this call fails, detach or destroy.)
    if (s->inj)
        if (int rc = inj_apply(s->inj, new_rows, n_rows, q)) return rc;
    if (s->cond)
        if (int rc = bf_cond_push(s->cond, new_rows, n_rows, q)) return rc;
    if (s->ring) {
        HIP_TRY(hipEventRecord(s->rows_ready[mine], q));
        s->rows_recorded[mine] = true;
    }
    const uint64_t emitted = s->pushed > D ? s->pushed - D : 0;          // output times [0, emitted) have been produced
    const uint64_t after = s->pushed + (uint64_t)n_rows;
    const uint64_t complete = after > D ? after - D : 0;                   // ... and [0, complete) can be now
    const int n_out = (int)(complete - emitted);
    const size_t n_t = carry + (size_t)n_rows;                            // the series the kernels see: starts at output time `emitted`
    // first row of [carry | new rows]: linear: fill - carry; ring: wpos - carry, through the second mapping when that is negative
    const size_t start = s->ring ? (s->wpos >= carry ? s->wpos - carry : s->wpos + s->cap_rows - carry) : s->fill - carry;
    if (n_out > 0) {
        dsabf::Geometry g = h->geom;
        g.n_freq = s->n_freq;
        h->dm_last = {};
        HIP_TRY(dsabf::launch_dedisperse_dm(g, s->d_buf + start * s->row_floats, (int)n_t, s->d_delays, s->n_dm, n_out, s->d_out[set],
                                            s->d_flags[set], q));
        dm_note_launch(h, g, s->d_buf + start * s->row_floats, (int)n_t, s->n_dm, n_out, s->d_out[set], s->d_flags[set], q, s);
        if (host_out)
            HIP_TRY(hipMemcpyAsync(host_out, s->d_out[set], (size_t)s->n_dm * n_out * h->cfg.n_beams * sizeof(float), hipMemcpyDeviceToHost, q));
        // the search reads the chunk where it lies, on this queue and BEFORE `done` below: only that event keeps push j + 3 out of set j % 3
        if (s->search)
            if (int rc = bf_sps_push(s->search, s->d_out[set], n_out, emitted, q)) return rc;
        // ... and so does the periodicity search (docs/PERIODICITY.md section 3), behind the search stage's kernels on this queue
        if (s->ffa)
            if (int rc = bf_ffa_push(s->ffa, s->d_out[set], n_out, emitted, q)) return rc;
    }
    // The folder's hook (docs/PULSAR_FOLDING.md section 2): the new rows are read where they lie, on this queue -- behind the copy-in and
    // the conditioner, so it folds what the dedispersion reads; behind rows_ready and the chunk, so neither the push after this one
    // nor this push's chunk waits for the fold -- and before `done` below, the event every producer that may overwrite these rows
    // waits for.
    if (s->fold)
        if (int rc = bf_psr_push(s->fold, new_rows, n_rows, q)) return rc;
    // the end of push j implies the end of every push before it (chunks leave in order; a producer that waits for push j - 3 knows
    // that nothing older reads the rows it overwrites)
    if (s->ring && s->n_push && s->done_recorded[prev]) HIP_TRY(hipStreamWaitEvent(q, s->done[prev], 0));
    HIP_TRY(hipEventRecord(s->done[mine], q));
    s->done_recorded[mine] = true;
    if (s->ring)
        s->wpos = (s->wpos + (size_t)n_rows) % s->cap_rows;
    else
        s->fill += (size_t)n_rows;
    s->pushed = after;
    s->n_push++;
    s->reserved = nullptr;
    s->reserved_rows = 0;
    if (first_t) *first_t = emitted;
    if (n_t_out) *n_t_out = n_out;
    return BF_OK;
}

// ---- stamps: dedispersed dynamic spectra of single beams, cut from the ring (docs/EVENTS.md section 2) ------------------------
// Series row t lies in physical row t % cap_rows (wpos == pushed % cap_rows: the ring starts at row 0 and only ever advances).
int bf_dm_stream_history(const bf_dm_stream* s, uint64_t* oldest_row, uint64_t* next_row, uint64_t* cap_rows)
{
    if (!s || !oldest_row || !next_row || !cap_rows) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    *next_row = s->pushed;
    *cap_rows = s->cap_rows;
    // the linear buffer keeps no history: an empty range
    const uint64_t taken = s->pushed + (uint64_t)s->reserved_rows;   // rows written, or being written by an outstanding reservation's producer
    *oldest_row = !s->ring ? s->pushed : taken > s->cap_rows ? taken - s->cap_rows : 0;
    return BF_OK;
}

int bf_dm_stream_cut(bf_dm_stream* s, const bf_stamp_request* reqs, int n_req, int n_tau, int tbin, int fbin, float* d_out, int32_t* status,
                     void* hip_stream)
{
    if (!s) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_req < 0) return fail(BF_ERR_INVALID, "n_req must be >= 0");
    if (n_req > 0 && (!reqs || !d_out || !status)) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (!s->ring) return fail(BF_ERR_STATE, "bf_dm_stream_cut: this DM stage runs on the linear buffer, which keeps no history");
    if (n_tau < 1 || tbin < 1 || fbin < 1 || s->n_freq % fbin != 0)
        return fail(BF_ERR_INVALID, "need n_tau, tbin, fbin >= 1 and fbin (%d) dividing the band's %d channels", fbin, s->n_freq);
    if (s->n_freq / fbin > 65535 * 4) return fail(BF_ERR_INVALID, "more than %d frequency groups", 65535 * 4);
    bf_handle* h = s->h;
    for (int r = 0; r < n_req; r++)
        if (reqs[r].dm < 0 || reqs[r].dm >= s->n_dm || reqs[r].beam < 0 || reqs[r].beam >= h->cfg.n_beams)
            return fail(BF_ERR_INVALID, "request %d: trial %d / beam %d outside [0, %d) / [0, %d)", r, reqs[r].dm, reqs[r].beam, s->n_dm, h->cfg.n_beams);
    // the statuses: pure arithmetic on what the host knows
    uint64_t oldest = 0, next = 0, cap = 0;
    (void)bf_dm_stream_history(s, &oldest, &next, &cap);
    int n_cut = 0;
    for (int r = 0; r < n_req; r++) {
        const uint64_t span = (uint64_t)n_tau * (uint64_t)tbin + (uint64_t)s->trial_delay[(size_t)reqs[r].dm];   // (< 2^62 + 2^31)
        const uint64_t t0 = reqs[r].t0;
        status[r] = t0 < oldest ? 1 : (t0 > next || span > next - t0) ? 2 : 0;
        n_cut += status[r] == 0;
    }
    if (!n_cut) return BF_OK;
    ON_DEVICE(h);
    hipStream_t q = as_stream(hip_stream);
    // The ordering, in three steps.  (1) rows_ready of the newest push: recorded behind its producer, its conditioner and rows_ready of
    // the push before it -- every row < pushed is in place and conditioned.
    const int newest = (int)((s->n_push + 2) % 3);
    if (s->n_push && s->rows_recorded[newest]) HIP_TRY(hipStreamWaitEvent(q, s->rows_ready[newest], 0));
    dsabf::StampBatch batch{};
    hipError_t launch_err = hipSuccess;
    int n_items = 0;
    for (int r = 0; r < n_req; r++) {
        if (status[r] == 0) {
            dsabf::StampItem& it = batch.item[n_items++];
            it.row = reqs[r].t0 % s->cap_rows;   // (the window is <= next - oldest <= cap_rows rows long: it ends inside the second mapping)
            it.dm = reqs[r].dm;
            it.beam = reqs[r].beam;
            it.slot = r;
        }
        if (n_items == dsabf::kStampBatch || (r == n_req - 1 && n_items)) {
            launch_err = dsabf::launch_stamp_cut(s->d_buf, s->row_floats, s->n_freq, h->cfg.n_beams, s->d_delays, batch, n_items, n_tau, tbin, fbin,
                                                 d_out, q);
            if (launch_err != hipSuccess) break;   // (what was launched before it is still recorded below)
            n_items = 0;
        }
    }
    // (2) cut_done, behind the cut before this one: the event then means "this cut and every earlier one have read their rows";
    // (3) dm_place_rows waits for it in front of every later producer.
    if (s->cut_recorded) HIP_TRY(hipStreamWaitEvent(q, s->cut_done, 0));
    HIP_TRY(hipEventRecord(s->cut_done, q));
    s->cut_recorded = true;
    if (launch_err != hipSuccess) return fail(BF_ERR_DEVICE, "bf_dm_stream_cut: the launch failed: %s", hipGetErrorString(launch_err));
    return BF_OK;
}

// The cut for a host consumer (run_observation): on a queue of the stage's own, into the stage's device buffer, copied to host_out
// (pinned for an asynchronous copy) and waited for THERE -- the caller's queues keep running.  host_out: [n_req][n_freq / fbin][n_tau];
// the stamps of requests with a non-zero status are not written.
int bf_dm_stream_cut_host(bf_dm_stream* s, const bf_stamp_request* reqs, int n_req, int n_tau, int tbin, int fbin, float* host_out, int32_t* status)
{
    if (!s) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_req < 0) return fail(BF_ERR_INVALID, "n_req must be >= 0");
    if (n_req > 0 && (!reqs || !host_out || !status)) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(s)) return rc;
    if (!s->ring) return fail(BF_ERR_STATE, "bf_dm_stream_cut_host: this DM stage runs on the linear buffer, which keeps no history");
    if (n_tau < 1 || tbin < 1 || fbin < 1 || s->n_freq % fbin != 0)
        return fail(BF_ERR_INVALID, "need n_tau, tbin, fbin >= 1 and fbin (%d) dividing the band's %d channels", fbin, s->n_freq);
    if (!n_req) return BF_OK;
    bf_handle* h = s->h;
    ON_DEVICE(h);
    const size_t stamp_floats = (size_t)(s->n_freq / fbin) * (size_t)n_tau, need = stamp_floats * (size_t)n_req;
    if (!s->cut_q) {
        s->res.queue(&s->cut_q);
        if (s->res.err != hipSuccess) return fail(BF_ERR_DEVICE, "bf_dm_stream_cut_host: %s", hipGetErrorString(s->res.err));
    }
    if (need > s->cut_floats) {   // (nothing of an earlier call is in flight: every call ends with a wait for its queue)
        float* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, need * sizeof(float)));
        for (void*& d : s->res.device)
            if (d == s->d_cut && d) {
                (void)hipFree(d);
                d = nullptr;
            }
        s->res.device.push_back(p);
        s->d_cut = p;
        s->cut_floats = need;
    }
    if (int rc = bf_dm_stream_cut(s, reqs, n_req, n_tau, tbin, fbin, s->d_cut, status, s->cut_q)) return rc;
    for (int r = 0; r < n_req; r++)
        if (status[r] == 0)
            HIP_TRY(hipMemcpyAsync(host_out + (size_t)r * stamp_floats, s->d_cut + (size_t)r * stamp_floats, stamp_floats * sizeof(float),
                                   hipMemcpyDeviceToHost, s->cut_q));
    HIP_TRY(hipStreamSynchronize(s->cut_q));
    return BF_OK;
}

}  // extern "C"
