// bf_runtime_internal.h -- what the C-ABI runtime's translation units share (bf_runtime.cpp, bf_queues.cpp, bf_dm_stream.cpp,
// bf_sps.cpp, bf_cond.cpp, bf_accum.cpp, bf_corr.cpp, bf_sk.cpp, bf_stokes.cpp, bf_psr.cpp, bf_ffa.cpp, bf_inj.cpp, bf_evt.cpp, bf_vhist.cpp, bf_cdd.cpp, bf_rm.cpp, bf_bench_abi.cpp): the handle, the base of its stages,
// the event chain and the ring of result sets that order the stages' work (bf_chain, bf_result_ring), the snapshot-and-zero accumulator on
// top of both (bf_accumulator) and the accumulator stage under the correlator and the voltage moments, the error string, the device scope.
// Host-only and not installed: no .hip / .hpp file includes it.
#pragma once
#include "../../include/dsabf.h"

#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "bf_kernels.h"

struct bf_event {
    hipEvent_t ev = nullptr;
    bool recorded = false;
};

struct bf_handle {
    bf_config cfg{};
    dsabf::Geometry geom{};
    int device = 0;
    int n_cus = 256;
    bool weights_set = false;
    void* d_wimage = nullptr;     // MFMA fragment image of the weights
    void* d_wimage_p = nullptr;   // conjugate-pair image (geometries with a paired kernel)
    void* d_wimage_f = nullptr;   // antenna-fold image (geometries with a fold kernel)
    int* d_flag = nullptr;        // relayout flags: [0] weight out of range, [1] weights are not conjugate-paired, [2] not antenna-mirror symmetric
    uint8_t* d_data = nullptr;    // ring: n_blocks_on_gpu x bytes_per_block
    float* d_out = nullptr;       // n_streams x floats_per_detect
    float* d_ded = nullptr;       // n_streams x n_beams
    // Scratch of the DM-trial dedispersion, ONE PER STREAM the caller has used (kDmScratchBytes each: which trial groups the
    // wide kernel takes + a 512-byte row of zeros).  The wide kernel writes the flags and the per-thread-window kernel reads
    // them later on the same stream: calls on one stream are ordered by the stream, calls on different streams must not share.
    std::vector<std::pair<hipStream_t, int*>> dm_scratch;
    // The most recent DM launch of this handle -- bf_dedisperse_dm*_device, or a push of a bf_dm_stream that launched -- for
    // bf_get_counter "dm_wide_groups" / "dm_wide_mask" (bf_dm_stream.cpp, dm_wide_taken).  Cleared wherever the scratch can go
    // away: the eviction in dm_scratch(), the release of the stage that owns it, bf_destroy.
    struct dm_launch {
        const int* flags = nullptr;             // the scratch the launch used: its first n_g ints are this launch's verdicts
        int n_g = 0;                            // trial groups of the launch
        hipStream_t stream = nullptr;           // the stream it was issued on
        bool wide = false;                      // the shared-window kernel was launched (false: nothing wrote the flags)
        const struct bf_stage* owner = nullptr; // the DM stage whose scratch it is; NULL: one of dm_scratch above
    } dm_last;
    bool force_general = false;   // bf_set_switch("paired", 0): never select the conjugate-pair kernel (nor the antenna-fold kernel)
    bool no_fold = false;         // bf_set_switch("fold", 0): never select the antenna-fold kernel
    bool dm_ring = true;          // bf_set_switch("dm_ring", 0): the next bf_dm_stream_create takes the linear buffer (test switch)
    bool cal_resident = true;     // bf_set_switch("cal_resident", 0): the gain solver re-reads the visibilities at every antenna count (test switch)
    bool null_resident = true;    // bf_set_switch("null_resident", 0): the same for bf_null_solve_device (test switch)
    // bf_enqueue_gemm_unit coalesces (see flush_units): the caller keeps the reference's one-unit-per-call loop
    // (src/beamformer.cu:454-519), the device sees one launch per run of consecutive gemm-units.
    struct pending_unit {
        int stream_idx, slot, time_slice;
        float* host_out;      // a4: D2H destination of the unit's detected powers (NULL: none)
        float* ded_row;       // a8: D2H destination of its DM-0 row (bf_enqueue_dedisperse after the unit), NULL: none
        bool ded;
    };
    std::vector<pending_unit> pending;
    bool coalesce = true;         // DSABF_COALESCE=0 / bf_set_switch("coalesce", 0): one launch per call, the literal pattern
    uint64_t flush_seq = 0;       // flushes alternate between the first two compute queues
    hipEvent_t flush_done = nullptr;   // end of the previous flush's host copies: the next flush's copies queue behind it
    bool flush_recorded = false;
    uint64_t n_fused_launches = 0;        // fused-kernel launches this handle has issued (bf_get_counter)
    int ib_beam = -1;             // bf_set_incoherent_beam: the beam column every detect launch overwrites with the incoherent beam (-1: none)
    std::vector<const float*> last_out;   // per caller-visible queue: where its most recent gemm-unit's powers are on the device ...
    std::vector<int> last_q;              // ... and the queue that wrote them
    // Per compute queue, device memory allocated at first use (bf_queues.cpp, ensure_buf); sized n_streams at bf_create.
    struct queue_bufs {
        float* out_blk = nullptr;     // n_gemms_per_block x floats_per_detect: bf_enqueue_block
        float* ded_blk = nullptr;     // n_gemms_per_block x n_beams: bf_enqueue_block_dedisperse
        float* full_blk = nullptr;    // the gathered block (world x as large): bf_block_gather_device
        float* stage_blk = nullptr;   // the staged transport's landing area: bf_block_gather_stage_device
        bool blk_ran = false;         // bf_enqueue_block has launched into out_blk
    };
    std::vector<queue_bufs> qbuf;
    int full_world = 0;
    std::vector<struct bf_stage*> stages;   // every stage created on this handle, of whatever kind: bf_destroy releases their device side
    hipStream_t h2d = nullptr;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> join;  // one per compute queue: queue_waits_for
    hipEvent_t t0 = nullptr, t1 = nullptr;
};

// What a stage owns on the device, held by value and shared with nobody.  Every call records what it made and keeps the FIRST
// error; after an error the calls that follow do nothing, so a create is straight-line code that looks at `err` once, at its end.
struct bf_resources {
    hipError_t err = hipSuccess;
    std::vector<void*> device, pinned;
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> queues;
    void* alloc(size_t bytes, bool zeroed, bool on_host);
    template <class T> void dev(T** p, size_t bytes, bool zeroed = false) { *p = static_cast<T*>(alloc(bytes, zeroed, false)); }   // (zeroed: on the null stream)
    template <class T> void host(T** p, size_t bytes) { *p = static_cast<T*>(alloc(bytes, false, true)); }                         // pinned
    void event(hipEvent_t* e);      // timing disabled
    void queue(hipStream_t* q);     // non-blocking
    void device_sync();             // end of a create that zeroed memory: the memsets ran on the null stream, pushes come on non-blocking ones
    // The one rule for in-flight work: every event is waited for, then every queue (wait); then events and queues are destroyed,
    // then the memory is freed.  (An event that was never recorded returns at once.)
    void wait();
    void release();
};

// The base of the twelve stage objects (bf_dm_stream, bf_sps, bf_cond, bf_corr, bf_sk, bf_stokes, bf_psr, bf_ffa, bf_inj, bf_vhist, bf_cdd, bf_rm: opaque to callers, each defined in its own file).
struct bf_stage {
    bf_handle* h = nullptr;                 // NULL: the handle went first and took the device side with it
    const char* const noun;                 // "DM stage", "search stage", ...: the orphan check's message
    struct bf_dm_stream* feeder = nullptr;  // search stage, conditioner, pulsar folder, periodicity stage, injector: the DM stage it is attached to
    bool ring = false;                      // DM stage: its buffer is the twice-mapped ring (bf_get_counter "dm_ring_stages")
    bf_resources res;
    explicit bf_stage(const char* noun_) : noun(noun_) {}
    virtual ~bf_stage() = default;
    virtual void release_device() { res.release(); }   // the handle's device is current; the object stays
    virtual void attached() {}                          // a DM stage has just become the feeder
};

// The event chain: an operation on memory that a stage shares waits for the one before it, whatever queue that came on, and then is
// the new end of the chain.  Two events take turns, so the event being recorded is never the one the queue has just been told to wait
// for.  A push is wait(q), kernel, extend(q); a kernel that must not be held up is kernel, join(q).
struct bf_chain {
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t end = nullptr;          // behind the most recent link (hipEventSynchronize on it: everything so far has run); NULL: the chain is empty
    uint64_t n = 0;                    // links recorded on `ev`
    void create(bf_resources& res) { for (auto& e : ev) res.event(&e); }
    hipError_t wait(hipStream_t q) const { return end ? hipStreamWaitEvent(q, end, 0) : hipSuccess; }   // an empty chain holds nothing up
    hipError_t extend(hipStream_t q)   // what q holds now is the new end
    {
        hipEvent_t e = ev[n++ % 2];
        const hipError_t rc = hipEventRecord(e, q);
        if (rc == hipSuccess) end = e;
        return rc;
    }
    void adopt(hipEvent_t theirs) { end = theirs; }    // an event someone else has recorded (a result set's `copied`, behind a dump) is the new end
    hipError_t join(hipStream_t q)     // behind what q holds now, q waits for the end and then is the end
    {
        const hipError_t rc = wait(q);
        return rc == hipSuccess ? extend(q) : rc;
    }
};

// The ring of result sets: issue j leaves its results in set j % max_in_flight, on the stage's own copy queue, and the sets are
// collected oldest first.  `Set` is the stage's own and derives from bf_result_set; the ring makes the queue and the `copied` events,
// the stage adds its buffers and further events per set.  The refusals ("... are uncollected", "no ... is pending") are the stage's words.
struct bf_result_set {
    hipEvent_t copied = nullptr;       // behind the set's last copy, on copy_q
};
template <class Set> struct bf_result_ring {
    std::vector<Set> sets;
    hipStream_t copy_q = nullptr;
    int max_in_flight = 0;
    uint64_t n_issued = 0, n_collected = 0;
    void create(bf_resources& res, int max_in_flight_)
    {
        max_in_flight = max_in_flight_;
        res.queue(&copy_q);
        sets.resize((size_t)max_in_flight);
        for (auto& r : sets) res.event(&r.copied);
    }
    int pending() const { return (int)(n_issued - n_collected); }
    bool room(uint64_t n = 1) const { return n_issued - n_collected + n <= (uint64_t)max_in_flight; }
    Set& next() { return sets[n_issued % (uint64_t)max_in_flight]; }            // the set the next issue uses
    Set& newest() { return sets[(n_issued - 1) % (uint64_t)max_in_flight]; }    // the set before that one (n_issued > 0)
    void issued() { n_issued++; }
    Set& oldest() { return sets[n_collected % (uint64_t)max_in_flight]; }       // the oldest uncollected set (pending() > 0)
    hipError_t wait_oldest()
    {
        Set& r = oldest();
        return hipEventSynchronize(r.copied);
    }
    void collected() { n_collected++; }   // (the set is free from here on)
};

// The snapshot-and-zero accumulator under bf_accum_stage and the pulsar folder (bf_accum.cpp): bytes on the device that pushes add
// to, the chain that orders the pushes and dumps, and the ring of pinned snapshots.  A push is the stage's own: chain.wait(q), its
// kernel into d_acc, chain.extend(q).  The callers refuse a dump without room and a collect with nothing pending, in their own words.
struct bf_accumulator {
    char* d_acc = nullptr;             // the integration in progress: every push adds to it, a dump copies it out and zeroes it
    size_t bytes = 0;
    bf_chain chain;
    struct snapshot : bf_result_set {
        char* h_acc = nullptr;         // pinned
        uint64_t record[2] = {0, 0};   // the caller's record of the integration
    };
    bf_result_ring<snapshot> ring;
    void create(bf_resources& res, size_t bytes_, int max_in_flight);   // (zeroes d_acc: the create ends with res.device_sync())
    // On copy_q (the dump never holds a caller's queue): behind the end of the chain, the copy out and the memset; the set's `copied` is the new end.
    int dump(uint64_t record0, uint64_t record1 = 0);
    // Waits for the oldest snapshot and frees its set: *h_acc and record[] are good until the next dump.
    int collect(const char** h_acc, uint64_t record[2]);
};

// What differs between the two kinds of accumulator stage, the correlator (bf_corr.cpp) and the voltage moments (bf_sk.cpp).
struct bf_accum_kind {
    const char* noun;                              // bf_stage::noun
    const char* abi;                               // "bf_corr" / "bf_sk": the prefix of the stage's entry points, as its messages name them
    size_t (*entries)(const bf_config* cfg);       // cells of a result; the accumulator holds two int64 per cell
    int (*check_create)(const bf_handle* h);       // what bf_*_create refuses about the geometry
    int (*check_launch)(const bf_handle* h, int n_units, const char* who);   // the bounds of one launch
    int (*launch)(bf_handle* h, const void* d_packed, int n_units, long long* d_acc, bool accumulate, hipStream_t q);
};

// The base of bf_corr and bf_sk (bf_accum.cpp): a bf_accumulator of two int64 per cell, pushed through its kind's launch.
struct bf_accum_stage : bf_stage {
    const bf_accum_kind& kind;
    explicit bf_accum_stage(const bf_accum_kind& k) : bf_stage(k.noun), kind(k) {}
    bf_accumulator acc;                // two int64 per cell of kind.entries
    uint64_t columns = 0;              // columns per polarisation pushed since the last dump
};

// (hidden: shared by the runtime's translation units, not exported from libdsabf.so)
#pragma GCC visibility push(hidden)
namespace dsabf::rt {

extern thread_local std::string g_err;   // bf_last_error(): ONE per thread for the whole library (defined in bf_runtime.cpp)
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int supported_geom(const bf_config* c, dsabf::Geometry& g);   // check_cfg + make_geom + dsabf::fused_supported
inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }
inline int check_weights(const bf_handle* h) { return h->weights_set ? BF_OK : fail(BF_ERR_STATE, "bf_set_weights has not been called"); }
int flush_units(bf_handle* h);                          // bf_queues.cpp
// Every detect launch of a handle: the fused kernel over n_units gemm-units at `in` -> out [unit][o][f][b] and, behind it on the same
// queue, the incoherent beam into column h->ib_beam of the same `out` if one is set (bf_queues.cpp)
int launch_detect(bf_handle* h, const void* in, int n_units, float* out, hipStream_t s);
// The resident gemm-units [first_unit, first_unit + n_units) of ring slot `slot`, for a launch on compute queue stream_idx: refuses a
// queue, a slot or units that are out of range, else *in is where the first of them starts (bf_queues.cpp)
int resident_units(const bf_handle* h, int stream_idx, int slot, int first_unit, int n_units, const uint8_t** in);

int orphaned(const bf_stage* s);                        // BF_ERR_STATE "the handle of this <noun> has been destroyed", or BF_OK
// End of every create: `s` (s->h set) joins its handle's list; a HIP error in s->res destroys it and fails as "<who>: <error>".
int stage_adopt(bf_stage* s, const char* who);
void stage_release(bf_stage* s);                        // device side of a stage; the object stays, detached from its handle
int stage_destroy(bf_stage* s);                         // every bf_*_destroy: unlinked from its feeder and its handle, released, deleted
// The accumulator stages' entry points (bf_accum.cpp); bf_corr_* and bf_sk_* are these.  accum_init takes over `fresh` (NULL: out of
// host memory): the handle adopts it, or it is deleted.
int accum_init(bf_accum_stage* fresh, bf_handle* h, int max_in_flight);
int accum_pending(const bf_accum_stage* s);
int accum_push(bf_accum_stage* s, const void* d_packed, int n_units, void* hip_stream);
int accum_push_block(bf_accum_stage* s, int stream_idx, int slot, int first_unit, int n_units);
int accum_dump(bf_accum_stage* s);
int accum_collect(bf_accum_stage* s, int64_t* out, uint64_t* n_columns_per_pol);
template <class Stage> int accum_create(bf_handle* h, int max_in_flight, Stage** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    Stage* s = new (std::nothrow) Stage();
    if (int rc = accum_init(s, h, max_in_flight)) return rc;
    *out = s;
    return BF_OK;
}
// The link "attached to a DM stage" has two ends: a member of the DM stage (search, cond, folder, periodicity, injector) and the feeder of the stage it points at.
bf_stage* as_stage(struct bf_sps* s);                   // bf_sps.cpp
bf_stage* as_stage(struct bf_cond* c);                  // bf_cond.cpp
bf_stage* as_stage(struct bf_psr* p);                   // bf_psr.cpp
bf_stage* as_stage(struct bf_ffa* s);                   // bf_ffa.cpp
bf_stage* as_stage(struct bf_inj* s);                   // bf_inj.cpp
void dm_stream_drop(struct bf_dm_stream* dm, bf_stage* attached);   // bf_dm_stream.cpp: `attached` is going away
// bf_get_counter "dm_wide_groups" / "dm_wide_mask" (bf_dm_stream.cpp): the trial groups the shared-window kernel took in h->dm_last
int dm_wide_taken(const bf_handle* h, uint64_t* groups, uint64_t* mask);
int sps_check_attach(const struct bf_sps* s, const bf_handle* h, int n_dm, int max_rows);            // bf_dm_stream_attach_search's conditions
int sps_max_in_flight(const struct bf_sps* s);
int cond_check_attach(const struct bf_cond* c, const bf_handle* h, int n_freq_total, int max_rows);  // bf_dm_stream_attach_conditioner's conditions
int psr_check_attach(const struct bf_psr* p, const bf_handle* h, int n_freq_total, int max_rows);    // bf_dm_stream_attach_folder's conditions
int psr_check_push(const struct bf_psr* p, int n_rows);   // what bf_psr_push refuses about a push of n_rows rows, before anything is queued
int ffa_check_attach(const struct bf_ffa* s, const bf_handle* h, int n_dm, int max_rows);            // bf_dm_stream_attach_periodicity's conditions
int ffa_check_push(const struct bf_ffa* s, int n_t);      // what bf_ffa_push refuses about a push of n_t times, before anything is queued
// bf_dm_stream_attach_injector's conditions: the three above, and that the injector has applied exactly the `pushed` rows of the DM stage
int inj_check_attach(const struct bf_inj* s, const bf_handle* h, int n_freq_total, int max_rows, uint64_t pushed);
int inj_check_apply(const struct bf_inj* s, int n_rows);   // what bf_inj_apply refuses about an apply of n_rows rows, before anything is queued
int inj_apply(struct bf_inj* s, float* d_rows, int n_rows, hipStream_t q);   // the apply behind that check: bf_inj_apply, and the DM stage's hook

// Makes `device` current for the duration of one entry point and puts the caller's device back afterwards: a library
// call must not change the current device of a multi-device host process (torch's included).
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
    }
    ~DeviceScope()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

}  // namespace dsabf::rt
#pragma GCC visibility pop
using namespace dsabf::rt;   // (the runtime's files and the macros below name these unqualified)

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(BF_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define ON_DEVICE(h_)                                                                                       \
    DeviceScope dev_scope_((h_)->device);                                                                   \
    if (dev_scope_.err != hipSuccess)                                                                       \
        return fail(BF_ERR_DEVICE, "hipSetDevice(%d) failed: %s", (h_)->device, hipGetErrorString(dev_scope_.err))
#define FLUSH_UNITS(h_) do { if (int rc_ = flush_units(h_)) return rc_; } while (0)
