// bf_run_observation.cpp -- host mirror, part 3: the production branch of the reference's main loop (src/beamformer.cu:364-534, #ifndef
// DEBUG) on the C-ABI of dsabf.h, run_observation, and the stages that ride on it: one struct per stage, walked by the loop.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>

#include "../../include/dsabf_host.h"
#include "bf_host_internal.h"
#include "bf_loop_internal.h"

namespace dsabf {
namespace {

// A sharded run enters its first collective -- the gather behind block 0 -- only if EVERY shard got through its setup: each rank
// takes part in ONE exchange of "ready" flags before the loop, whichever way its setup went (a rank that bailed out alone would
// leave the others waiting in that gather for ever: ADVICE r05).  The caller's own preparations count too (local_setup_ok).
struct setup_gate {
    bf_comm* comm;
    bool done = false;
    int fail(int rc)   // an early return of the setup: tell the other shards, once
    {
        if (comm && !done) {
            done = true;
            bool all = false;
            (void)comm_all_ok(comm, false, &all);
        }
        return rc;
    }
    int pass(bool local_setup_ok)   // the end of the setup: BF_OK if every shard (and every caller) is ready
    {
        if (!comm)
            return local_setup_ok ? BF_OK : set_error(BF_ERR_STATE, "run_observation: the caller reported a failed setup (local_setup_ok = false)");
        done = true;
        bool all = false;
        const int rc = comm_all_ok(comm, local_setup_ok, &all);
        if (rc != BF_OK || all) return rc;
        return set_error(BF_ERR_STATE, local_setup_ok ? "run_observation: another shard of this run failed its setup; nothing was started"
                                                      : "run_observation: this shard's caller reported a failed setup (local_setup_ok = false)");
    }
};

// who holds the gathered band after every block: one rank, or (BF_GATHER_ROOT_ALL) every rank
bool holds_band(const observation_options& opt) { return !opt.comm || opt.gather_root == BF_GATHER_ROOT_ALL || opt.rank == opt.gather_root; }

// How the loop launches, resolved once from the options and the lab switches (DSABF_LAB=1).
struct launch_plan {
    bool block_launch = true;   // bf_enqueue_block launches, or the reference's per-gemm-unit pattern
    int upl = 0;                // gemm-units per launch of the block path
    int n_queues_used = 0;      // compute queues the block launches rotate over
    bool staged = false;        // transport of the sharded gather
    bool is_root = true;        // this rank holds the (gathered) band
    int dm_first = 0, dm_count = 0;   // this rank's share of the DM ladder
    int n_freq_band = 0;        // channels of the band the DM stage sees
    int dm_rows = 0;            // beam-blocks per launch = rows per push
    bool dm_run = false;        // this rank runs a DM stage
};

struct dm_chunk {
    uint64_t block, first_t;
    int n_t;
    float* host;
};

// What every stage sees of its run: the geometry, the options, the log, the handle with its pinned memory, the plan.
struct run_env {
    const bf_config& cfg;
    const observation_options& opt;
    std::ostream& log;
    run_device dev;
    launch_plan plan;
};

int refuse(const char* why) { return set_error(BF_ERR_INVALID, why); }
const char* const kGatherNeedsBlockLaunches = "run_observation: the sharded gather needs block-granular launches";

// One stage of the run: its C-ABI object, its pending queue, host buffers and counters, and the steps of the loop it takes part in --
// the others stay empty.  The loop walks the stages of a step in that step's own order (walk, below) and stops at the first failure.
struct stage {
    run_env& e;
    const bf_config& cfg = e.cfg;
    const observation_options& opt = e.opt;
    std::ostream& log = e.log;
    const launch_plan& plan = e.plan;
    explicit stage(run_env& env) : e(env) {}
    virtual ~stage() {}
    virtual int check() { return BF_OK; }                          // the options alone: before anything is read or created
    virtual const char* unit_launch_refusal() { return nullptr; }  // the stage is on and needs block-granular launches: the refusal
    virtual int create() { return BF_OK; }
    virtual int after_launch(int q, uint64_t block_index, int gpu_block, int first, int upl) { return BF_OK; }   // on the launch's queue
    virtual int after_dm_push(uint64_t block_index, void* dm_qs) { return BF_OK; }
    virtual int after_block(uint64_t block_index) { return BF_OK; }
    virtual int per_chunk(const dm_chunk& c) { return BF_OK; }     // a DM chunk whose block has been analysed
    virtual int per_deliver(uint64_t blocks_analyzed) { return BF_OK; }
    virtual int finish() { return BF_OK; }                         // the end of the run, after the final sync
    virtual void close_sink() {}
    virtual void report(observation_result* res) {}                // its counters into res (if any), then its closing line
    virtual void destroy() {}
    int fail(int rc) const { return gpu_error(log, rc); }
    int refuse_unit_launches() { return refuse(unit_launch_refusal()); }
};

template <class... P, class... A>
int walk(std::initializer_list<stage*> order, int (stage::*step)(P...), A... args)
{
    for (stage* s : order)
        if (const int rc = (s->*step)(args...)) return rc;
    return BF_OK;
}
template <class... P, class... A>
void walk(std::initializer_list<stage*> order, void (stage::*step)(P...), A... args)
{
    for (stage* s : order) (s->*step)(args...);
}
template <class Sink>
void close(Sink* sink)
{
    if (sink) sink->close();
}

// What a stage issued behind a launch and has not collected yet: the block whose analysis event releases it, and what the sink is told.
struct issued {
    uint64_t block, at;
};

// Drains a stage's queue up to the blocks analysed so far: collect(&at) fetches the next result and counts it (it may correct `at`),
// deliver(at) hands it to the sink, if there is one.  (The collect waits for the result's own copy.)
template <class Collect, class Deliver>
int drain(const stage& s, std::deque<issued>& pending, uint64_t blocks_analyzed, const char* sink_failed_at, Collect collect, Deliver deliver)
{
    while (!pending.empty() && pending.front().block < blocks_analyzed) {
        uint64_t at = pending.front().at;
        pending.pop_front();
        const int rc = collect(&at);
        if (rc != BF_OK) return s.fail(rc);
        if (!deliver(at)) {
            s.log << "ERROR: " << sink_failed_at << " " << at << std::endl;
            return BF_ERR_STATE;
        }
    }
    return BF_OK;
}

struct cut_counts {
    uint64_t cut = 0, dropped = 0, missed = 0, beyond_end = 0;
};

// One round of cuts over everything pending: a call of `cut` per group of requests that `same` puts together (`batch` at most); cut
// ones go to the sink (`deliver`), those whose rows have left the ring are counted as missed, those not pushed yet stay -- at the end
// of the run (`last`) they are counted as beyond it: their window passes the last row the run produced.
template <class Want, class Same, class Cut, class Deliver>
int cut_round(const stage& s, std::deque<Want>& pending, size_t batch, bool last, cut_counts& n, const char* sink_failed_at, Same same, Cut cut,
              Deliver deliver)
{
    std::deque<Want> todo;
    todo.swap(pending);
    while (!todo.empty()) {
        std::vector<Want> group;
        std::deque<Want> rest;
        for (const Want& w : todo)
            if (same(w, todo.front()) && group.size() < batch) group.push_back(w); else rest.push_back(w);
        todo.swap(rest);
        std::vector<decltype(Want::rq)> rq;
        for (const Want& w : group) rq.push_back(w.rq);
        std::vector<int32_t> status(group.size(), -1);
        const int rc = cut(rq, group.front(), status.data());
        if (rc != BF_OK) return s.fail(rc);
        for (size_t i = 0; i < group.size(); i++) {
            const Want& w = group[i];
            if (status[i] == 2) {   // not pushed yet: retried at the next deliver -- or, at the end of the run, never there
                if (last) n.beyond_end++; else pending.push_back(w);
            } else if (status[i] == 1) {
                n.missed++;
            } else {
                n.cut++;
                if (!deliver(w, i)) {
                    s.log << "ERROR: " << sink_failed_at << " " << w.rq.t0 << std::endl;
                    return BF_ERR_STATE;
                }
            }
        }
    }
    return BF_OK;
}

// ---- the DM stage: where the reference's loop has its frequency collapse, src/beamformer.cu:492-511 ----
struct dm_stage : stage {
    using stage::stage;
    bf_dm_stream* stream = nullptr;
    size_t n_buf = 0;           // chunks in flight: the launches of MAX_TOTAL_SEP blocks queued + the one being delivered
    std::vector<float*> host;   // pinned chunk buffers, used round robin
    uint64_t seq = 0, times = 0, chunks = 0;
    int check() override
    {
        if (opt.dm_delays && opt.n_dm <= 0) return refuse("run_observation: dm_delays without n_dm");
        if (opt.dm_sink && !opt.dm_delays) return refuse("run_observation: a dm_sink needs dm_delays");
        return BF_OK;
    }
    int check_sharded() const   // behind every other stage's rules
    {
        if (opt.comm && opt.dm_sink && !holds_band(opt)) return refuse("run_observation: only the gather root may have a dm_sink");
        if (opt.dm_split_trials && (!opt.comm || opt.gather_root != BF_GATHER_ROOT_ALL))
            return refuse("run_observation: dm_split_trials needs a sharded run gathered to every rank (BF_GATHER_ROOT_ALL)");
        return BF_OK;
    }
    const char* unit_launch_refusal() override { return opt.dm_delays ? "run_observation: the DM stage needs block-granular launches" : nullptr; }
    int create() override
    {
        if (!plan.dm_run) return BF_OK;
        n_buf = (size_t)(kMaxTotalSep + 2) * (size_t)(cfg.n_gemms_per_block / plan.upl);
        int history_rows = 0;
        if (opt.evt && opt.stamp_sink) {   // docs/EVENTS.md section 3: span / 2 + t_tol + max_width + (n_buf + 1) dm_rows
            const int max_width = 1 << (opt.sps_widths - 1), tbin_max = opt.stamp_tbin ? opt.stamp_tbin : std::max(1, max_width / 2);
            history_rows = opt.stamp_bins * tbin_max / 2 + opt.evt->t_tol + max_width + (int)(n_buf + 1) * plan.dm_rows;
        }
        int rc = bf_dm_stream_create_history(e.dev.h, opt.dm_delays + (size_t)plan.dm_first * plan.n_freq_band, plan.dm_count, plan.n_freq_band,
                                             plan.dm_rows, history_rows, &stream);
        if (rc != BF_OK) return fail(rc);
        if (history_rows) {
            uint64_t oldest = 0, next = 0, cap = 0;
            bf_dm_stream_history(stream, &oldest, &next, &cap);
            log << "Stamps: DM ring of " << cap << " rows (" << ((cap * (uint64_t)plan.n_freq_band * (uint64_t)cfg.n_beams * 4) >> 20) << " MiB), "
                << history_rows << " of them history" << std::endl;
        }
        for (size_t i = 0; i < n_buf; i++) {
            float* chunk = nullptr;
            if ((rc = e.dev.alloc_pinned((size_t)plan.dm_count * plan.dm_rows * cfg.n_beams, &chunk)) != BF_OK) return rc;
            host.push_back(chunk);
        }
        return BF_OK;
    }
    // this launch's rows are in the stream's buffer already; its kernels run on the launch's own queue, the chunk that becomes complete
    // travels to a pinned buffer
    int push(uint64_t block_index, float* d_rows, void* dm_qs, std::deque<dm_chunk>& pending)
    {
        uint64_t first_t = 0;
        int n_t = 0;
        float* chunk = host[(size_t)(seq++ % host.size())];
        const int rc = bf_dm_stream_push(stream, d_rows, plan.dm_rows, chunk, &first_t, &n_t, dm_qs);
        if (rc == BF_OK && n_t > 0) pending.push_back({block_index, first_t, n_t, chunk});
        return rc;
    }
    int per_chunk(const dm_chunk& c) override
    {
        times += (uint64_t)c.n_t;
        if (!opt.dm_sink) return BF_OK;
        chunks++;
        if (!opt.dm_sink->deliver(c.first_t, c.n_t, plan.dm_count, cfg.n_beams, c.host)) {
            log << "ERROR: DM sink failed at output time " << c.first_t << std::endl;
            return BF_ERR_STATE;
        }
        return BF_OK;
    }
    void close_sink() override { close(opt.dm_sink); }
    void report(observation_result* res) override
    {
        if (res) res->dm_times = times, res->dm_chunks = chunks;
        if (plan.dm_run)
            log << "DM stage: trials " << plan.dm_first << " .. " << plan.dm_first + plan.dm_count - 1 << " of " << opt.n_dm << ", " << times
                << " output times (largest delay " << bf_dm_stream_max_delay(stream) << " samples carried over on the device)" << std::endl;
    }
    void destroy() override { bf_dm_stream_destroy(stream); }
};

// A stage that is created next to the DM stage and attached to it: it works on the rows in the stage's buffer.
struct dm_side_stage : stage {
    dm_stage& dm;
    dm_side_stage(run_env& env, dm_stage& d) : stage(env), dm(d) {}
};

// ---- the injector: in front of the conditioner, on the rows in the stage's buffer (docs/INJECTION.md) ----
struct inj_stage : dm_side_stage {
    using dm_side_stage::dm_side_stage;
    bf_inj* inj = nullptr;
    int check() override
    {
        if (opt.inj && !opt.dm_delays) return refuse("run_observation: pulse injection needs the DM stage (dm_delays)");
        if (!opt.inj) return BF_OK;
        // the tables' sizes: the whole band (every rank that dedisperses injects all of it), the handle's beams
        const size_t band = (size_t)cfg.n_freq * (size_t)(opt.comm ? opt.world : 1), n_beams = (size_t)cfg.n_beams;
        for (const inj_plan::burst& b : opt.inj->bursts)
            if (b.W < 1 || b.delay.size() != band || b.profile.size() != band * (size_t)b.W || b.response.size() != n_beams)
                return refuse("run_observation: an injected burst needs W >= 1, delay [band], profile [band][W] and response [n_beams]");
        for (const inj_plan::train& t : opt.inj->trains)
            if (t.n_bins < 2 || t.delay.size() != band || t.profile.size() != band * (size_t)t.n_bins || t.response.size() != n_beams)
                return refuse("run_observation: an injected train needs n_bins >= 2, delay [band], profile [band][n_bins] and response [n_beams]");
        if (opt.inj->trains.size() > (size_t)BF_INJ_MAX_TRAINS || opt.inj->size() > (size_t)BF_INJ_MAX_PULSES)
            return refuse("run_observation: the injection plan holds more than BF_INJ_MAX_TRAINS trains or BF_INJ_MAX_PULSES pulses");
        return BF_OK;
    }
    int create() override
    {
        if (!plan.dm_run || !opt.inj || !opt.inj->size()) return BF_OK;
        int max_width = 1;
        for (const inj_plan::burst& b : opt.inj->bursts) max_width = std::max(max_width, b.W);
        for (const inj_plan::train& t : opt.inj->trains) max_width = std::max(max_width, t.n_bins);
        int rc = bf_inj_create(e.dev.h, plan.n_freq_band, plan.dm_rows, (int)opt.inj->size(), max_width, &inj);
        // every pulse before the first push: the bursts' ids first, then the trains'
        for (size_t i = 0; rc == BF_OK && i < opt.inj->bursts.size(); i++) {
            const inj_plan::burst& b = opt.inj->bursts[i];
            rc = bf_inj_add_burst(inj, b.t0, b.W, b.delay.data(), b.profile.data(), b.response.data(), nullptr);
        }
        for (size_t i = 0; rc == BF_OK && i < opt.inj->trains.size(); i++) {
            const inj_plan::train& t = opt.inj->trains[i];
            rc = bf_inj_add_train(inj, &t.model, t.first_row, t.n_rows, t.n_bins, t.delay.data(), t.profile.data(), t.response.data(), nullptr);
        }
        if (rc == BF_OK) rc = bf_dm_stream_attach_injector(dm.stream, inj);
        return rc == BF_OK ? BF_OK : fail(rc);
    }
    void report(observation_result* res) override
    {
        if (res) res->inj_pulses = inj ? (uint64_t)opt.inj->size() : 0;
        if (inj)
            log << "Injector: " << opt.inj->bursts.size() << " bursts and " << opt.inj->trains.size()
                << " trains added to the rows in front of the DM stage, " << bf_inj_launches(inj) << " kernels launched" << std::endl;
    }
    void destroy() override { bf_inj_destroy(inj); }
};

// ---- the conditioner: in front of the DM stage, on the rows in its buffer (docs/CONDITIONING.md) ----
struct cond_stage : dm_side_stage {
    using dm_side_stage::dm_side_stage;
    bf_cond* cond = nullptr;
    float* mask_host = nullptr;   // pinned, whole dwords: where the conditioner's mask of the last push is read back at the end
    int check() override
    {
        if (opt.cond_baseline < 0 || opt.cond_baseline > 64) return refuse("run_observation: cond_baseline must be 0 (off) .. 64");
        if (opt.cond_baseline && !opt.dm_delays) return refuse("run_observation: the conditioner needs the DM stage (dm_delays)");
        if (!opt.cond_baseline && (opt.cond_mask || opt.cond_auto_threshold != 0.0))
            return refuse("run_observation: cond_mask / cond_auto_threshold need cond_baseline > 0");
        return BF_OK;
    }
    int create() override
    {
        if (!plan.dm_run || opt.cond_baseline <= 0) return BF_OK;
        bf_cond_options co;
        bf_cond_default_options(&co);
        co.baseline_pushes = opt.cond_baseline;
        co.zero_dm = opt.cond_zero_dm ? 1 : 0;
        co.auto_threshold = opt.cond_auto_threshold;
        int rc = bf_cond_create(e.dev.h, plan.n_freq_band, plan.dm_rows, &co, &cond);
        if (rc == BF_OK && opt.cond_mask) rc = bf_cond_set_mask(cond, opt.cond_mask);
        if (rc == BF_OK) rc = bf_dm_stream_attach_conditioner(dm.stream, cond);
        if (rc != BF_OK) return fail(rc);
        return e.dev.alloc_pinned(((size_t)plan.n_freq_band + 3) / 4, &mask_host);
    }
    // channels the conditioner masked in the last push (-1: no conditioner, or no push)
    int masked_channels()
    {
        const uint8_t* d_mask = nullptr;
        if (!cond || !dm.seq || bf_cond_mask_device(cond, &d_mask) != BF_OK) return -1;
        if (bf_enqueue_d2h(e.dev.h, 0, reinterpret_cast<const float*>(d_mask), mask_host, ((size_t)plan.n_freq_band + 3) / 4) != BF_OK) return -1;
        if (bf_stream_sync(e.dev.h, 0) != BF_OK) return -1;
        int n = 0;
        for (int f = 0; f < plan.n_freq_band; f++) n += reinterpret_cast<const uint8_t*>(mask_host)[f] != 0;
        return n;
    }
    void report(observation_result* res) override
    {
        if (res) res->cond_masked = masked_channels();
        if (!cond) return;
        log << "Conditioner: window of " << opt.cond_baseline << " pushes, zero-DM " << (opt.cond_zero_dm ? "on" : "off") << ", automatic mask ";
        if (opt.cond_auto_threshold > 0.0)
            log << "at " << opt.cond_auto_threshold << " deviations";
        else
            log << "off";
        log << std::endl;
        if (opt.verbose) log << "Conditioner: " << masked_channels() << " of " << plan.n_freq_band << " channels masked in the last push" << std::endl;
    }
    void destroy() override { bf_cond_destroy(cond); }
};

// ---- the pulsar folder: behind the conditioner, on the rows in the stage's buffer (docs/PULSAR_FOLDING.md); a dump per launch at most ----
struct psr_stage : dm_side_stage {
    using dm_side_stage::dm_side_stage;
    bf_psr* psr = nullptr;
    uint64_t rows_folded = 0, dumps = 0;   // rows folded since the last dump; dumps delivered
    std::deque<issued> pending;            // the block behind whose last launch each uncollected dump was issued
    std::vector<double> prof;
    std::vector<uint64_t> hits;
    int check() override
    {
        if (opt.n_psr < 0 || opt.n_psr > BF_PSR_MAX_PULSARS) return refuse("run_observation: n_psr must be 0 (off) .. 4");
        if (opt.n_psr && !opt.dm_delays) return refuse("run_observation: the pulsar folder needs the DM stage (dm_delays)");
        if (opt.n_psr && (!opt.psr_models || !opt.psr_delays)) return refuse("run_observation: n_psr > 0 needs psr_models and psr_delays");
        if (opt.n_psr && (opt.psr_bins < 2 || opt.psr_bins > BF_PSR_MAX_BINS || opt.psr_dump_rows < 1))
            return refuse("run_observation: the pulsar folder needs psr_bins in 2 .. 4096 and psr_dump_rows >= 1");
        if (!opt.n_psr && opt.psr_sink) return refuse("run_observation: a psr_sink needs n_psr > 0");
        return BF_OK;
    }
    int create() override
    {
        if (!plan.dm_run || opt.n_psr <= 0) return BF_OK;
        int rc = bf_psr_create(e.dev.h, plan.n_freq_band, plan.dm_rows, opt.psr_bins, opt.psr_models, opt.psr_delays, opt.n_psr, (int)dm.n_buf, &psr);
        if (rc == BF_OK) rc = bf_dm_stream_attach_folder(dm.stream, psr);
        if (rc != BF_OK) return fail(rc);
        prof.resize(bf_psr_entries(opt.n_psr, plan.n_freq_band, opt.psr_bins, cfg.n_beams));
        hits.resize(prof.size() / (size_t)cfg.n_beams);
        return BF_OK;
    }
    int after_dm_push(uint64_t block_index, void* dm_qs) override   // the attached folder has folded the rows of this push
    {
        if (!psr || (rows_folded += (uint64_t)plan.dm_rows) < (uint64_t)opt.psr_dump_rows) return BF_OK;
        const int rc = bf_psr_dump(psr, dm_qs);
        pending.push_back({block_index, 0});
        rows_folded = 0;
        return rc;
    }
    int per_deliver(uint64_t blocks_analyzed) override
    {
        uint64_t n_rows = 0;
        return drain(*this, pending, blocks_analyzed, "fold sink failed at row",
                     [&](uint64_t* first_row) {
                         const int rc = bf_psr_collect(psr, prof.data(), hits.data(), first_row, &n_rows);
                         if (rc == BF_OK) dumps++;
                         return rc;
                     },
                     [&](uint64_t first_row) {
                         return !opt.psr_sink || opt.psr_sink->deliver(first_row, n_rows, opt.n_psr, plan.n_freq_band, opt.psr_bins, cfg.n_beams,
                                                                           hits.data(), prof.data());
                     });
    }
    void close_sink() override { close(opt.psr_sink); }
    void report(observation_result* res) override
    {
        if (res) res->psr_dumps = dumps;
        if (psr)
            log << "Pulsar folder: " << opt.n_psr << " pulsars, " << opt.psr_bins << " bins, " << dumps << " dumps of at least " << opt.psr_dump_rows
                << " rows each (an incomplete integration at the end is dropped)" << std::endl;
    }
    void destroy() override { bf_psr_destroy(psr); }
};

// ---- the periodicity search (docs/PERIODICITY.md) ----
struct ffa_stage : dm_side_stage {
    using dm_side_stage::dm_side_stage;
    bf_ffa* ffa = nullptr;
    uint64_t times = 0, segments = 0, candidates = 0;   // output times of the delivered chunks; segments collected
    std::vector<bf_ffa_candidate> cands;
    int check() override
    {
        if (opt.ffa_p_hi < 0) return refuse("run_observation: ffa_p_hi must be 0 (off) or the end of the period range");
        if (opt.ffa_p_hi && !opt.dm_delays) return refuse("run_observation: the periodicity search needs the DM stage (dm_delays)");
        if (!opt.ffa_p_hi && opt.ffa_sink) return refuse("run_observation: an ffa_sink needs ffa_p_hi > 0");
        return BF_OK;
    }
    int create() override
    {
        if (!plan.dm_run || opt.ffa_p_hi <= 0) return BF_OK;
        // a result set for every segment the chunks in flight can complete: at most n_buf chunks of dm_rows times are pushed
        // and not yet delivered, and X times behind a segment in progress complete at most X / seg_rows + 1 segments
        const uint64_t seg_rows = (uint64_t)std::max(opt.ffa_seg, 1) * (uint64_t)std::max(opt.ffa_dec, 1);
        const int in_flight = (int)((uint64_t)dm.n_buf * (uint64_t)plan.dm_rows / seg_rows + 1);
        int rc = bf_ffa_create(e.dev.h, plan.dm_count, plan.dm_first, opt.ffa_dec, opt.ffa_seg, opt.ffa_oct, opt.ffa_p_lo, opt.ffa_p_hi, opt.ffa_widths,
                               plan.dm_rows, in_flight, opt.ffa_threshold, &ffa);
        if (rc == BF_OK && (opt.ffa_detrend_blk || opt.ffa_detrend_win)) rc = bf_ffa_set_detrend(ffa, opt.ffa_detrend_blk, opt.ffa_detrend_win);
        if (rc == BF_OK) rc = bf_dm_stream_attach_periodicity(dm.stream, ffa);
        if (rc != BF_OK) return fail(rc);
        cands.resize((size_t)plan.dm_count * cfg.n_beams);
        return BF_OK;
    }
    // the segments this chunk completed: their kernels ran behind the chunk's on its queue; the collect waits for their records
    int per_chunk(const dm_chunk& c) override
    {
        if (!ffa) return BF_OK;
        times += (uint64_t)c.n_t;
        const uint64_t seg_rows = (uint64_t)opt.ffa_seg * (uint64_t)opt.ffa_dec;
        while (segments < times / seg_rows) {
            size_t n = 0;
            const int rc = bf_ffa_collect(ffa, cands.data(), cands.size(), &n);
            if (rc != BF_OK) return fail(rc);
            segments++;
            candidates += n;
            if (opt.ffa_sink && !opt.ffa_sink->deliver(cands.data(), n)) {
                log << "ERROR: periodicity sink failed at segment " << segments - 1 << std::endl;
                return BF_ERR_STATE;
            }
        }
        return BF_OK;
    }
    void close_sink() override { close(opt.ffa_sink); }
    void report(observation_result* res) override
    {
        if (res) res->ffa_segments = segments, res->ffa_candidates = candidates;
        if (ffa)
            log << "Periodicity search: periods " << opt.ffa_p_lo << " .. " << opt.ffa_p_hi - 1 << " samples x " << opt.ffa_oct
                << " octaves at decimation " << opt.ffa_dec << ", " << segments << " segments of " << opt.ffa_seg << " samples, " << candidates
                << " candidates at S/N >= " << opt.ffa_threshold << " (an incomplete segment at the end is dropped)" << std::endl;
    }
    void destroy() override { bf_ffa_destroy(ffa); }
};

// ---- the search stage: as many result sets as chunk buffers (a chunk in flight = a search push in flight) ----
struct sps_stage : dm_side_stage {
    using dm_side_stage::dm_side_stage;
    using candidate = bf_sps_candidate;
    bf_sps* sps = nullptr;
    std::vector<candidate> cands;   // what the collect returned for the last chunk, n_cands of them
    size_t n_cands = 0;
    uint64_t candidates = 0;
    int check() override
    {
        if (opt.sps_widths < 0 || opt.sps_widths > 8) return refuse("run_observation: sps_widths must be 0 (off) .. 8");
        if ((opt.sps_widths || opt.sps_sink) && !opt.dm_delays) return refuse("run_observation: the single-pulse search needs the DM stage (dm_delays)");
        if (opt.sps_sink && !opt.sps_widths) return refuse("run_observation: a sps_sink needs sps_widths > 0");
        return BF_OK;
    }
    int create() override
    {
        if (!plan.dm_run || opt.sps_widths <= 0) return BF_OK;
        int rc = bf_sps_create(e.dev.h, plan.dm_count, plan.dm_first, opt.sps_widths, plan.dm_rows, (int)dm.n_buf, /*baseline_pushes=*/8,
                               /*min_samples=*/64, opt.sps_threshold, &sps);
        if (rc == BF_OK) rc = bf_dm_stream_attach_search(dm.stream, sps);
        if (rc != BF_OK) return fail(rc);
        cands.resize((size_t)plan.dm_count * cfg.n_beams);
        return BF_OK;
    }
    // one search push per chunk, in the same order: its kernels ran on the chunk's queue; the collect waits for its records
    int per_chunk(const dm_chunk& c) override
    {
        if (!sps) return BF_OK;
        const int rc = bf_sps_collect(sps, cands.data(), cands.size(), &n_cands);
        if (rc != BF_OK) return fail(rc);
        candidates += n_cands;
        if (opt.sps_sink && !opt.sps_sink->deliver(cands.data(), n_cands)) {
            log << "ERROR: candidate sink failed at output time " << c.first_t << std::endl;
            return BF_ERR_STATE;
        }
        return BF_OK;
    }
    void close_sink() override { close(opt.sps_sink); }
    void report(observation_result* res) override
    {
        if (res) res->sps_candidates = candidates;
        if (sps)
            log << "Single-pulse search: boxcar widths 1 .. " << (1 << (opt.sps_widths - 1)) << ", " << candidates << " candidates at S/N >= "
                << opt.sps_threshold << std::endl;
    }
    void destroy() override { bf_sps_destroy(sps); }
};

// ---- the event builder (docs/EVENTS.md): the search's candidates of every chunk in, the events that close out ----
struct event_stage : stage {
    using event = bf_evt_event;
    sps_stage& search;
    event_stage(run_env& env, sps_stage& s) : stage(env), search(s) {}
    bf_evt* evt = nullptr;
    bf_evt_options evt_opt{};   // opt.evt with max_width and ib_beam filled in
    std::vector<event> out;     // what the last feed (or the flush) closed, n_out of them
    size_t n_out = 0;
    uint64_t events = 0;
    int check() override
    {
        if (opt.evt && !opt.sps_widths) return refuse("run_observation: the event builder (evt) needs sps_widths > 0");
        if ((opt.event_sink || opt.stamp_sink) && !opt.evt) return refuse("run_observation: an event_sink or a stamp_sink needs evt");
        return BF_OK;
    }
    int create() override
    {
        if (!plan.dm_run || !opt.evt) return BF_OK;
        evt_opt = *opt.evt;
        evt_opt.max_width = 1 << (opt.sps_widths - 1);
        if (evt_opt.ib_beam < 0) evt_opt.ib_beam = opt.incoherent_beam;
        const int rc = bf_evt_create(&evt_opt, &evt);
        return rc == BF_OK ? BF_OK : fail(rc);
    }
    int closed(int rc)   // the events a feed or the flush closed: to the sink
    {
        if (rc != BF_OK) return fail(rc);
        events += n_out;
        if (opt.event_sink && n_out && !opt.event_sink->deliver(out.data(), n_out)) {
            log << "ERROR: event sink failed" << std::endl;
            return BF_ERR_STATE;
        }
        return BF_OK;
    }
    int per_chunk(const dm_chunk& c) override   // the chunk's candidates (global trial indices) into the builder
    {
        if (!evt) return BF_OK;
        out.resize((size_t)bf_evt_open(evt) + search.n_cands);
        return closed(bf_evt_feed(evt, search.cands.data(), search.n_cands, c.first_t + (uint64_t)c.n_t, out.data(), out.size(), &n_out));
    }
    int finish() override   // the end of the run: every open cluster closes
    {
        if (!evt) return BF_OK;
        out.resize((size_t)bf_evt_open(evt));
        return closed(bf_evt_flush(evt, out.data(), out.size(), &n_out));
    }
    // The selection rule of the stamps and the voltage cuts over the events of the last feed: unflagged ones unless `flagged`, by snr
    // descending, then event order, at most `cap`; the rest are counted as dropped.
    std::vector<size_t> select(bool flagged, int cap, uint64_t& dropped) const
    {
        std::vector<size_t> pick;
        for (size_t i = 0; i < n_out; i++)
            if (flagged || !out[i].flags) pick.push_back(i);
        std::stable_sort(pick.begin(), pick.end(), [&](size_t a, size_t b) { return out[a].best.snr > out[b].best.snr; });
        if (pick.size() > (size_t)cap) {
            dropped += pick.size() - (size_t)cap;
            pick.resize((size_t)cap);
        }
        return pick;
    }
    void close_sink() override { close(opt.event_sink); }
    void destroy() override { bf_evt_destroy(evt); }
};

// ---- the stamps (docs/EVENTS.md): cuts of the DM stage's history around the events that are wanted ----
struct stamp_stage : dm_side_stage {
    event_stage& ev;
    stamp_stage(run_env& env, dm_stage& d, event_stage& v) : dm_side_stage(env, d), ev(v) {}
    // A stamp that is wanted: the request (local trial index), and what the sink is told about the event it belongs to.
    struct want {
        bf_stamp_request rq;
        int tbin, width, dm_global;
        double snr;
    };
    std::deque<want> pending;   // wanted, not yet cut: new ones, and those answered "not pushed yet"
    float* host = nullptr;      // pinned: the stamps of one cut
    size_t batch = 0;           // requests one cut takes
    cut_counts n;
    int check() override
    {
        if (opt.evt && (opt.stamp_bins < 1 || opt.stamp_tbin < 0 || opt.stamp_fbin < 1 || opt.stamp_max_per_deliver < 0 ||
                        (cfg.n_freq * (opt.comm ? opt.world : 1)) % opt.stamp_fbin != 0))
            return refuse("run_observation: need stamp_bins >= 1, stamp_tbin >= 0, stamp_max_per_deliver >= 0 and stamp_fbin >= 1 dividing the band");
        return BF_OK;
    }
    int create() override
    {
        if (!ev.evt || !opt.stamp_sink) return BF_OK;
        batch = (size_t)std::max(1, opt.stamp_max_per_deliver);
        return e.dev.alloc_pinned(batch * (size_t)(plan.n_freq_band / opt.stamp_fbin) * (size_t)opt.stamp_bins, &host);
    }
    int want_stamps()   // of the events the last feed closed: stamp_bins bins centred on the best member
    {
        if (!ev.evt || !opt.stamp_sink) return BF_OK;
        for (size_t i : ev.select(opt.stamp_flagged, opt.stamp_max_per_deliver, n.dropped)) {
            const auto& b = ev.out[i].best;
            const int tbin = opt.stamp_tbin ? opt.stamp_tbin : std::max(1, b.width / 2);
            const uint64_t centre = b.t_start + (uint64_t)(b.width / 2), half = (uint64_t)opt.stamp_bins * (uint64_t)tbin / 2;
            pending.push_back({{centre > half ? centre - half : 0, b.dm - plan.dm_first, b.beam}, tbin, b.width, b.dm, b.snr});
        }
        return BF_OK;
    }
    int cut(bool last)   // a call per time binning, on the stage's own queue: the compute queues keep running
    {
        if (!opt.stamp_sink) return BF_OK;
        const int n_freq_out = plan.n_freq_band / opt.stamp_fbin;
        const size_t stamp_floats = (size_t)n_freq_out * (size_t)opt.stamp_bins;
        return cut_round(*this, pending, batch, last, n, "stamp sink failed at time", [](const want& a, const want& b) { return a.tbin == b.tbin; },
                         [&](std::vector<bf_stamp_request>& rq, const want& w, int32_t* status) {
                             return bf_dm_stream_cut_host(dm.stream, rq.data(), (int)rq.size(), opt.stamp_bins, w.tbin, opt.stamp_fbin, host, status);
                         },
                         [&](const want& w, size_t i) {
                             return opt.stamp_sink->deliver(w.rq.t0, w.dm_global, w.rq.beam, w.tbin, w.width, w.snr, host + i * stamp_floats, n_freq_out,
                                                              opt.stamp_bins);
                         });
    }
    int per_chunk(const dm_chunk&) override { return want_stamps(); }
    int per_deliver(uint64_t) override { return cut(/*last=*/false); }
    int finish() override { return want_stamps(), cut(/*last=*/true); }
    void close_sink() override { close(opt.stamp_sink); }
    void report(observation_result* res) override   // (the events' closing line carries the stamps' counters)
    {
        if (res) res->events = ev.events, res->stamps = n.cut, res->stamps_dropped = n.dropped, res->stamps_missed = n.missed, res->stamps_beyond_end = n.beyond_end;
        if (!ev.evt) return;
        log << "Events: " << ev.events << " events";
        if (opt.stamp_sink)
            log << ", stamps " << n.cut << ", stamps_dropped " << n.dropped << ", stamps_missed " << n.missed << ", beyond the end of the run " << n.beyond_end;
        log << std::endl;
    }
};

// ---- the voltage history (docs/VOLTAGE_CUTS.md): a device copy of every launch's units, and dedispersed cuts of it around the events ----
struct vcut_stage : dm_side_stage {
    event_stage& ev;
    vcut_stage(run_env& env, dm_stage& d, event_stage& v) : dm_side_stage(env, d), ev(v) {}
    // A voltage cut that is wanted: the request (samples, local trial index), and what the sink is told about the event it belongs to.
    struct want {
        bf_vcut_request rq;
        int beam, width, dm_global;
        double snr;
    };
    bf_vhist* vhist = nullptr;
    std::deque<want> pending;       // wanted, not yet cut: new ones, and those answered "not pushed yet"
    uint8_t* host = nullptr;        // pinned: the units of one cut
    size_t batch = 0, bytes = 0;    // requests one cut takes; bytes of one request's units
    cut_counts n;
    int check() override
    {
        if (opt.vcut_sink && !opt.evt) return refuse("run_observation: a vcut_sink needs evt");
        if (opt.vcut_sink && opt.comm) return refuse("run_observation: voltage cuts are not available on a sharded run");
        if (opt.vcut_sink && (opt.vcut_units < 1 || opt.vcut_history_units < 0 || opt.vcut_max_per_deliver < 0))
            return refuse("run_observation: need vcut_units >= 1, vcut_history_units >= 0 and vcut_max_per_deliver >= 0");
        return BF_OK;
    }
    // The delay table is the DM stage's row delays of this rank's trials in samples -- the ladder of the detected stream, nothing finer
    // -- and the ring what bf_vhist_units_needed says, unless the caller sizes it.
    int create() override
    {
        if (!ev.evt || !opt.vcut_sink) return BF_OK;
        const size_t n_del = (size_t)plan.dm_count * (size_t)cfg.n_freq;
        std::vector<int32_t> delays(n_del);
        const int32_t* rows = opt.dm_delays + (size_t)plan.dm_first * plan.n_freq_band;
        for (size_t i = 0; i < n_del; i++) delays[i] = rows[i] * cfg.n_avg;
        const int max_width = 1 << (opt.sps_widths - 1);
        const int units = opt.vcut_history_units ? opt.vcut_history_units
                                                 : bf_vhist_units_needed(&cfg, bf_dm_stream_max_delay(dm.stream), plan.dm_rows, (int)dm.n_buf,
                                                                         opt.evt->t_tol, max_width, opt.vcut_units);
        int rc = bf_vhist_create(e.dev.h, delays.data(), plan.dm_count, units, &vhist);
        if (rc != BF_OK) return fail(rc);
        uint64_t oldest = 0, next = 0, cap = 0;
        bf_vhist_history(vhist, &oldest, &next, &cap);
        bytes = (size_t)opt.vcut_units * (size_t)bf_bytes_per_gemm(&cfg);
        log << "Voltage cuts: history of " << cap << " gemm-units (" << ((cap * (uint64_t)bf_bytes_per_gemm(&cfg)) >> 20) << " MiB), cuts of "
            << opt.vcut_units << " units" << std::endl;
        batch = (size_t)std::max(1, opt.vcut_max_per_deliver);
        float* p = nullptr;
        if ((rc = e.dev.alloc_pinned((batch * bytes + 3) / 4, &p)) != BF_OK) return rc;
        host = reinterpret_cast<uint8_t*>(p);
        return BF_OK;
    }
    int after_launch(int q, uint64_t, int gpu_block, int first, int upl) override { return vhist ? bf_vhist_push_block(vhist, q, gpu_block, first, upl) : BF_OK; }
    int want_cuts()   // of the events the last feed closed: vcut_units units centred on the best member
    {
        if (!ev.evt || !opt.vcut_sink) return BF_OK;
        const uint64_t S = (uint64_t)cfg.n_out_per_gemm * (uint64_t)cfg.n_avg;
        for (size_t i : ev.select(opt.vcut_flagged, opt.vcut_max_per_deliver, n.dropped)) {
            const auto& b = ev.out[i].best;
            const uint64_t centre = (b.t_start + (uint64_t)(b.width / 2)) * (uint64_t)cfg.n_avg, half = (uint64_t)opt.vcut_units * S / 2;
            pending.push_back({{centre > half ? centre - half : 0, b.dm - plan.dm_first, 0}, b.beam, b.width, b.dm, b.snr});
        }
        return BF_OK;
    }
    int cut(bool last)   // vcut_batch requests at most per call, on the history's own queue
    {
        if (!opt.vcut_sink) return BF_OK;
        return cut_round(*this, pending, batch, last, n, "voltage sink failed at sample", [](const want&, const want&) { return true; },
                         [&](std::vector<bf_vcut_request>& rq, const want&, int32_t* status) {
                             return bf_vhist_cut_host(vhist, rq.data(), (int)rq.size(), opt.vcut_units, host, status);
                         },
                         [&](const want& w, size_t i) {
                             return opt.vcut_sink->deliver(w.rq.t0, w.dm_global, w.beam, w.width, w.snr, host + i * bytes, bytes);
                         });
    }
    int per_chunk(const dm_chunk&) override { return want_cuts(); }
    int per_deliver(uint64_t) override { return cut(/*last=*/false); }
    int finish() override { return want_cuts(), cut(/*last=*/true); }
    void close_sink() override { close(opt.vcut_sink); }
    void report(observation_result* res) override
    {
        if (res) res->vcuts = n.cut, res->vcuts_dropped = n.dropped, res->vcuts_missed = n.missed, res->vcuts_beyond_end = n.beyond_end;
        if (vhist)
            log << "Voltage cuts: " << n.cut << " cuts of " << opt.vcut_units << " gemm-units, vcuts_dropped " << n.dropped << ", vcuts_missed " << n.missed
                << ", beyond the end of the run " << n.beyond_end << std::endl;
    }
    void destroy() override { bf_vhist_destroy(vhist); }
};

// ---- the incoherent beam (docs/INCOHERENT_BEAM.md): a setting of the handle, made with the weights ----
struct ib_stage : stage {
    using stage::stage;
    int check() override
    {
        if (opt.incoherent_beam < -1 || opt.incoherent_beam >= cfg.n_beams)
            return refuse("run_observation: incoherent_beam must be -1 (off) or a beam index");
        return BF_OK;
    }
    void report(observation_result*) override
    {
        if (opt.incoherent_beam >= 0) log << "Incoherent beam: in beam column " << opt.incoherent_beam << " of the detected stream" << std::endl;
    }
};

// A tap on the resident voltage blocks that integrates over whole blocks -- the correlator, the voltage moments: a push per launch on
// the launch's queue, a dump after every `blocks`-th analysed block, each dump collected and delivered once that block's analysis
// event has fired.  What the stage is, its calls of the C-ABI, the two stages below say; the bookkeeping is written once, here.
struct accum_stage : stage {
    struct texts {
        const char *title, *sink_failed_at, *blocks_range, *sink_needs_blocks, *needs_block_launches;
    };
    const texts t;
    const int blocks;              // blocks per dump (0: off)
    const bool has_sink;
    uint64_t observation_result::*const dumps_out;
    std::deque<issued> pending;    // dumps issued and not yet collected -- {last block of the integration, its first block}
    std::vector<int64_t> host;     // what collect returns for one dump
    uint64_t blocks_pushed = 0, dumps = 0;
    accum_stage(run_env& env, const texts& txt, int b, bool sink, uint64_t observation_result::*out)
        : stage(env), t(txt), blocks(b), has_sink(sink), dumps_out(out) {}
    virtual int make(int max_in_flight, size_t* n_int64) = 0;   // the stage, and the size of one dump
    virtual int push(int q, int slot, int first_unit, int n_units) = 0;
    virtual int dump() = 0;
    virtual int collect(uint64_t* n_columns) = 0;
    virtual bool to_sink(uint64_t first_block, uint64_t n_columns) = 0;   // if there is one
    int check() override
    {
        if (blocks < 0) return refuse(t.blocks_range);
        if (has_sink && !blocks) return refuse(t.sink_needs_blocks);
        return !opt.block_launch && blocks ? refuse_unit_launches() : BF_OK;
    }
    const char* unit_launch_refusal() override { return blocks ? t.needs_block_launches : nullptr; }
    int create() override
    {
        if (blocks <= 0) return BF_OK;
        size_t n_int64 = 0;   // dumps in flight: one per block queued at most, + the one being delivered
        const int rc = make(kMaxTotalSep + 2, &n_int64);
        if (rc != BF_OK) return fail(rc);
        host.resize(n_int64);
        return BF_OK;
    }
    // reads the same resident units on the same queue, behind the detect launch and what follows it
    int after_launch(int q, uint64_t, int gpu_block, int first, int upl) override { return blocks > 0 ? push(q, gpu_block, first, upl) : BF_OK; }
    int after_block(uint64_t block_index) override
    {
        if (blocks <= 0 || ++blocks_pushed % (uint64_t)blocks) return BF_OK;
        if (const int rc = dump()) return fail(rc);   // the integration is complete: snapshot and zero
        pending.push_back({block_index, block_index + 1 - (uint64_t)blocks});
        return BF_OK;
    }
    int per_deliver(uint64_t blocks_analyzed) override
    {
        uint64_t n_columns = 0;
        return drain(*this, pending, blocks_analyzed, t.sink_failed_at,
                     [&](uint64_t*) {
                         const int rc = collect(&n_columns);
                         if (rc == BF_OK) dumps++;
                         return rc;
                     },
                     [&](uint64_t first_block) { return to_sink(first_block, n_columns); });
    }
    void report(observation_result* res) override
    {
        if (res) res->*dumps_out = dumps;
        if (blocks > 0)
            log << t.title << ": " << dumps << " dumps of " << blocks << " blocks each (an incomplete integration at the end is dropped)" << std::endl;
    }
};

// ---- the correlator (docs/CORRELATOR.md) ----
struct corr_stage : accum_stage {
    bf_corr* corr = nullptr;
    explicit corr_stage(run_env& env)
        : accum_stage(env, {"Correlator", "visibility sink failed at block", "run_observation: corr_blocks must be 0 (off) or the blocks per dump",
                            "run_observation: a vis_sink needs corr_blocks > 0", "run_observation: the correlator needs block-granular launches"},
                      env.opt.corr_blocks, env.opt.vis_sink != nullptr, &observation_result::vis_dumps) {}
    int make(int n, size_t* n_int64) override
    {
        *n_int64 = 2 * bf_corr_entries(&cfg);
        return bf_corr_create(e.dev.h, n, &corr);
    }
    int push(int q, int slot, int first, int n) override { return bf_corr_push_block(corr, q, slot, first, n); }
    int dump() override { return bf_corr_dump(corr, nullptr); }
    int collect(uint64_t* n) override { return bf_corr_collect(corr, host.data(), n); }
    bool to_sink(uint64_t b, uint64_t n) override { return !opt.vis_sink || opt.vis_sink->deliver(b, n, host.data(), host.size()); }
    void close_sink() override { close(opt.vis_sink); }
    void destroy() override { bf_corr_destroy(corr); }
};

// ---- the voltage moments (docs/SPECTRAL_KURTOSIS.md) ----
struct sk_stage : accum_stage {
    bf_sk* sk = nullptr;
    explicit sk_stage(run_env& env)
        : accum_stage(env, {"Voltage moments", "moments sink failed at block", "run_observation: sk_blocks must be 0 (off) or the blocks per dump",
                            "run_observation: a sk_sink needs sk_blocks > 0", "run_observation: the voltage moments need block-granular launches"},
                      env.opt.sk_blocks, env.opt.sk_sink != nullptr, &observation_result::sk_dumps) {}
    int make(int n, size_t* n_int64) override
    {
        *n_int64 = 2 * bf_sk_entries(&cfg);
        return bf_sk_create(e.dev.h, n, &sk);
    }
    int push(int q, int slot, int first, int n) override { return bf_sk_push_block(sk, q, slot, first, n); }
    int dump() override { return bf_sk_dump(sk, nullptr); }
    int collect(uint64_t* n) override { return bf_sk_collect(sk, host.data(), n); }
    bool to_sink(uint64_t b, uint64_t n) override { return !opt.sk_sink || opt.sk_sink->deliver(b, n, host.data(), host.size()); }
    void close_sink() override { close(opt.sk_sink); }
    void destroy() override { bf_sk_destroy(sk); }
};

constexpr size_t kStokesSetBytesMax = (size_t)8 << 30;   // all result sets of a run's Stokes stage, per side (device, pinned)

// ---- the Stokes beams (docs/STOKES.md): one set per launch ----
struct stokes_stage : stage {
    using stage::stage;
    bf_stokes* stokes = nullptr;
    std::deque<issued> pending;    // pushes issued and not yet collected -- {block of the launch, its first gemm-unit}
    std::vector<int8_t> weights;   // the host weights the handle got: what the stage's beams are picked from
    std::vector<int64_t> host;     // what the collect returns for one push
    uint64_t units = 0;
    int n_int() const { return opt.stokes_int ? opt.stokes_int : cfg.n_avg; }
    int check() override
    {
        if (opt.stokes_beams.empty() && (opt.stokes_sink || opt.stokes_int)) return refuse("run_observation: a stokes_sink / stokes_int needs stokes_beams");
        if (opt.stokes_beams.empty()) return BF_OK;
        if (!opt.block_launch) return refuse_unit_launches();
        if (opt.stokes_beams.size() > (size_t)BF_STOKES_MAX_BEAMS) return refuse("run_observation: stokes_beams holds more than BF_STOKES_MAX_BEAMS beams");
        for (int b : opt.stokes_beams)
            if (b < 0 || b >= cfg.n_beams) return refuse("run_observation: a stokes_beams index is not a beam");
        if (n_int() < 1 || (cfg.n_out_per_gemm * cfg.n_avg) % n_int()) return refuse("run_observation: stokes_int must divide n_out_per_gemm * n_avg");
        return BF_OK;
    }
    const char* unit_launch_refusal() override
    {
        return opt.stokes_beams.empty() ? nullptr : "run_observation: the Stokes beams need block-granular launches";
    }
    int create() override   // sets in flight: as the DM chunks -- the launches of the blocks queued + the one being delivered
    {
        if (opt.stokes_beams.empty()) return BF_OK;
        const int n_sel = (int)opt.stokes_beams.size(), n_sets = (kMaxTotalSep + 2) * (cfg.n_gemms_per_block / plan.upl);
        // The C-ABI sizes every set for a whole block, on the device and again pinned: small launches multiply that.  Reported, and
        // refused beyond kStokesSetBytesMax per side before anything is allocated.
        const size_t set_bytes = (size_t)cfg.n_gemms_per_block * bf_stokes_entries(&cfg, n_sel, n_int()) * 4 * sizeof(int64_t);
        log << "Stokes beams: " << n_sets << " result sets of " << (set_bytes >> 20) << " MiB, on the device and pinned" << std::endl;
        if ((size_t)n_sets * set_bytes > kStokesSetBytesMax) {
            log << "ERROR: the Stokes result sets exceed " << (kStokesSetBytesMax >> 30) << " GiB per side" << std::endl;
            return refuse("run_observation: the Stokes result sets (sets in flight x a block of entries) exceed 8 GiB on the device "
                          "and pinned: fewer stokes_beams, a longer stokes_int or more units_per_launch");
        }
        int rc = bf_stokes_create(e.dev.h, n_int(), n_sets, &stokes);
        if (rc != BF_OK) return fail(rc);
        if ((rc = bf_stokes_set_weights(stokes, weights.data(), opt.stokes_beams.data(), n_sel)) != BF_OK) return fail(rc);
        host.resize(4 * (size_t)plan.upl * bf_stokes_entries(&cfg, n_sel, n_int()));
        std::vector<int8_t>().swap(weights);
        return BF_OK;
    }
    int after_launch(int q, uint64_t block_index, int gpu_block, int first, int upl) override
    {
        if (!stokes) return BF_OK;
        const int rc = bf_stokes_push_block(stokes, q, gpu_block, first, upl);
        if (rc == BF_OK) pending.push_back({block_index, block_index * (uint64_t)cfg.n_gemms_per_block + (uint64_t)first});
        return rc;
    }
    int per_deliver(uint64_t blocks_analyzed) override
    {
        int n = 0;
        return drain(*this, pending, blocks_analyzed, "Stokes sink failed at gemm-unit",
                     [&](uint64_t*) {
                         const int rc = bf_stokes_collect(stokes, host.data(), &n);
                         if (rc == BF_OK) units += (uint64_t)n;
                         return rc;
                     },
                     [&](uint64_t first_unit) { return !opt.stokes_sink || opt.stokes_sink->deliver(first_unit, (uint64_t)n, host.data(), host.size()); });
    }
    void close_sink() override { close(opt.stokes_sink); }
    void report(observation_result* res) override
    {
        if (res) res->stokes_units = units;
        if (stokes)
            log << "Stokes beams: " << opt.stokes_beams.size() << " beams, windows of " << n_int() << " samples, " << units << " gemm-units" << std::endl;
    }
    void destroy() override { bf_stokes_destroy(stokes); }
};

// The stages of a run.  Every step of the loop has its own order among them -- what follows a launch on its queue is not the order of
// creation, nor that of the closing lines -- so each walk below and in production_run names the stages of its step, in that step's order.
struct run_stages {
    run_env& e;
    dm_stage dm{e};
    inj_stage inj{e, dm};
    cond_stage cond{e, dm};
    psr_stage psr{e, dm};
    ffa_stage ffa{e, dm};
    sps_stage sps{e, dm};
    event_stage events{e, sps};
    stamp_stage stamps{e, dm, events};
    vcut_stage vcut{e, dm, events};
    ib_stage ib{e};
    corr_stage corr{e};
    sk_stage sk{e};
    stokes_stage stokes{e};
    explicit run_stages(run_env& env) : e(env) {}
    // Teardown: sync first, then the stages in this order -- all of them before their handle (run_device, which the run releases next).
    ~run_stages()
    {
        if (e.dev.h) bf_stream_sync(e.dev.h, -1);
        walk({&corr, &sk, &stokes, &vcut, &sps, &events, &cond, &psr, &ffa, &inj, &dm}, &stage::destroy);
    }
    // The option combinations run_observation refuses, before anything is read or created.
    int check()
    {
        const observation_options& opt = e.opt;
        if (e.cfg.n_gemms_per_block % e.cfg.n_streams) return BF_ERR_INVALID;
        if (opt.world < 1 || opt.rank < 0 || opt.rank >= opt.world || opt.gather_root < BF_GATHER_ROOT_ALL || opt.gather_root >= opt.world)
            return refuse("run_observation: need 0 <= rank < world and gather_root a rank or BF_GATHER_ROOT_ALL");
        if (opt.comm && (bf_comm_rank(opt.comm) != opt.rank || bf_comm_world(opt.comm) != opt.world))
            return refuse("run_observation: the communicator's rank / world differ from the options'");
        if (opt.comm && !opt.block_launch) return refuse(kGatherNeedsBlockLaunches);
        if (opt.comm && opt.sink && !holds_band(opt)) return refuse("run_observation: only the gather root may have a sink");
        if (const int rc = walk({&dm, &sps, &events, &stamps, &vcut, &cond, &ib, &corr, &psr, &inj, &ffa, &sk, &stokes}, &stage::check)) return rc;
        return dm.check_sharded();
    }
    // The launch plan, from the options and the lab switches.  DSABF_UNIT_LAUNCH can turn block launches off after the options have
    // passed: the stages that need them are asked again.
    int resolve_plan()
    {
        const bf_config& cfg = e.cfg;
        const observation_options& opt = e.opt;
        launch_plan& p = e.plan;
        const char* unit_env = lab_getenv("DSABF_UNIT_LAUNCH");   // measurement / test switch: the reference's per-gemm-unit launches
        p.block_launch = opt.block_launch && !(unit_env && unit_env[0] == '1');
        if (opt.comm && !p.block_launch) return refuse(kGatherNeedsBlockLaunches);
        p.upl = opt.units_per_launch;
        if (const char* env = lab_getenv("DSABF_UNITS_PER_LAUNCH")) p.upl = atoi(env);
        if (p.upl <= 0 || p.upl > cfg.n_gemms_per_block || opt.comm) p.upl = cfg.n_gemms_per_block;   // 0 / sharded: the whole block
        while (cfg.n_gemms_per_block % p.upl) p.upl--;                                                  // whole launches only
        // whole blocks alternate between TWO queues (block i + 1's kernel under block i's copies, as in the DEBUG flow):
        // more queues only put more concurrent host copies beside the H2D stream (9.6 -> 9.2 us per beam-block, and
        // 11.6 -> 9.x with other streams alive in the process: tools/stream_queues.py); sub-block launches rotate over all
        p.n_queues_used = p.upl == cfg.n_gemms_per_block ? std::min(cfg.n_streams, 2) : cfg.n_streams;
        p.staged = opt.gather_staged;
        if (const char* env = lab_getenv("DSABF_GATHER_STAGED")) p.staged = env[0] == '1';
        p.is_root = holds_band(opt);
        // dm_split_trials: every rank holds the whole band (one all-gather instead of a gather) and takes ITS share of the trial ladder --
        // the DM work scales with the GPUs, the path still has ONE collective; rank r: trials [r n / R, (r + 1) n / R), the first n % R
        // ranks one more
        p.dm_count = opt.n_dm;
        if (opt.dm_split_trials) dm_trial_share(opt.n_dm, opt.world, opt.rank, &p.dm_first, &p.dm_count);
        p.n_freq_band = cfg.n_freq * (opt.comm ? opt.world : 1);
        p.dm_rows = p.upl * cfg.n_out_per_gemm;
        for (stage* s : std::initializer_list<stage*>{&dm, &corr, &sk, &stokes})
            if (!p.block_launch && s->unit_launch_refusal()) return s->refuse_unit_launches();
        // a sharded run dedisperses the gathered band (more ranks than trials: the surplus ranks only beamform)
        p.dm_run = opt.dm_delays && p.is_root && p.dm_count > 0;
        return BF_OK;
    }
    int create()
    {
        if (const int rc = walk({&dm, &inj, &cond, &psr, &ffa, &sps, &events, &stamps, &vcut, &corr, &sk, &stokes}, &stage::create)) return rc;
        if (e.plan.block_launch)   // the per-queue block buffers are allocated on first use: do that here, not inside the timed loop
            for (int q = 0; q < e.plan.n_queues_used; q++) {
                float* unused = nullptr;
                int rc = BF_OK;
                if ((!e.plan.dm_run || e.opt.comm) && (rc = bf_block_output_device(e.dev.h, q, &unused)) != BF_OK) return rc;   // (a DM stage takes the rows itself)
                if (e.opt.comm && e.plan.is_root && !e.plan.dm_run && (rc = bf_block_gather_device(e.dev.h, q, e.opt.world, &unused)) != BF_OK) return rc;
                if (e.opt.comm && e.plan.staged && e.plan.is_root && (rc = bf_block_gather_stage_device(e.dev.h, q, e.opt.world, &unused)) != BF_OK) return rc;
            }
        return BF_OK;
    }
};

// One production run: its device and plan, its stages, and what the steps of the loop itself hand to each other.
struct production_run {
    run_env e;
    run_stages s{e};
    const bf_config& cfg = e.cfg;
    const observation_options& opt = e.opt;
    std::ostream& log = e.log;
    const launch_plan& plan = e.plan;
    // beam_out: the reference's pinned D2H destination (:249), [stream][beam_out_stride]; the root of a sharded run receives the whole band there
    const size_t n_f_per_detect = bf_floats_per_detect(&cfg), beam_out_stride = n_f_per_detect * (size_t)(opt.comm ? opt.world : 1);
    float* beam_out = nullptr;
    std::vector<int> timeSlice;           // :319
    std::vector<long long> last_gemm;     // the gemm-unit beam_out[q] ends up holding
    std::vector<float*> unit_dst;         // the D2H destination of every unit of the block being launched
    uint64_t launch_seq = 0, sink_committed = 0;
    std::deque<dm_chunk> dm_pending;      // pushed, not yet delivered (their block's analysis event has not fired)

    int create_handle_and_weights(const antenna* pos, const beam_direction* dir)
    {
        int rc = bf_create(&cfg, opt.device, &e.dev.h);
        if (rc != BF_OK) return gpu_error(log, rc);
        if ((rc = e.dev.alloc_pinned(beam_out_stride * cfg.n_streams, &beam_out)) != BF_OK) return rc;
        ::memset(beam_out, 0, beam_out_stride * cfg.n_streams * sizeof(float));
        std::vector<int8_t> fourier_coefficients((size_t)cfg.n_freq * cfg.n_ant * cfg.n_beams * 2);
        generate_fourier_coefficients(cfg.n_beams, cfg.n_ant, cfg.n_freq, opt.rank * cfg.n_freq, opt.gpu, pos, dir, fourier_coefficients.data());
        const bool follow = !opt.stokes_beams.empty();   // (the Stokes stage takes the weights as they were set: calibrated, in place)
        rc = set_run_weights(e.dev.h, opt.device, fourier_coefficients, opt.gains, opt.nulls, opt.ant_flags, follow ? fourier_coefficients.data() : nullptr, log);
        if (rc != BF_OK) return rc;
        if (follow) s.stokes.weights.swap(fourier_coefficients);
        return opt.incoherent_beam >= 0 ? bf_set_incoherent_beam(e.dev.h, opt.incoherent_beam) : BF_OK;
    }

    // :378-401: the next block of the source to its slot of the device ring, or the end of the observation
    int transfer_block(observation_loop_state& obs_state, block_source& source, size_t block_bytes)
    {
        char* block = source.read();             // :384
        if (!source.check_transfers_complete()) {  // :386
            const int rc = bf_submit_block(e.dev.h, (int)obs_state.get_next_gpu_transfer_block(), block, block_bytes, nullptr);  // :389-393
            if (rc != BF_OK) return gpu_error(log, rc);
            obs_state.generate_transfer_event();  // :396
            if (source.close_releases_block())      // not in the reference: see block_source::close_releases_block
                while (obs_state.status() == BF_OK && obs_state.get_blocks_transferred() < obs_state.get_blocks_transfer_queue())
                    obs_state.check_transfer_events();
        } else {
            obs_state.set_transfers_complete(true);  // :398
        }
        source.close();  // :401
        return BF_OK;
    }

    // unit gemm_index's powers go to its sink slot, or to `fallback`; nullptr (logged): the sink is full
    float* unit_destination(float* fallback, uint64_t gemm_index)
    {
        if (!opt.sink) return fallback;
        float* slot = opt.sink->acquire(gemm_index);
        if (!slot) log << "ERROR: detected sink has no free slot" << std::endl;
        return slot;
    }

    // :452-519: the launches of the block at the head of the analysis queue, in the plan's pattern
    int analyse_block(const observation_loop_state& obs_state)
    {
        const int n_units = cfg.n_gemms_per_block;
        const long long block_index = (long long)obs_state.get_blocks_analysis_queue();
        const int gpu_block = (int)obs_state.get_next_gpu_analysis_block();
        if (!plan.block_launch)   // the reference's launch pattern; beam_out[st] is the reference's destination, :485-488
            return enqueue_block_by_units(e.dev.h, cfg, gpu_block, timeSlice, log, nullptr, [&](int st, int unit) {
                last_gemm[st] = block_index * n_units + unit;
                return unit_destination(&beam_out[(size_t)st * n_f_per_detect], (uint64_t)last_gemm[st]);
            });
        unit_dst.assign((size_t)n_units, nullptr);
        for (int first = 0; first < n_units; first += plan.upl)
            if (const int rc = launch_units(block_index, gpu_block, first)) return rc;
        return walk({&s.corr, &s.sk}, &stage::after_block, (uint64_t)block_index);
    }

    // One block launch over the gemm-units [first, first + upl) of the block, with everything that follows it on its queue.
    int launch_units(long long block_index, int gpu_block, int first)
    {
        const int n_units = cfg.n_gemms_per_block, upl = plan.upl;
        const int q = (int)(launch_seq++ % (uint64_t)plan.n_queues_used);   // (why these queues: resolve_plan)
        // unit u's powers go to its sink slot, or to beam_out[queue of its launch] (later units on that queue
        // overwrite earlier ones, in order: beam_out[q] ends up holding gemm-unit last_gemm[q])
        for (int u = first; u < first + upl; u++) {
            unit_dst[u] = unit_destination(&beam_out[(size_t)q * beam_out_stride], (uint64_t)block_index * n_units + u);
            if (!unit_dst[u]) return BF_ERR_STATE;
            last_gemm[q] = block_index * n_units + u;
        }
        // The DM stage owns the place its rows belong in -- directly behind its carried-over delay window: the beamformer
        // (one GPU) or the gather (a holder of a sharded run) writes them THERE, and the push below only launches.  The
        // reference's collapse reads what detect wrote, no copy in between (src/beamformer.cu:481,492-511).
        float* d_rows = nullptr;     // where this launch's beam-blocks are on the device, [row][freq (over the band)][beam]
        void* dm_qs = nullptr;
        int rc = BF_OK;
        if (plan.dm_run && (rc = bf_queue_stream(e.dev.h, q, &dm_qs)) == BF_OK) rc = bf_dm_stream_reserve(s.dm.stream, plan.dm_rows, &d_rows, dm_qs);
        if (rc == BF_OK)
            rc = (plan.dm_run && !opt.comm) ? bf_enqueue_block_to(e.dev.h, q, gpu_block, first, upl, d_rows, &unit_dst[first])
                                            : bf_enqueue_block(e.dev.h, q, gpu_block, first, upl, opt.comm ? nullptr : &unit_dst[first]);
        if (rc == BF_OK && opt.comm) rc = gather_block(q, d_rows);
        if (rc == BF_OK && plan.dm_run) rc = s.dm.push((uint64_t)block_index, d_rows, dm_qs, dm_pending);
        if (rc == BF_OK && plan.dm_run) rc = walk({&s.psr}, &stage::after_dm_push, (uint64_t)block_index, dm_qs);
        // the taps on the resident units, on the same queue: the correlator, the voltage moments, the Stokes beams, the voltage history
        if (rc == BF_OK) rc = walk({&s.corr, &s.sk, &s.stokes, &s.vcut}, &stage::after_launch, q, (uint64_t)block_index, gpu_block, first, upl);
        return rc == BF_OK ? BF_OK : gpu_error(log, rc);
    }

    // sharded (upl == n_units): bring the shards' powers together on the root, in [unit][o][f over the band][b], behind the launch on
    // the same queue; only the root copies to the host
    int gather_block(int q, float* d_rows)
    {
        const int n_units = cfg.n_gemms_per_block;
        float *d_blk = nullptr, *d_full = nullptr, *d_stage = nullptr;
        void* qs = nullptr;
        const size_t full_det = n_f_per_detect * (size_t)opt.world;
        const size_t rows = (size_t)n_units * cfg.n_out_per_gemm, row_floats = (size_t)cfg.n_freq * cfg.n_beams;
        const bool root = plan.is_root;
        if (plan.dm_run) d_full = d_rows;     // (a holder with a DM stage receives straight into the stage's buffer)
        int rc = bf_block_output_device(e.dev.h, q, &d_blk);
        if (rc == BF_OK) rc = bf_queue_stream(e.dev.h, q, &qs);
        if (rc == BF_OK && root && !plan.dm_run) rc = bf_block_gather_device(e.dev.h, q, opt.world, &d_full);
        if (rc == BF_OK && root && plan.staged) rc = bf_block_gather_stage_device(e.dev.h, q, opt.world, &d_stage);
        if (rc == BF_OK)
            rc = plan.staged ? bf_gather_detected_staged(opt.comm, d_blk, rows, row_floats, opt.gather_root, d_full, d_stage, qs)
                             : bf_gather_detected(opt.comm, d_blk, rows, row_floats, opt.gather_root, BF_GATHER_LAYOUT_FREQ_MAJOR, d_full, qs);
        for (int u = 0; rc == BF_OK && root && u < n_units; u++)
            rc = bf_enqueue_d2h(e.dev.h, q, d_full + full_det * (size_t)u, unit_dst[u], full_det);
        return rc;
    }

    // What the blocks analysed so far finished: their DM chunks have landed (their copies sit on the queues the analysis event joins),
    // and so has every D2H copy of their gemm-units: hand those over, in order.
    int deliver(uint64_t blocks_analyzed)
    {
        while (!dm_pending.empty() && dm_pending.front().block < blocks_analyzed) {
            const dm_chunk c = dm_pending.front();
            dm_pending.pop_front();
            if (const int rc = walk({&s.sps, &s.events, &s.vcut, &s.stamps, &s.ffa, &s.dm}, &stage::per_chunk, c)) return rc;
        }
        if (const int rc = walk({&s.stamps, &s.vcut, &s.corr, &s.sk, &s.psr, &s.stokes}, &stage::per_deliver, blocks_analyzed)) return rc;
        for (; opt.sink && sink_committed < blocks_analyzed * (uint64_t)cfg.n_gemms_per_block; sink_committed++)
            if (!opt.sink->commit(sink_committed)) {
                log << "ERROR: detected sink failed at gemm-unit " << sink_committed << std::endl;
                return BF_ERR_STATE;
            }
        return BF_OK;
    }
};

}  // namespace

int run_observation(const bf_config& cfg, const observation_options& opt, block_source& source, const antenna* pos,
                    const beam_direction* dir, observation_result* res, std::ostream& log)
{
    setup_gate gate{opt.comm};
    production_run run{{cfg, opt, log}};
    run_stages& s = run.s;
    int rc = s.check();
    if (rc != BF_OK) return gate.fail(rc);
    source.read_headers();  // :334 (before the device exists here: the block-size check below needs no GPU)
    const size_t block_bytes = bf_bytes_per_block(&cfg);
    if (source.get_block_size() != block_bytes) {
        // The reference prints this (src/beamformer.cu:336-339) and carries on; every ring block is then copied with the
        // GEOMETRY's size: a smaller ring block is read past its end (past the mapping on the last one), a larger one is
        // silently truncated.  Neither can produce a meaningful beam: refuse.
        log << "ERROR: block size " << source.get_block_size() << ", Should also be " << block_bytes << std::endl;
        return gate.fail(set_error(BF_ERR_INVALID, "run_observation: the source's block size does not match bf_bytes_per_block(cfg)"));
    }

    for (int i = 0; i < cfg.n_streams; i++) run.timeSlice.push_back(i);  // :319
    run.last_gemm.assign((size_t)cfg.n_streams, -1);
    if ((rc = run.create_handle_and_weights(pos, dir)) != BF_OK) return gate.fail(rc);
    bf_handle* const h = run.e.dev.h;
    hip_backend backend(h);
    observation_loop_state obs_state(kMaxTransferSep, kMaxTotalSep, cfg, &backend, /*debug_mode=*/false);  // :322
    if (opt.burn_in > 0) {  // :348-355
        log << "Burning IN" << std::endl;
        for (int i = 0; i < opt.burn_in; i++) {
            source.read();
            source.close();
        }
        log << "Done Burn in" << std::endl;
    }
    if ((rc = s.resolve_plan()) != BF_OK) return gate.fail(rc);
    if ((rc = s.create()) != BF_OK) return gate.fail(rc);
    if ((rc = gate.pass(opt.local_setup_ok)) != BF_OK) return rc;

    bf_timer_start(h);  // :358
    while (!obs_state.check_observations_complete()) {  // :364
        if (opt.verbose) log << "##########################################" << std::endl << obs_state << std::endl;
        if (obs_state.check_ready_for_transfer())  // :378
            if ((rc = run.transfer_block(obs_state, source, block_bytes)) != BF_OK) return rc;
        obs_state.check_transfer_events();  // :446
        if (obs_state.check_ready_for_analysis()) {  // :452
            if ((rc = run.analyse_block(obs_state)) != BF_OK) return rc;
            obs_state.generate_analysis_event();  // :525
        }
        obs_state.check_analysis_events();  // :532
        if (obs_state.status() != BF_OK) return event_backend_error(log, obs_state);
        if ((rc = run.deliver(obs_state.get_blocks_analyzed())) != BF_OK) return rc;
    }
    float ms = 0;
    bf_timer_stop(h, &ms);
    bf_stream_sync(h, -1);  // :560-562
    // the end of the run: the events still open close, then one last round of voltage cuts and of stamps
    if ((rc = walk({&s.events, &s.vcut, &s.stamps}, &stage::finish)) != BF_OK) return rc;
    walk({&s.events, &s.stamps, &s.vcut}, &stage::close_sink);
    if (opt.sink) opt.sink->close();
    walk({&s.dm, &s.sps, &s.corr, &s.sk, &s.stokes, &s.psr, &s.ffa}, &stage::close_sink);
    const uint64_t chunks = obs_state.get_current_transfer_gemm() * cfg.n_out_per_gemm;  // :552
    const double rate = (double)source.get_block_size() * obs_state.get_blocks_transfer_queue() / ms / 1e6;  // :554
    closing_report(log, ms, chunks, ms / (chunks ? chunks : 1), rate, run.plan.block_launch ? "bf_enqueue_block" : kUnitLaunchPattern);
    if (res) {
        res->observation_time_ms = ms;
        res->blocks = obs_state.get_blocks_analyzed();
        res->data_chunks = chunks;
        res->gbytes_per_s = rate;
        res->beam_out.assign(run.beam_out, run.beam_out + run.beam_out_stride * cfg.n_streams);
        res->last_gemm = run.last_gemm;
    }
    walk({&s.dm, &s.cond, &s.ib, &s.corr, &s.sk, &s.stokes, &s.inj, &s.psr, &s.ffa, &s.sps, &s.stamps, &s.vcut}, &stage::report, res);
    return BF_OK;
}

}  // namespace dsabf
