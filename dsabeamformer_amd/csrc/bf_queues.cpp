// bf_queues.cpp -- the compute queues of a handle (include/dsabf.h): the coalescing of bf_enqueue_gemm_unit, the per-queue block
// buffers, and the copies and syncs that order a caller's work against the queues.
#include "bf_runtime_internal.h"
#include "ib/bf_incoherent.h"

int dsabf::rt::launch_detect(bf_handle* h, const void* in, int n_units, float* out, hipStream_t s)
{
    h->n_fused_launches++;
    HIP_TRY(dsabf::launch_fused(h->geom, h->d_wimage, h->d_wimage_p, h->d_wimage_f, in, n_units, out, h->n_cus, s));
    if (h->ib_beam >= 0)   // the tied beam of that column has been computed like every other: overwrite it
        HIP_TRY(dsabf::launch_incoherent(h->geom.n_ant, h->geom.n_freq, h->geom.n_ipo, h->geom.n_out, in, n_units, out + h->ib_beam,
                                         (size_t)h->geom.n_beams, h->n_cus, s));
    return BF_OK;
}

static int check_queue(const bf_handle* h, int q)
{
    return q >= 0 && q < h->cfg.n_streams ? BF_OK : fail(BF_ERR_INVALID, "stream %d out of range", q);
}

static int check_units(const bf_handle* h, int first_unit, int n_units)
{
    if (first_unit >= 0 && n_units > 0 && first_unit + n_units <= h->cfg.n_gemms_per_block) return BF_OK;
    return fail(BF_ERR_INVALID, "gemm-units [%d, %d) are not inside a block of %d", first_unit, first_unit + n_units, h->cfg.n_gemms_per_block);
}

// a launch on compute queue q that reads ring slot `slot`
static int check_queue_and_slot(const bf_handle* h, int q, int slot)
{
    if (int rc = check_queue(h, q)) return rc;
    if (slot < 0 || slot >= h->cfg.n_blocks_on_gpu) return fail(BF_ERR_INVALID, "slot %d out of range", slot);
    return BF_OK;
}

int dsabf::rt::resident_units(const bf_handle* h, int stream_idx, int slot, int first_unit, int n_units, const uint8_t** in)
{
    if (int rc = check_queue_and_slot(h, stream_idx, slot)) return rc;
    if (int rc = check_units(h, first_unit, n_units)) return rc;
    // src/beamformer.cu:464: &d_data[N_BYTES_PRE_EXPANSION_PER_GEMM*(N_GEMMS_PER_BLOCK*block + timeSlice)]
    *in = h->d_data + bf_bytes_per_gemm(&h->cfg) * ((size_t)h->cfg.n_gemms_per_block * slot + first_unit);
    return BF_OK;
}

// One of a queue's block buffers (bf_handle::queue_bufs): n_floats of device memory, allocated at its first use.
static int ensure_buf(float*& p, size_t n_floats)
{
    if (!p) HIP_TRY(hipMalloc((void**)&p, n_floats * sizeof(float)));
    return BF_OK;
}

// Queue `waiter` runs what it is given next behind everything queue `producer` has been given so far (the same queue: nothing to do).
static int queue_waits_for(bf_handle* h, int waiter, int producer)
{
    if (waiter == producer) return BF_OK;
    HIP_TRY(hipEventRecord(h->join[producer], h->streams[producer]));
    HIP_TRY(hipStreamWaitEvent(h->streams[waiter], h->join[producer], 0));
    return BF_OK;
}

// The host copies of units [0, n), `stride` floats each: unit k from src(k) on the device to dst(k) (NULL: none).  Units that
// continue each other on the device (next(k): unit k follows unit k - 1) and whose destinations follow each other travel as ONE copy.
template <class Dst, class Src, class Next>
static int copy_runs_to_host(size_t n, size_t stride, Dst dst, Src src, Next next, hipStream_t s)
{
    for (size_t i = 0; i < n;) {
        if (!dst(i)) {
            i++;
            continue;
        }
        size_t j = i + 1;
        while (j < n && next(j) && dst(j) == dst(j - 1) + stride) j++;
        HIP_TRY(hipMemcpyAsync(dst(i), src(i), stride * sizeof(float) * (j - i), hipMemcpyDeviceToHost, s));
        i = j;
    }
    return BF_OK;
}

// Launches what bf_enqueue_gemm_unit / bf_enqueue_dedisperse have queued: per run of consecutive gemm-units of one ring
// slot ONE fused launch (the reference's loop enqueues time slices 0, 1, 2, ... of a block: one run = the block), one
// DM-0 launch per run of units that asked for it, and the host copies -- every unit's, in the order they were enqueued,
// neighbours in device AND host memory as one copy.  All of it on ONE compute queue (they rotate per flush); the host copies
// wait for the previous flush's, so that two units copied to the same host buffer land in enqueue order as they do on
// the reference's per-queue streams (src/beamformer.cu:485-488 overwrites beam_out[stream] unit after unit), while this
// flush's kernel already overlaps the previous flush's copies.
// A launch on compute queue q is about to overwrite gemm-units [ts0, ts1) of that queue's block buffer.  A caller-visible queue
// whose MOST RECENT gemm-unit's powers still live there -- bf_enqueue_dedisperse may yet be called for it: "the unit last
// enqueued on stream_idx", include/dsabf.h -- and that is not given a newer unit by this very launch (`reassigned`) gets them
// moved to its own slot of d_out first: behind whatever queue s still has in flight on that slot (a literal-pattern unit's
// host copy), in front of the launch.  Never happens in the reference's loop (a time slice belongs to one queue there).
static int preserve_last_units(bf_handle* h, int q, size_t ts0, size_t ts1, const std::vector<char>* reassigned)
{
    const float* blk = h->qbuf[q].out_blk;
    if (!blk) return BF_OK;
    const size_t per_det = bf_floats_per_detect(&h->cfg);
    const float* lo = blk + per_det * ts0;
    const float* hi = blk + per_det * ts1;
    for (int s = 0; s < h->cfg.n_streams; s++) {
        if (reassigned && (*reassigned)[(size_t)s]) continue;
        const float* p = h->last_out[s];
        if (p < lo || p >= hi) continue;
        float* keep = h->d_out + per_det * (size_t)s;
        if (int rc = queue_waits_for(h, q, s)) return rc;
        HIP_TRY(hipMemcpyAsync(keep, p, per_det * sizeof(float), hipMemcpyDeviceToDevice, h->streams[q]));
        h->last_out[s] = keep;
        h->last_q[s] = q;
    }
    return BF_OK;
}

int dsabf::rt::flush_units(bf_handle* h)
{
    if (h->pending.empty()) return BF_OK;
    std::vector<bf_handle::pending_unit> units;
    units.swap(h->pending);              // (whatever happens below, nothing stays queued)
    // two queues take turns (each owns a block-sized device buffer, allocated at first use): flush i + 1's kernel runs under
    // flush i's host copies; more queues would only hold more buffers
    const int q = (int)(h->flush_seq++ % (uint64_t)(h->cfg.n_streams < 2 ? 1 : 2));
    hipStream_t s = h->streams[q];
    const size_t per_gemm = bf_bytes_per_gemm(&h->cfg), per_det = bf_floats_per_detect(&h->cfg);
    const size_t n_beams = (size_t)h->cfg.n_beams;
    bool any_ded = false;
    for (const auto& u : units) any_ded |= u.ded;
    bf_handle::queue_bufs& qb = h->qbuf[q];
    if (int rc = ensure_buf(qb.out_blk, per_det * (size_t)h->cfg.n_gemms_per_block)) return rc;
    if (any_ded)
        if (int rc = ensure_buf(qb.ded_blk, n_beams * (size_t)h->cfg.n_gemms_per_block)) return rc;
    float* blk = qb.out_blk;
    const size_t n = units.size();
    auto follows = [&](size_t k) {       // unit k continues the run of unit k - 1
        return units[k].slot == units[k - 1].slot && units[k].time_slice == units[k - 1].time_slice + 1;
    };
    std::vector<char> reassigned((size_t)h->cfg.n_streams, 0);   // queues that get a newer "most recent unit" from this flush
    for (const auto& u : units) reassigned[(size_t)u.stream_idx] = 1;
    for (size_t i = 0; i < n;) {
        size_t j = i + 1;
        while (j < n && follows(j)) j++;
        const uint8_t* in = h->d_data + per_gemm * ((size_t)h->cfg.n_gemms_per_block * units[i].slot + units[i].time_slice);
        if (int rc = preserve_last_units(h, q, (size_t)units[i].time_slice, (size_t)units[i].time_slice + (j - i), &reassigned)) return rc;
        if (int rc = launch_detect(h, in, (int)(j - i), blk + per_det * (size_t)units[i].time_slice, s)) return rc;
        for (size_t a = i; a < j;) {     // DM-0 rows of the run: one launch per stretch of units that asked for one
            if (!units[a].ded) {
                a++;
                continue;
            }
            size_t b = a + 1;
            while (b < j && units[b].ded) b++;
            HIP_TRY(dsabf::launch_dedisperse_units(h->geom, blk + per_det * (size_t)units[a].time_slice, per_det, (int)(b - a),
                                                   qb.ded_blk + n_beams * (size_t)units[a].time_slice, s));
            a = b;
        }
        i = j;
    }
    if (h->flush_recorded) HIP_TRY(hipStreamWaitEvent(s, h->flush_done, 0));
    if (int rc = copy_runs_to_host(n, per_det, [&](size_t k) { return units[k].host_out; },   // a4: the detected powers
                                   [&](size_t k) { return blk + per_det * (size_t)units[k].time_slice; }, follows, s))
        return rc;
    if (int rc = copy_runs_to_host(n, n_beams, [&](size_t k) { return units[k].ded ? units[k].ded_row : nullptr; },   // a8: the DM-0 rows
                                   [&](size_t k) { return qb.ded_blk + n_beams * (size_t)units[k].time_slice; }, follows, s))
        return rc;
    HIP_TRY(hipEventRecord(h->flush_done, s));
    h->flush_recorded = true;
    // The per-queue ordering guarantee of the literal pattern, kept: every caller-visible queue that had a unit in this flush
    // waits for the flush's end.  Whatever the caller orders on streams[stream_idx] afterwards -- a raw hipStreamSynchronize on
    // the stream bf_queue_stream handed out earlier, its own event, a bf_enqueue_d2h, RCCL chained on it -- is behind the
    // unit's launch AND its host copy, exactly as when the unit itself ran there.
    for (int st = 0; st < h->cfg.n_streams; st++)
        if (reassigned[(size_t)st] && st != q) HIP_TRY(hipStreamWaitEvent(h->streams[st], h->flush_done, 0));
    for (const auto& u : units) {
        h->last_out[u.stream_idx] = blk + per_det * (size_t)u.time_slice;
        h->last_q[u.stream_idx] = q;
    }
    return BF_OK;
}

extern "C" {

int bf_enqueue_gemm_unit(bf_handle* h, int stream_idx, int slot, int time_slice, float* host_out)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    if (int rc = check_weights(h)) return rc;
    if (int rc = check_queue_and_slot(h, stream_idx, slot)) return rc;
    if (time_slice < 0 || time_slice >= h->cfg.n_gemms_per_block)
        return fail(BF_ERR_INVALID, "time_slice %d out of range", time_slice);
    ON_DEVICE(h);
    if (h->coalesce) {
        // a whole block is queued, or this time slice's place in the block buffer is taken: launch what is there first
        bool clash = h->pending.size() >= (size_t)h->cfg.n_gemms_per_block;
        for (const auto& u : h->pending) clash |= u.time_slice == time_slice;
        if (clash) FLUSH_UNITS(h);
        h->pending.push_back({stream_idx, slot, time_slice, host_out, nullptr, false});
        return BF_OK;
    }
    const size_t per_det = bf_floats_per_detect(&h->cfg);
    const uint8_t* in = nullptr;
    if (int rc = resident_units(h, stream_idx, slot, time_slice, 1, &in)) return rc;   // (in range, see above: this asks where the unit is)
    float* out = h->d_out + per_det * (size_t)stream_idx;
    hipStream_t s = h->streams[stream_idx];
    if (h->last_out[stream_idx] == out) {
        // this queue's slot holds powers that preserve_last_units may have moved here on ANOTHER queue (and a DM-0 request may be
        // reading them there): overwrite it behind that queue's work
        if (int rc = queue_waits_for(h, stream_idx, h->last_q[stream_idx])) return rc;
    }
    if (int rc = launch_detect(h, in, 1, out, s)) return rc;
    if (host_out) HIP_TRY(hipMemcpyAsync(host_out, out, per_det * sizeof(float), hipMemcpyDeviceToHost, s));
    h->last_out[stream_idx] = out;
    h->last_q[stream_idx] = stream_idx;
    return BF_OK;
}

// d_dst: where the launch's powers go ([unit][o][f][b] of its n_units gemm-units); NULL: this queue's block buffer
static int enqueue_block_impl(bf_handle* h, int stream_idx, int slot, int first_unit, int n_units, float* d_dst, float* const* host_out)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    if (int rc = check_weights(h)) return rc;
    const uint8_t* in = nullptr;
    if (int rc = resident_units(h, stream_idx, slot, first_unit, n_units, &in)) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);
    const size_t per_det = bf_floats_per_detect(&h->cfg);
    float* out = d_dst;
    if (!d_dst) {
        bf_handle::queue_bufs& b = h->qbuf[stream_idx];
        // This queue's block buffer, at first use.  A hipMalloc in the middle of a stream of blocks stalls the device (measured: 9.4 ->
        // 10.9 us per beam-block), so a caller that rotates over queues reserves them BEFORE its loop with bf_block_output_device
        // (run_observation does, for the queues it will use; include/dsabf.h says so at bf_enqueue_block) -- the library does not
        // guess and allocate all n_streams of them (8 x 128 MiB at the production geometry, six of them dead for a two-queue loop).
        if (int rc = ensure_buf(b.out_blk, per_det * (size_t)h->cfg.n_gemms_per_block)) return rc;
        b.blk_ran = true;
        if (int rc = preserve_last_units(h, stream_idx, (size_t)first_unit, (size_t)first_unit + (size_t)n_units, nullptr)) return rc;
        out = b.out_blk + per_det * (size_t)first_unit;
    }
    hipStream_t s = h->streams[stream_idx];
    if (int rc = launch_detect(h, in, n_units, out, s)) return rc;
    if (!host_out) return BF_OK;
    return copy_runs_to_host((size_t)n_units, per_det, [&](size_t k) { return host_out[k]; }, [&](size_t k) { return out + per_det * k; },
                             [](size_t) { return true; }, s);
}

int bf_enqueue_block(bf_handle* h, int stream_idx, int slot, int first_unit, int n_units, float* const* host_out)
{
    return enqueue_block_impl(h, stream_idx, slot, first_unit, n_units, nullptr, host_out);
}

int bf_enqueue_block_to(bf_handle* h, int stream_idx, int slot, int first_unit, int n_units, float* d_dst, float* const* host_out)
{
    if (!d_dst) return fail(BF_ERR_INVALID, "d_dst is NULL");
    return enqueue_block_impl(h, stream_idx, slot, first_unit, n_units, d_dst, host_out);
}

int bf_enqueue_block_dedisperse(bf_handle* h, int stream_idx, int first_unit, int n_units, float* host_rows)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    if (int rc = check_queue(h, stream_idx)) return rc;
    if (int rc = check_units(h, first_unit, n_units)) return rc;
    if (!h->qbuf[stream_idx].blk_ran)
        return fail(BF_ERR_STATE, "bf_enqueue_block has not run on queue %d", stream_idx);
    ON_DEVICE(h);
    FLUSH_UNITS(h);
    const size_t per_det = bf_floats_per_detect(&h->cfg);
    bf_handle::queue_bufs& b = h->qbuf[stream_idx];
    if (int rc = ensure_buf(b.ded_blk, (size_t)h->cfg.n_beams * (size_t)h->cfg.n_gemms_per_block)) return rc;   // (32 KiB)
    hipStream_t s = h->streams[stream_idx];
    float* ded = b.ded_blk + (size_t)h->cfg.n_beams * first_unit;
    HIP_TRY(dsabf::launch_dedisperse_units(h->geom, b.out_blk + per_det * (size_t)first_unit, per_det, n_units, ded, s));
    if (host_rows)
        HIP_TRY(hipMemcpyAsync(host_rows, ded, (size_t)h->cfg.n_beams * sizeof(float) * (size_t)n_units, hipMemcpyDeviceToHost, s));
    return BF_OK;
}

int bf_block_output_device(bf_handle* h, int stream_idx, float** d_out)
{
    if (!h || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_queue(h, stream_idx)) return rc;
    ON_DEVICE(h);
    bf_handle::queue_bufs& b = h->qbuf[stream_idx];
    if (int rc = ensure_buf(b.out_blk, bf_floats_per_detect(&h->cfg) * (size_t)h->cfg.n_gemms_per_block)) return rc;
    b.blk_ran = true;   // (the caller may fill the buffer itself and ask for its DM-0 rows)
    *d_out = b.out_blk;
    return BF_OK;
}

// bf_block_gather_device / bf_block_gather_stage_device: queue stream_idx's buffer `which`, world block buffers large
static int gather_buf(bf_handle* h, int stream_idx, int world, float* bf_handle::queue_bufs::*which, float** out)
{
    if (!h || !out) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_queue(h, stream_idx)) return rc;
    if (world < 1) return fail(BF_ERR_INVALID, "world must be positive");
    if (h->full_world && h->full_world != world) return fail(BF_ERR_STATE, "the gather buffers were sized for world %d", h->full_world);
    ON_DEVICE(h);
    h->full_world = world;
    float*& p = h->qbuf[stream_idx].*which;
    if (int rc = ensure_buf(p, bf_floats_per_detect(&h->cfg) * (size_t)h->cfg.n_gemms_per_block * (size_t)world)) return rc;
    *out = p;
    return BF_OK;
}

int bf_block_gather_device(bf_handle* h, int stream_idx, int world, float** d_full)
{
    return gather_buf(h, stream_idx, world, &bf_handle::queue_bufs::full_blk, d_full);
}

int bf_block_gather_stage_device(bf_handle* h, int stream_idx, int world, float** d_stage)
{
    return gather_buf(h, stream_idx, world, &bf_handle::queue_bufs::stage_blk, d_stage);
}

int bf_enqueue_d2h(bf_handle* h, int stream_idx, const float* d_src, float* host_dst, size_t n_floats)
{
    if (!h || !d_src || !host_dst) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_queue(h, stream_idx)) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);
    HIP_TRY(hipMemcpyAsync(host_dst, d_src, n_floats * sizeof(float), hipMemcpyDeviceToHost, h->streams[stream_idx]));
    return BF_OK;
}

int bf_queue_stream(bf_handle* h, int stream_idx, void** hip_stream)
{
    if (!h || !hip_stream) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_queue(h, stream_idx)) return rc;
    ON_DEVICE(h);
    FLUSH_UNITS(h);   // the caller is about to order its own work against this queue: nothing of ours may still be only queued
    *hip_stream = h->streams[stream_idx];
    return BF_OK;
}

int bf_enqueue_dedisperse(bf_handle* h, int stream_idx, float* host_out_row)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    if (int rc = check_queue(h, stream_idx)) return rc;
    ON_DEVICE(h);
    // the gemm-unit this call refers to -- the most recent one of queue stream_idx -- may still be queued: its DM-0 row is then
    // part of the same flush (one launch for all the rows of a run)
    for (size_t k = h->pending.size(); k-- > 0;)
        if (h->pending[k].stream_idx == stream_idx) {
            if (h->pending[k].ded) break;   // a second collapse of the same unit: run it directly below
            h->pending[k].ded = true;
            h->pending[k].ded_row = host_out_row;
            return BF_OK;
        }
    FLUSH_UNITS(h);
    // d_ded[stream_idx] and the host row belong to queue stream_idx: every direct request runs THERE, in call order, behind the
    // queue that produced (or moved) the unit's powers if that was another one -- two successive requests can then neither
    // overwrite d_ded under a copy in flight nor land their rows out of order
    hipStream_t s = h->streams[stream_idx];
    const int lq = h->last_q[stream_idx];
    if (int rc = queue_waits_for(h, stream_idx, lq)) return rc;
    float* ded = h->d_ded + (size_t)h->cfg.n_beams * stream_idx;
    HIP_TRY(dsabf::launch_dedisperse(h->geom, h->last_out[stream_idx], ded, s));
    // ... and the producer queue waits for this read: the next launch that overwrites the unit's place in ITS block buffer (a later
    // flush on queue lq, for a queue whose latest unit is being replaced: preserve_last_units skips those) must not start under
    // it.  (Found by tools/fuzz_calls.py, seed 2118: unit, flush on queue A, late DM-0 on its own queue, next flush on A.)
    if (int rc = queue_waits_for(h, lq, stream_idx)) return rc;
    if (host_out_row)
        HIP_TRY(hipMemcpyAsync(host_out_row, ded, (size_t)h->cfg.n_beams * sizeof(float), hipMemcpyDeviceToHost, s));
    return BF_OK;
}

int bf_set_incoherent_beam(bf_handle* h, int beam)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    if (beam < -1 || beam >= h->cfg.n_beams) return fail(BF_ERR_INVALID, "incoherent beam %d: must be -1 (off) or a beam index below %d", beam, h->cfg.n_beams);
    if (beam >= 0 && !dsabf::incoherent_supported(h->geom.n_ant, h->geom.n_ipo))
        return fail(BF_ERR_INVALID, "incoherent beam: 128 * %d antennas * %d samples per output exceeds 2^24 (the sum would not convert to float exactly)",
                    h->geom.n_ant, h->geom.n_ipo);
    ON_DEVICE(h);
    FLUSH_UNITS(h);   // gemm-units still queued were enqueued under the old setting: launch them with it
    h->ib_beam = beam;
    return BF_OK;
}

int bf_record_analysis_event(bf_handle* h, bf_event* ev)
{
    if (!h || !ev) return fail(BF_ERR_INVALID, "NULL argument");
    ON_DEVICE(h);
    FLUSH_UNITS(h);
    const int last = h->cfg.n_streams - 1;
    for (int i = 0; i < last; i++)
        if (int rc = queue_waits_for(h, last, i)) return rc;
    HIP_TRY(hipEventRecord(ev->ev, h->streams[last]));
    ev->recorded = true;
    return BF_OK;
}

int bf_stream_sync(bf_handle* h, int stream_idx)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    ON_DEVICE(h);
    FLUSH_UNITS(h);
    if (stream_idx < 0) {
        HIP_TRY(hipStreamSynchronize(h->h2d));
        for (auto s : h->streams) HIP_TRY(hipStreamSynchronize(s));
        return BF_OK;
    }
    if (int rc = check_queue(h, stream_idx)) return rc;
    HIP_TRY(hipStreamSynchronize(h->streams[stream_idx]));
    if (h->last_q[stream_idx] != stream_idx)   // its most recent gemm-unit was coalesced into a launch on another queue
        HIP_TRY(hipStreamSynchronize(h->streams[h->last_q[stream_idx]]));
    return BF_OK;
}

}  // extern "C"
