// bf_cond.cpp -- conditioning of the detected stream in front of the DM stage (include/dsabf.h: bf_cond_*; contract, ordering and
// measurements: docs/CONDITIONING.md).  The device code is csrc/cond/bf_cond.hip; this file owns the stage's memory, keeps the
// window's row counts and orders the pushes (a bf_chain: bf_runtime_internal.h).
#include <algorithm>
#include <deque>
#include <new>

#include "bf_runtime_internal.h"
#include "cond/bf_cond_kernels.h"

struct bf_cond : bf_stage {
    bf_cond() : bf_stage("conditioner") {}
    int n_freq = 0, n_beams = 0, max_rows = 0, window = 0;
    bool zero_dm = true;
    double k_auto = 0.0;                  // auto_threshold * 1.4826, formed once, here, in fp64
    dsabf::CondBuffers buf{};
    uint8_t* d_static = nullptr;          // the caller's mask (buf.static_mask)
    bf_chain pushes;                      // the pushes share the ring of totals, the per-cell and per-channel scratch and the mask
    std::deque<int> rows_in_window;       // row counts of the pushes in the window, oldest first
    void attached() override { rows_in_window.clear(); }   // attached, in mid-stream or not: the window starts empty there
};

bf_stage* dsabf::rt::as_stage(bf_cond* c) { return c; }

int dsabf::rt::cond_check_attach(const bf_cond* c, const bf_handle* h, int n_freq_total, int max_rows)
{
    if (int rc = orphaned(c)) return rc;
    if (c->h != h) return fail(BF_ERR_INVALID, "bf_dm_stream_attach_conditioner: the two stages belong to different handles");
    if (c->n_freq != n_freq_total)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_conditioner: the conditioner has %d channels, the DM stage %d", c->n_freq, n_freq_total);
    if (c->max_rows < max_rows)
        return fail(BF_ERR_INVALID, "bf_dm_stream_attach_conditioner: max_rows_per_push %d < the DM stage's %d", c->max_rows, max_rows);
    if (c->feeder) return fail(BF_ERR_STATE, "bf_dm_stream_attach_conditioner: the conditioner is attached to another DM stage");
    return BF_OK;
}

extern "C" {

void bf_cond_default_options(bf_cond_options* o)
{
    if (!o) return;
    o->baseline_pushes = 8;
    o->zero_dm = 1;
    o->auto_threshold = 0.0;
}

int bf_cond_create(bf_handle* h, int n_freq_total, int max_rows_per_push, const bf_cond_options* o, bf_cond** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h || !o) return fail(BF_ERR_INVALID, "bf_cond_create: NULL argument");
    if (n_freq_total < 1 || max_rows_per_push < 1) return fail(BF_ERR_INVALID, "bf_cond_create: need n_freq_total, max_rows_per_push >= 1");
    if (o->baseline_pushes < 1 || o->baseline_pushes > dsabf::kCondMaxWindow)
        return fail(BF_ERR_INVALID, "bf_cond_create: baseline_pushes must be 1 .. %d, not %d", dsabf::kCondMaxWindow, o->baseline_pushes);
    if (!(o->auto_threshold >= 0.0)) return fail(BF_ERR_INVALID, "bf_cond_create: auto_threshold must be >= 0 (0: no automatic mask), not negative or NaN");
    ON_DEVICE(h);
    bf_cond* c = new (std::nothrow) bf_cond();
    if (!c) return fail(BF_ERR_DEVICE, "out of host memory");
    c->h = h;
    c->n_freq = n_freq_total;
    c->n_beams = h->cfg.n_beams;
    c->max_rows = max_rows_per_push;
    c->window = o->baseline_pushes;
    c->zero_dm = o->zero_dm != 0;
    c->k_auto = o->auto_threshold * 1.4826;
    const size_t F = (size_t)n_freq_total, cells = F * c->n_beams;
    const size_t n_seg = ((size_t)max_rows_per_push + dsabf::kCondSegment - 1) / dsabf::kCondSegment;
    bf_resources& res = c->res;
    res.dev(&c->buf.ring, (size_t)c->window * cells * sizeof(dsabf::CondStat));
    res.dev(&c->buf.cell_mu, cells * sizeof(double));
    res.dev(&c->buf.cell_var, cells * sizeof(double));
    res.dev(&c->buf.seg, n_seg * cells * sizeof(dsabf::CondStat));
    res.dev(&c->buf.mr32, cells * sizeof(float2));
    for (double** p : {&c->buf.cm, &c->buf.cv, &c->buf.q, &c->buf.dev}) res.dev(p, F * sizeof(double));
    res.dev(&c->d_static, F, true);
    res.dev(&c->buf.mask, (F + 3) / 4 * 4, true);   // (whole dwords: a host mirror may copy it as such)
    res.dev(&c->buf.params, sizeof(dsabf::CondParams));
    c->pushes.create(res);
    res.device_sync();
    c->buf.static_mask = c->d_static;
    if (int rc = stage_adopt(c, "bf_cond_create")) return rc;
    *out = c;
    return BF_OK;
}

int bf_cond_destroy(bf_cond* c) { return stage_destroy(c); }

int bf_cond_set_mask(bf_cond* c, const uint8_t* host_mask)
{
    if (!c || !host_mask) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = orphaned(c)) return rc;
    bf_handle* h = c->h;
    ON_DEVICE(h);
    // the push in flight still reads the old mask: wait for it, then copy (a blocking call: masks change rarely)
    if (c->pushes.end) HIP_TRY(hipEventSynchronize(c->pushes.end));
    HIP_TRY(hipMemcpy(c->d_static, host_mask, (size_t)c->n_freq, hipMemcpyHostToDevice));
    return BF_OK;
}

int bf_cond_push(bf_cond* c, float* d_rows, int n_rows, void* hip_stream)
{
    if (!c || !d_rows) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_rows < 1 || n_rows > c->max_rows) return fail(BF_ERR_INVALID, "n_rows must be 1 .. %d (max_rows_per_push)", c->max_rows);
    if (int rc = orphaned(c)) return rc;
    bf_handle* h = c->h;
    ON_DEVICE(h);
    hipStream_t q = as_stream(hip_stream);
    // behind the push before this one, whatever queue it ran on: the window, the scratch and the mask are shared
    HIP_TRY(c->pushes.wait(q));
    const int n_sets = (int)std::min<size_t>(c->rows_in_window.size() + 1, (size_t)c->window);
    uint64_t n_window = (uint64_t)n_rows;
    for (size_t i = c->rows_in_window.size() + 1 - (size_t)n_sets; i < c->rows_in_window.size(); i++) n_window += (uint64_t)c->rows_in_window[i];
    HIP_TRY(dsabf::launch_cond_push(d_rows, n_rows, c->n_freq, c->n_beams, c->buf, c->window, (int)(c->pushes.n % (uint64_t)c->window), n_sets, n_window,
                                    c->zero_dm, c->k_auto, q));
    HIP_TRY(c->pushes.extend(q));
    c->rows_in_window.push_back(n_rows);
    while (c->rows_in_window.size() > (size_t)c->window) c->rows_in_window.pop_front();
    return BF_OK;
}

int bf_cond_mask_device(bf_cond* c, const uint8_t** d_mask)
{
    if (!c || !d_mask) return fail(BF_ERR_INVALID, "NULL argument");
    *d_mask = nullptr;
    if (int rc = orphaned(c)) return rc;
    *d_mask = c->buf.mask;
    return BF_OK;
}

}  // extern "C"
