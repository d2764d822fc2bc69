// bf_corr.cpp -- the correlator (include/dsabf.h: bf_correlate_device, bf_corr_*; contract and measurements: docs/CORRELATOR.md).
// The device code is csrc/corr/bf_corr.hip; this file checks the bounds and launches.  The stage is an accumulator stage
// (bf_accum.cpp owns the accumulator and orders its pushes and dumps): what makes it the correlator is the table at the end.
#include "bf_runtime_internal.h"
#include "corr/bf_corr_kernels.h"

// The bounds of one launch (include/dsabf.h): n_ant <= 256, fewer than 2^24 columns per polarisation.
static int check_launch(const bf_handle* h, int n_units, const char* who)
{
    if (n_units <= 0) return fail(BF_ERR_INVALID, "%s: n_units must be positive", who);
    if (h->cfg.n_ant > dsabf::kCorrMaxAnt)
        return fail(BF_ERR_INVALID, "%s: %d antennas; the correlator is defined up to %d (the output grows as n_ant^2)", who, h->cfg.n_ant,
                    dsabf::kCorrMaxAnt);
    const long long n = (long long)n_units * h->cfg.n_out_per_gemm * h->cfg.n_avg;
    if (n > dsabf::kCorrMaxColumns)
        return fail(BF_ERR_INVALID, "%s: %lld columns per polarisation in one call; the sums of a call are exact below 2^24 (128 * N <= 2^31 - 1)",
                    who, n);
    return BF_OK;
}

static int launch(bf_handle* h, const void* d_packed, int n_units, long long* d_vis, bool accumulate, hipStream_t q)
{
    HIP_TRY(dsabf::launch_correlate(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_pol, h->cfg.n_out_per_gemm * h->cfg.n_avg, d_packed, n_units, d_vis,
                                    accumulate, q));
    return BF_OK;
}

extern "C" {

size_t bf_corr_entries(const bf_config* cfg)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_pol <= 0 || cfg->n_ant <= 0) return 0;
    return (size_t)cfg->n_freq * (size_t)cfg->n_pol * dsabf::corr_baselines(cfg->n_ant);
}

int bf_correlate_device(bf_handle* h, const void* d_packed, int n_units, int64_t* d_vis, int accumulate, void* hip_stream)
{
    if (!h || !d_packed || !d_vis) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_launch(h, n_units, "bf_correlate_device")) return rc;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_vis & 7))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned, d_vis 8-byte aligned");
    ON_DEVICE(h);
    return launch(h, d_packed, n_units, (long long*)d_vis, accumulate != 0, as_stream(hip_stream));
}

}  // extern "C"

// bf_corr_create looks at the antennas only: the columns of a launch are a push's matter.
static int check_create(const bf_handle* h)
{
    if (h->cfg.n_ant > dsabf::kCorrMaxAnt)
        return fail(BF_ERR_INVALID, "bf_corr_create: %d antennas; the correlator is defined up to %d", h->cfg.n_ant, dsabf::kCorrMaxAnt);
    return BF_OK;
}

static const bf_accum_kind kCorrStage = {"correlator stage", "bf_corr", bf_corr_entries, check_create, check_launch, launch};

// The stage (bf_accum.cpp): its accumulator holds the visibilities.
struct bf_corr : bf_accum_stage {
    bf_corr() : bf_accum_stage(kCorrStage) {}
};

extern "C" {

int bf_corr_create(bf_handle* h, int max_in_flight, bf_corr** out) { return accum_create(h, max_in_flight, out); }
int bf_corr_destroy(bf_corr* c) { return stage_destroy(c); }
int bf_corr_pending(const bf_corr* c) { return accum_pending(c); }
int bf_corr_push(bf_corr* c, const void* d_packed, int n_units, void* hip_stream) { return accum_push(c, d_packed, n_units, hip_stream); }
int bf_corr_push_block(bf_corr* c, int stream_idx, int slot, int first_unit, int n_units) { return accum_push_block(c, stream_idx, slot, first_unit, n_units); }
int bf_corr_dump(bf_corr* c, void*) { return accum_dump(c); }
int bf_corr_collect(bf_corr* c, int64_t* out, uint64_t* n_columns_per_pol) { return accum_collect(c, out, n_columns_per_pol); }

}  // extern "C"
