// bf_sk.cpp -- voltage moments and spectral kurtosis (include/dsabf.h: bf_sk_device, bf_sk_select, bf_sk_*; contract and
// measurements: docs/SPECTRAL_KURTOSIS.md).  The device code is csrc/sk/bf_sk.hip; this file checks the bounds, launches, and holds the
// host rule that turns moments into flags.  The stage is an accumulator stage (bf_accum.cpp owns the accumulator and orders its pushes
// and dumps): what makes it the moments stage is the table at the end.
#include <cmath>

#include "bf_runtime_internal.h"
#include "sk/bf_sk_kernels.h"

// The bounds of one launch (include/dsabf.h): n_ant <= 2048, n_pol <= 64, fewer than 2^24 columns per polarisation.
static int check_launch(const bf_handle* h, int n_units, const char* who)
{
    if (n_units <= 0) return fail(BF_ERR_INVALID, "%s: n_units must be positive", who);
    if (h->cfg.n_ant > dsabf::kSkMaxAnt || h->cfg.n_ant % 4)
        return fail(BF_ERR_INVALID, "%s: %d antennas; the moments are defined for a multiple of 4 up to %d", who, h->cfg.n_ant, dsabf::kSkMaxAnt);
    if (h->cfg.n_pol > dsabf::kSkMaxPol)
        return fail(BF_ERR_INVALID, "%s: %d polarisations; the moments are defined up to %d", who, h->cfg.n_pol, dsabf::kSkMaxPol);
    const long long n = (long long)n_units * h->cfg.n_out_per_gemm * h->cfg.n_avg;
    if (n > dsabf::kSkMaxColumns)
        return fail(BF_ERR_INVALID, "%s: %lld columns per polarisation in one call; a call is defined below 2^24 (M1 <= 128 * N fits int32)", who, n);
    return BF_OK;
}

static int launch(bf_handle* h, const void* d_packed, int n_units, long long* d_mom, bool accumulate, hipStream_t q)
{
    HIP_TRY(dsabf::launch_moments(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_pol, h->cfg.n_out_per_gemm * h->cfg.n_avg, d_packed, n_units, d_mom,
                                  accumulate, h->n_cus, q));
    return BF_OK;
}

extern "C" {

size_t bf_sk_entries(const bf_config* cfg)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_pol <= 0 || cfg->n_ant <= 0) return 0;
    return (size_t)cfg->n_freq * (size_t)cfg->n_pol * (size_t)cfg->n_ant;
}

int bf_sk_default_options(bf_sk_options* o)
{
    if (!o) return fail(BF_ERR_INVALID, "NULL argument");
    o->centre = 1.0;
    o->n_sigma = 5.0;
    o->max_bad_fraction_ant = 0.5;
    o->max_bad_fraction_chan = 0.5;
    return BF_OK;
}

// Host arithmetic in fp64, one rounding per operation (the library is built with -ffp-contract=off), in the order of include/dsabf.h.
int bf_sk_select(const int64_t* moments, uint64_t n_columns_per_pol, int n_freq, int n_pol, int n_ant, const bf_sk_options* opt, double* sk,
                 uint8_t* cell, uint8_t* ant_flags, uint8_t* chan_flags)
{
    if (!moments) return fail(BF_ERR_INVALID, "bf_sk_select: moments is NULL");
    if (n_columns_per_pol < 2) return fail(BF_ERR_INVALID, "bf_sk_select: the estimator needs at least 2 columns per polarisation");
    if (n_freq <= 0 || n_pol <= 0 || n_ant <= 0) return fail(BF_ERR_INVALID, "bf_sk_select: n_freq, n_pol and n_ant must be positive");
    bf_sk_options o;
    bf_sk_default_options(&o);
    if (opt) o = *opt;
    const double M = (double)n_columns_per_pol;
    const double scale = (double)(n_columns_per_pol + 1) / (double)(n_columns_per_pol - 1);
    const double half_width = o.n_sigma * 2.0 / std::sqrt(M);
    const double lo = o.centre - half_width, hi = o.centre + half_width;
    const size_t layers = (size_t)n_freq * (size_t)n_pol, n_cells = layers * (size_t)n_ant;
    std::vector<uint8_t> code(n_cells), bad_ant((size_t)n_ant);
    std::vector<size_t> bad((size_t)n_ant, 0);
    for (size_t l = 0; l < layers; l++)
        for (int a = 0; a < n_ant; a++) {
            const size_t i = l * (size_t)n_ant + (size_t)a;
            const int64_t m1 = moments[2 * i], m2 = moments[2 * i + 1];
            double v = 0.0;
            uint8_t c = 0;
            if (m1 == 0) {
                c = BF_SK_DEAD;
            } else {
                const double r = (M * (double)m2) / ((double)m1 * (double)m1);
                v = scale * (r - 1.0);
                if (v < lo) c |= BF_SK_LOW;
                if (v > hi) c |= BF_SK_HIGH;
            }
            code[i] = c;
            if (sk) sk[i] = v;
            if (cell) cell[i] = c;
            if (c) bad[(size_t)a]++;
        }
    int n_good = 0;
    for (int a = 0; a < n_ant; a++) {
        bad_ant[(size_t)a] = (double)bad[(size_t)a] > o.max_bad_fraction_ant * (double)layers ? 1 : 0;
        if (!bad_ant[(size_t)a]) n_good++;
        if (ant_flags) ant_flags[a] = bad_ant[(size_t)a];
    }
    if (chan_flags)
        for (int f = 0; f < n_freq; f++) {
            size_t bad_f = 0;
            for (int p = 0; p < n_pol; p++)
                for (int a = 0; a < n_ant; a++)
                    if (!bad_ant[(size_t)a] && code[((size_t)f * (size_t)n_pol + (size_t)p) * (size_t)n_ant + (size_t)a]) bad_f++;
            chan_flags[f] = (n_good == 0 || (double)bad_f > o.max_bad_fraction_chan * (double)((size_t)n_good * (size_t)n_pol)) ? 1 : 0;
        }
    return BF_OK;
}

int bf_sk_device(bf_handle* h, const void* d_packed, int n_units, int64_t* d_moments, int accumulate, void* hip_stream)
{
    if (!h || !d_packed || !d_moments) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_launch(h, n_units, "bf_sk_device")) return rc;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_moments & 7))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned, d_moments 8-byte aligned");
    ON_DEVICE(h);
    return launch(h, d_packed, n_units, (long long*)d_moments, accumulate != 0, as_stream(hip_stream));
}

}  // extern "C"

static int check_create(const bf_handle* h) { return check_launch(h, 1, "bf_sk_create"); }

static const bf_accum_kind kSkStage = {"moments stage", "bf_sk", bf_sk_entries, check_create, check_launch, launch};

// The stage (bf_accum.cpp): its accumulator holds the moments.
struct bf_sk : bf_accum_stage {
    bf_sk() : bf_accum_stage(kSkStage) {}
};

extern "C" {

int bf_sk_create(bf_handle* h, int max_in_flight, bf_sk** out) { return accum_create(h, max_in_flight, out); }
int bf_sk_destroy(bf_sk* c) { return stage_destroy(c); }
int bf_sk_pending(const bf_sk* c) { return accum_pending(c); }
int bf_sk_push(bf_sk* c, const void* d_packed, int n_units, void* hip_stream) { return accum_push(c, d_packed, n_units, hip_stream); }
int bf_sk_push_block(bf_sk* c, int stream_idx, int slot, int first_unit, int n_units) { return accum_push_block(c, stream_idx, slot, first_unit, n_units); }
int bf_sk_dump(bf_sk* c, void*) { return accum_dump(c); }
int bf_sk_collect(bf_sk* c, int64_t* out, uint64_t* n_columns_per_pol) { return accum_collect(c, out, n_columns_per_pol); }

}  // extern "C"
