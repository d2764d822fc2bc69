// bf_rm.cpp -- Faraday synthesis of Stokes beams (include/dsabf.h: bf_rm_*; contract and measurements: docs/FARADAY.md).
// The device code is csrc/rm/bf_rm.hip; this file checks the bounds, owns a stage's tables, orders the upload of a new table against
// the kernels in flight (a bf_chain: bf_runtime_internal.h), and holds the host helpers (lambda^2, resolution, table, RMSF, the fit of a peak record).
#include <cmath>
#include <new>
#include <vector>

#include "bf_runtime_internal.h"
#include "rm/bf_rm_kernels.h"

struct bf_rm : bf_stage {
    bf_rm() : bf_stage("Faraday synthesis stage") {}
    int n_chan = 0, n_phi = 0;
    float* d_table = nullptr;   // the MFMA operands, dsabf::rm_permute_table_host (ONE copy: an upload waits for the kernels in flight)
    float* d_wn = nullptr;      // [chan]
    float* h_table = nullptr;   // pinned: the table, then wn
    hipStream_t copy_q = nullptr;
    hipEvent_t uploaded = nullptr;               // end of the last upload: every kernel waits for it
    bf_chain kernels;                            // its end fires when EVERY kernel issued so far has run (each joins the one before it)
};

static const double kLight = 0.299792458;   // m GHz

static int upload(bf_rm* s, const float* rot, const float* wn)
{
    const size_t floats = dsabf::rm_table_floats(s->n_chan, s->n_phi);
    dsabf::rm_permute_table_host(rot, s->n_chan, s->n_phi, s->h_table);
    for (int c = 0; c < s->n_chan; c++) s->h_table[floats + c] = wn[c];
    HIP_TRY(s->kernels.wait(s->copy_q));
    HIP_TRY(hipMemcpyAsync(s->d_table, s->h_table, floats * sizeof(float), hipMemcpyHostToDevice, s->copy_q));
    HIP_TRY(hipMemcpyAsync(s->d_wn, s->h_table + floats, (size_t)s->n_chan * sizeof(float), hipMemcpyHostToDevice, s->copy_q));
    HIP_TRY(hipEventRecord(s->uploaded, s->copy_q));
    HIP_TRY(hipEventSynchronize(s->uploaded));
    return BF_OK;
}

// What the helpers share: the weights must be >= 0 and finite with a positive sum, the frequencies positive.
static int check_channels(const char* who, const double* freq_ghz, const double* w, int n_chan, double* wsum)
{
    if (!freq_ghz || !w) return fail(BF_ERR_INVALID, "%s: NULL argument", who);
    if (n_chan < 1 || n_chan > dsabf::kRmMaxChan) return fail(BF_ERR_INVALID, "%s: n_chan = %d; 1 ... %d channels", who, n_chan, dsabf::kRmMaxChan);
    double sum = 0.0;
    for (int c = 0; c < n_chan; c++) {
        if (!(freq_ghz[c] > 0.0) || !std::isfinite(freq_ghz[c])) return fail(BF_ERR_INVALID, "%s: the frequency of channel %d is not positive", who, c);
        if (!(w[c] >= 0.0) || !std::isfinite(w[c])) return fail(BF_ERR_INVALID, "%s: the weight of channel %d is negative or not finite", who, c);
        sum += w[c];
    }
    if (!(sum > 0.0)) return fail(BF_ERR_INVALID, "%s: every channel is masked", who);
    *wsum = sum;
    return BF_OK;
}

static int check_grid(const char* who, double phi0, double dphi, int n_phi)
{
    if (n_phi < 1 || n_phi > dsabf::kRmMaxPhi) return fail(BF_ERR_INVALID, "%s: n_phi = %d; 1 ... %d depths", who, n_phi, dsabf::kRmMaxPhi);
    if (!std::isfinite(phi0) || !std::isfinite(dphi)) return fail(BF_ERR_INVALID, "%s: the grid is not finite", who);
    return BF_OK;
}

static double lambda0_2(const double* freq_ghz, const double* w, int n_chan, double wsum)
{
    double l0 = 0.0;
    for (int c = 0; c < n_chan; c++) l0 += w[c] * bf_rm_lambda2(freq_ghz[c]);
    return l0 / wsum;
}

extern "C" {

double bf_rm_lambda2(double f_ghz) { return (kLight / f_ghz) * (kLight / f_ghz); }

int bf_rm_resolution(const double* freq_ghz, const double* w, int n_chan, double* fwhm, double* phi_max)
{
    double wsum;
    if (int rc = check_channels("bf_rm_resolution", freq_ghz, w, n_chan, &wsum)) return rc;
    if (!fwhm || !phi_max) return fail(BF_ERR_INVALID, "bf_rm_resolution: NULL argument");
    double lo = 0.0, hi = 0.0, step = 0.0;
    bool any = false;
    for (int c = 0; c < n_chan; c++) {
        const double l2 = bf_rm_lambda2(freq_ghz[c]);
        if (c > 0 && std::fabs(l2 - bf_rm_lambda2(freq_ghz[c - 1])) > step) step = std::fabs(l2 - bf_rm_lambda2(freq_ghz[c - 1]));
        if (w[c] > 0.0) {
            lo = any && lo < l2 ? lo : l2;
            hi = any && hi > l2 ? hi : l2;
            any = true;
        }
    }
    if (!(hi > lo) || !(step > 0.0)) return fail(BF_ERR_INVALID, "bf_rm_resolution: the unmasked channels span no range of lambda^2");
    *fwhm = 2.0 * std::sqrt(3.0) / (hi - lo);
    *phi_max = std::sqrt(3.0) / step;
    return BF_OK;
}

int bf_rm_table(const double* freq_ghz, const double* w, int n_chan, double phi0, double dphi, int n_phi, float* rot, float* wn, double* lambda0_2_out)
{
    double wsum;
    if (int rc = check_channels("bf_rm_table", freq_ghz, w, n_chan, &wsum)) return rc;
    if (int rc = check_grid("bf_rm_table", phi0, dphi, n_phi)) return rc;
    if (!rot || !wn) return fail(BF_ERR_INVALID, "bf_rm_table: NULL argument");
    const double l0 = lambda0_2(freq_ghz, w, n_chan, wsum);
    for (int c = 0; c < n_chan; c++) wn[c] = (float)(w[c] / wsum);
    for (int p = 0; p < n_phi; p++) {
        const double phi = phi0 + p * dphi;
        for (int c = 0; c < n_chan; c++) {
            const double a = 2.0 * phi * (bf_rm_lambda2(freq_ghz[c]) - l0), wc = w[c] / wsum;
            rot[((size_t)p * n_chan + c) * 2] = (float)(wc * std::cos(a));
            rot[((size_t)p * n_chan + c) * 2 + 1] = (float)(wc * -std::sin(a));
        }
    }
    if (lambda0_2_out) *lambda0_2_out = l0;
    return BF_OK;
}

int bf_rm_rmsf(const double* freq_ghz, const double* w, int n_chan, double phi0, double dphi, int n_phi, double* out)
{
    double wsum;
    if (int rc = check_channels("bf_rm_rmsf", freq_ghz, w, n_chan, &wsum)) return rc;
    if (int rc = check_grid("bf_rm_rmsf", phi0, dphi, n_phi)) return rc;
    if (!out) return fail(BF_ERR_INVALID, "bf_rm_rmsf: NULL argument");
    const double l0 = lambda0_2(freq_ghz, w, n_chan, wsum);
    for (int p = 0; p < n_phi; p++) {
        const double phi = phi0 + p * dphi;
        double re = 0.0, im = 0.0;
        for (int c = 0; c < n_chan; c++) {
            const double a = 2.0 * phi * (bf_rm_lambda2(freq_ghz[c]) - l0);
            re += w[c] / wsum * std::cos(a);
            im -= w[c] / wsum * std::sin(a);
        }
        out[2 * p] = re;
        out[2 * p + 1] = im;
    }
    return BF_OK;
}

int bf_rm_refine(const bf_rm_peak* peaks, size_t n, double phi0, double dphi, int n_phi, double lambda0_2_in, bf_rm_fit* fits)
{
    if (!peaks || !fits) return fail(BF_ERR_INVALID, "bf_rm_refine: NULL argument");
    if (int rc = check_grid("bf_rm_refine", phi0, dphi, n_phi)) return rc;
    const double pi = 3.14159265358979323846;
    for (size_t i = 0; i < n; i++) {
        const bf_rm_peak& k = peaks[i];
        if (k.p < 0 || k.p >= n_phi) return fail(BF_ERR_INVALID, "bf_rm_refine: record %zu has depth index %d outside the grid of %d", i, k.p, n_phi);
        const double lo = k.pow_lo, pk = k.pow_pk, hi = k.pow_hi, den = lo - 2.0 * pk + hi;
        const double delta = k.p == 0 || k.p == n_phi - 1 || den == 0.0 ? 0.0 : 0.5 * (lo - hi) / den;
        bf_rm_fit& f = fits[i];
        f.rm = phi0 + (k.p + delta) * dphi;
        double pa = 0.5 * std::atan2((double)k.im, (double)k.re) - f.rm * lambda0_2_in;
        pa -= pi * std::floor((pa + pi / 2.0) / pi);   // into [-pi/2, pi/2)
        if (pa >= pi / 2.0) pa -= pi;
        if (pa < -pi / 2.0) pa += pi;
        f.pa = pa;
        f.lin = std::sqrt(pk);
        f.frac = k.isum > 0.f ? f.lin / (double)k.isum : 0.0;
    }
    return BF_OK;
}

int bf_rm_create(bf_handle* h, int n_chan, int n_phi, const float* rot, const float* wn, bf_rm** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h) return fail(BF_ERR_INVALID, "bf_rm_create: the handle is NULL");
    if (!rot || !wn) return fail(BF_ERR_INVALID, "bf_rm_create: the table is NULL");
    if (n_chan < 1 || n_chan > dsabf::kRmMaxChan) return fail(BF_ERR_INVALID, "bf_rm_create: n_chan = %d; 1 ... %d channels", n_chan, dsabf::kRmMaxChan);
    if (n_phi < 1 || n_phi > dsabf::kRmMaxPhi) return fail(BF_ERR_INVALID, "bf_rm_create: n_phi = %d; 1 ... %d depths", n_phi, dsabf::kRmMaxPhi);
    ON_DEVICE(h);
    bf_rm* s = new (std::nothrow) bf_rm();
    if (!s) return fail(BF_ERR_DEVICE, "out of host memory");
    s->h = h;
    s->n_chan = n_chan;
    s->n_phi = n_phi;
    const size_t floats = dsabf::rm_table_floats(n_chan, n_phi);
    bf_resources& res = s->res;
    res.dev(&s->d_table, floats * sizeof(float));
    res.dev(&s->d_wn, (size_t)n_chan * sizeof(float));
    res.host(&s->h_table, (floats + n_chan) * sizeof(float));
    res.queue(&s->copy_q);
    res.event(&s->uploaded);
    s->kernels.create(res);
    if (int rc = stage_adopt(s, "bf_rm_create")) return rc;
    if (int rc = upload(s, rot, wn)) {
        stage_destroy(s);
        return rc;
    }
    *out = s;
    return BF_OK;
}

int bf_rm_destroy(bf_rm* s) { return stage_destroy(s); }

int bf_rm_set_table(bf_rm* s, const float* rot, const float* wn)
{
    if (!s || !rot || !wn) return fail(BF_ERR_INVALID, "bf_rm_set_table: NULL argument");
    if (int rc = orphaned(s)) return rc;
    ON_DEVICE(s->h);
    return upload(s, rot, wn);
}

int bf_rm_device(bf_rm* s, const void* d_stokes, int K, int64_t n_rows, const void* d_base, void* d_spec, void* d_peaks, void* hip_stream)
{
    const char* who = "bf_rm_device";
    if (!s || !d_stokes) return fail(BF_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = orphaned(s)) return rc;
    if (!d_spec && !d_peaks) return fail(BF_ERR_INVALID, "%s: d_spec and d_peaks are both NULL; at least one output", who);
    if (K < 1) return fail(BF_ERR_INVALID, "%s: K = %d beams; at least one", who, K);
    if (n_rows < 1 || n_rows > 0x7fffffffLL || n_rows * K > 0x7fffffffLL)
        return fail(BF_ERR_INVALID, "%s: n_rows = %lld with K = %d; at least one row and n_rows K < 2^31", who, (long long)n_rows, K);
    if (((uintptr_t)d_stokes & 7) || ((uintptr_t)d_base & 7) || ((uintptr_t)d_spec & 7) || ((uintptr_t)d_peaks & 7))
        return fail(BF_ERR_INVALID, "%s: misaligned device pointer: d_stokes, d_base, d_spec and d_peaks must be 8-byte aligned", who);
    ON_DEVICE(s->h);
    hipStream_t q = as_stream(hip_stream);
    HIP_TRY(hipStreamWaitEvent(q, s->uploaded, 0));
    dsabf::RmLaunch l = {d_stokes, d_base, s->d_table, s->d_wn, d_spec, d_peaks, s->n_chan, s->n_phi, K, (int)n_rows};
    HIP_TRY(dsabf::launch_rm(l, q));
    // one chain for all launches: behind this kernel the queue joins the launch before it (the kernel itself is not held up)
    HIP_TRY(s->kernels.join(q));
    return BF_OK;
}

}  // extern "C"
