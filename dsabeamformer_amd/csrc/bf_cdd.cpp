// bf_cdd.cpp -- coherent dedispersion of beam voltages (include/dsabf.h: bf_cdd_*; contract and measurements:
// docs/COHERENT_DEDISPERSION.md).  The device code is csrc/cdd/bf_cdd.hip; this file checks the bounds, owns a stage's twiddle and
// chirp tables, orders the uploads of a new chirp against the kernels in flight (a bf_chain: bf_runtime_internal.h), and holds the host helpers (sweep, edge, chirp).
#include <cmath>
#include <new>

#include "bf_runtime_internal.h"
#include "cdd/bf_cdd_kernels.h"

struct bf_cdd : bf_stage {
    bf_cdd() : bf_stage("coherent dedispersion stage") {}
    int n_chan = 0, n_fft = 0, n_edge = 0;
    float* d_tw = nullptr;      // n_fft / 2 twiddles {cos, -sin}
    float* d_chirp = nullptr;   // [chan][n_fft]{re, im}, rows bit-reversed (ONE copy: an upload waits for the kernels in flight)
    float* h_chirp = nullptr;   // pinned: where bf_cdd_set_chirp builds the rows (free again when that call returns)
    hipStream_t copy_q = nullptr;
    hipEvent_t uploaded = nullptr;               // end of the last upload: every kernel waits for it
    bf_chain kernels;                            // its end fires when EVERY kernel issued so far has run (each joins the one before it)
};

static const double kDispersion = 4.15;   // ms GHz^2 per pc cm^-3: the constant of dm_delays (bf_geometry.cpp)

static int upload(bf_cdd* c, const float* chirp)
{
    const size_t row = (size_t)c->n_fft * 2;
    for (int f = 0; f < c->n_chan; f++) dsabf::cdd_permute_row_host(chirp + f * row, c->n_fft, c->h_chirp + f * row);
    HIP_TRY(c->kernels.wait(c->copy_q));
    HIP_TRY(hipMemcpyAsync(c->d_chirp, c->h_chirp, (size_t)c->n_chan * row * sizeof(float), hipMemcpyHostToDevice, c->copy_q));
    HIP_TRY(hipEventRecord(c->uploaded, c->copy_q));
    HIP_TRY(hipEventSynchronize(c->uploaded));
    return BF_OK;
}

// Both entry points: n_int 0 is the voltage output.
static int run(bf_cdd* c, const void* d_in, int K, long long n_time64, int n_int, void* d_out, void* hip_stream, const char* who)
{
    if (!c || !d_in || !d_out) return fail(BF_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = orphaned(c)) return rc;
    if (K < 1) return fail(BF_ERR_INVALID, "%s: K = %d beams; at least one", who, K);
    if (n_time64 < 1 || n_time64 > 0x7fffffffLL) return fail(BF_ERR_INVALID, "%s: n_time = %lld; 1 ... 2^31 - 1 samples", who, n_time64);
    const int n_time = (int)n_time64;
    const int V = c->n_fft - 2 * c->n_edge;
    if (n_int && (n_int < 1 || V % n_int || n_time % n_int))
        return fail(BF_ERR_INVALID, "%s: n_int %d does not divide both the %d valid samples of a segment and n_time %d", who, n_int, V, n_time);
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return fail(BF_ERR_INVALID, "%s: misaligned device pointer: d_in and d_out must be 8-byte aligned", who);
    const long long groups = dsabf::cdd_segments(n_time, c->n_fft, c->n_edge) * c->n_chan * K;
    if (groups > 0x7fffffffLL)
        return fail(BF_ERR_INVALID, "%s: %lld segments x %d channels x %d beams overflow the grid (2^31 - 1 workgroups)", who,
                    dsabf::cdd_segments(n_time, c->n_fft, c->n_edge), c->n_chan, K);
    ON_DEVICE(c->h);
    hipStream_t q = as_stream(hip_stream);
    HIP_TRY(hipStreamWaitEvent(q, c->uploaded, 0));
    dsabf::CddLaunch l = {d_in, d_out, c->d_tw, c->d_chirp, c->n_chan, K, n_time, c->n_fft, c->n_edge, n_int};
    HIP_TRY(dsabf::launch_cdd(l, q));
    // one chain for all launches: behind this kernel the queue joins the launch before it (the kernel itself is not held up)
    HIP_TRY(c->kernels.join(q));
    return BF_OK;
}

extern "C" {

double bf_cdd_sweep_samples(double dm, double f_ghz, double bw_mhz)
{
    const double lo = f_ghz - bw_mhz / 2000.0, hi = f_ghz + bw_mhz / 2000.0;
    return kDispersion * 1e3 * dm * (1.0 / (lo * lo) - 1.0 / (hi * hi)) * bw_mhz;
}

int bf_cdd_edge(double dm, const double* freq_ghz, int n_chan, double bw_mhz)
{
    if (!freq_ghz) return fail(BF_ERR_INVALID, "bf_cdd_edge: freq_ghz is NULL");
    if (n_chan < 1) return fail(BF_ERR_INVALID, "bf_cdd_edge: n_chan must be positive");
    double most = 0.0;
    for (int f = 0; f < n_chan; f++) {
        const double s = std::ceil(bf_cdd_sweep_samples(dm, freq_ghz[f], bw_mhz));
        if (!(s < 1e9)) return fail(BF_ERR_INVALID, "bf_cdd_edge: the sweep of channel %d is not a usable number of samples", f);
        if (s > most) most = s;
    }
    return (int)most;
}

int bf_cdd_chirp(double dm, const double* freq_ghz, int n_chan, double bw_mhz, int sideband, int n_fft, float* out)
{
    if (!freq_ghz || !out) return fail(BF_ERR_INVALID, "bf_cdd_chirp: NULL argument");
    if (n_chan < 1) return fail(BF_ERR_INVALID, "bf_cdd_chirp: n_chan must be positive");
    if (sideband != 1 && sideband != -1) return fail(BF_ERR_INVALID, "bf_cdd_chirp: sideband is +1 or -1, not %d", sideband);
    if (dsabf::cdd_log2(n_fft) < 0) return fail(BF_ERR_INVALID, "bf_cdd_chirp: n_fft %d is not a power of two in 64 ... 4096", n_fft);
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int f = 0; f < n_chan; f++) {
        const double F = 1000.0 * freq_ghz[f];
        for (int j = 0; j < n_fft; j++) {
            const double nu = sideband * (double)(j < n_fft / 2 ? j : j - n_fft) * bw_mhz / n_fft;
            const double phi = two_pi * kDispersion * 1e9 * dm * nu * nu / (F * F * (F + nu));
            out[((size_t)f * n_fft + j) * 2] = (float)(std::cos(phi) / n_fft);
            out[((size_t)f * n_fft + j) * 2 + 1] = (float)(std::sin(phi) / n_fft);
        }
    }
    return BF_OK;
}

int bf_cdd_create(bf_handle* h, int n_chan, int n_fft, int n_edge, const float* chirp, bf_cdd** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!h) return fail(BF_ERR_INVALID, "bf_cdd_create: the handle is NULL");
    if (!chirp) return fail(BF_ERR_INVALID, "bf_cdd_create: chirp is NULL");
    if (n_chan < 1) return fail(BF_ERR_INVALID, "bf_cdd_create: n_chan must be positive");
    if (dsabf::cdd_log2(n_fft) < 0) return fail(BF_ERR_INVALID, "bf_cdd_create: n_fft %d is not a power of two in 64 ... 4096", n_fft);
    if (n_edge < 0 || n_edge > n_fft / 4) return fail(BF_ERR_INVALID, "bf_cdd_create: n_edge %d is outside 0 ... n_fft / 4 = %d", n_edge, n_fft / 4);
    if ((long long)n_chan * n_fft > (1LL << 28)) return fail(BF_ERR_INVALID, "bf_cdd_create: a chirp table of %d channels x %d bins is beyond 2^28 entries", n_chan, n_fft);
    ON_DEVICE(h);
    bf_cdd* c = new (std::nothrow) bf_cdd();
    if (!c) return fail(BF_ERR_DEVICE, "out of host memory");
    c->h = h;
    c->n_chan = n_chan;
    c->n_fft = n_fft;
    c->n_edge = n_edge;
    const size_t table = (size_t)n_chan * n_fft * 2 * sizeof(float);
    bf_resources& res = c->res;
    res.dev(&c->d_tw, (size_t)n_fft * sizeof(float));
    res.dev(&c->d_chirp, table);
    res.host(&c->h_chirp, table > (size_t)n_fft * sizeof(float) ? table : (size_t)n_fft * sizeof(float));
    res.queue(&c->copy_q);
    res.event(&c->uploaded);
    c->kernels.create(res);
    if (int rc = stage_adopt(c, "bf_cdd_create")) return rc;
    auto fill = [&]() -> int {
        dsabf::cdd_twiddles_host(n_fft, c->h_chirp);   // (through the pinned buffer, before the chirp takes it)
        HIP_TRY(hipMemcpyAsync(c->d_tw, c->h_chirp, (size_t)n_fft * sizeof(float), hipMemcpyHostToDevice, c->copy_q));
        HIP_TRY(hipStreamSynchronize(c->copy_q));
        return upload(c, chirp);
    };
    if (int rc = fill()) {
        stage_destroy(c);
        return rc;
    }
    *out = c;
    return BF_OK;
}

int bf_cdd_destroy(bf_cdd* c) { return stage_destroy(c); }

int bf_cdd_set_chirp(bf_cdd* c, const float* chirp)
{
    if (!c || !chirp) return fail(BF_ERR_INVALID, "bf_cdd_set_chirp: NULL argument");
    if (int rc = orphaned(c)) return rc;
    ON_DEVICE(c->h);
    return upload(c, chirp);
}

int bf_cdd_voltages_device(bf_cdd* c, const void* d_in, int K, int64_t n_time, void* d_out, void* hip_stream)
{
    return run(c, d_in, K, n_time, 0, d_out, hip_stream, "bf_cdd_voltages_device");
}

int bf_cdd_stokes_device(bf_cdd* c, const void* d_in, int K, int64_t n_time, int n_int, void* d_out, void* hip_stream)
{
    if (n_int < 1) return fail(BF_ERR_INVALID, "bf_cdd_stokes_device: n_int must be positive");
    return run(c, d_in, K, n_time, n_int, d_out, hip_stream, "bf_cdd_stokes_device");
}

}  // extern "C"
