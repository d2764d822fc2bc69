// bf_cal.hip -- device code of the gain solver (include/dsabf.h: bf_solve_gains_device, bf_calibrate_weights_device; contract:
// docs/CALIBRATION.md).
//
// solve_kernel: StEFCal, one workgroup (8 waves) per problem = one (polarisation layer, channel).  fp64 throughout, one rounding per
// operation (no FMA contraction), every sum in the contract's OSUM order:
//   lane l of a wave owns the columns q = l (mod 64): it adds its (up to four) terms in ascending q onto +0.0, and six butterfly
//   steps (xor 32, 16, 8, 4, 2, 1) are the six halving steps -- lane l < 32 forms s[l] + s[l + 32] as the contract writes it, lane
//   l + 32 the same two numbers in the other order, which is the same double; after six steps every lane holds the one result.
// Wave w owns the rows p = w, w + 8, ...; the gains live in LDS twice (the previous iteration's and the one being written: Jacobi
// updates), one barrier per iteration and a second one on even iterations, behind the convergence test that reads both sets.  Every
// wave forms the test's two sums itself, from the same LDS words in the same order, so the stop decision is workgroup-uniform without
// a broadcast.
// x[p][q], the visibility with the model folded in, comes from load_x() on either storage path:
//   RESIDENT   (n_ant <= 64) the fp64 square is built once in LDS (16 n^2 bytes) -- a wave's row read is 64 consecutive 16-byte words;
//   streamed   the int64 triangle is re-read every iteration (row p below the diagonal, column p above it) and converted and folded on
//              the fly.  No scratch memory, so concurrent solves on any queues share nothing.
// calw_kernel: the elementwise weight correction, one workgroup per (channel, antenna) row of the weight array.
#include "bf_cal_kernels.h"
#include "../rec/bf_launch_record.h"

#pragma clang fp contract(off)

namespace dsabf {

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTerms = kCalMaxAnt / 64;   // terms per lane of one OSUM

struct __attribute__((aligned(16))) cd {
    double re, im;
};
typedef long long v2ll __attribute__((ext_vector_type(2)));

__device__ __forceinline__ cd cmul(cd a, cd b) { return cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// the six halving steps of OSUM on the 64 partial sums of a wave; every lane returns the result
__device__ __forceinline__ double halve(double s)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) s = s + __shfl_xor(s, w, 64);
    return s;
}

struct CalArgs {
    const long long* __restrict__ vis;   // [f][pol][bl]{re, im}, 16-byte aligned
    const cd* __restrict__ model;        // [f][ant] or NULL
    const uint8_t* __restrict__ flags;   // [ant] or NULL
    cd* __restrict__ gains;              // [pol_out][f][ant]
    int32_t* __restrict__ info;          // [pol_out][f]{iterations, status}
    double tol;
    int n_ant, n_freq, n_pol, max_iter, ref_ant, joint;
};

// The integer visibility (a1, a2), a2 <= a1, of this problem: one polarisation's entry, or the int64 sum over all of them.
__device__ __forceinline__ v2ll load_v(const long long* tri, size_t n_bl, int n_sum, int a1, int a2)
{
    const size_t e = (size_t)a1 * (size_t)(a1 + 1) / 2 + (size_t)a2;
    v2ll v = *reinterpret_cast<const v2ll*>(tri + 2 * e);
    for (int k = 1; k < n_sum; k++) v += *reinterpret_cast<const v2ll*>(tri + 2 * (e + (size_t)k * n_bl));
    return v;
}

// x[p][q] of the contract (steps 1 and 2): (0, 0) on the diagonal and for a flagged p or q
__device__ __forceinline__ cd load_x(const long long* tri, size_t n_bl, int n_sum, int p, int q, bool dead, bool fold, cd sp_conj, cd sq)
{
    if (p == q || dead) return cd{0.0, 0.0};
    const v2ll v = q < p ? load_v(tri, n_bl, n_sum, p, q) : load_v(tri, n_bl, n_sum, q, p);
    cd x{(double)v.x, (double)v.y};
    if (q > p) x.im = -x.im;
    if (fold) x = cmul(cmul(x, sp_conj), sq);
    return x;
}

template <bool RESIDENT>
__global__ __launch_bounds__(kThreads) void solve_kernel(CalArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = a.n_ant;
    cd* gbuf = reinterpret_cast<cd*>(smem);                       // [2][n]: the gains, old and new
    cd* sm = gbuf + 2 * n;                                        // [n]: the model's phasors (ones without a model)
    cd* xs = sm + n;                                              // [n][n] (RESIDENT)
    uint8_t* fl = reinterpret_cast<uint8_t*>(xs + (RESIDENT ? n * n : 0));   // [n]

    const int po = blockIdx.x / a.n_freq, f = blockIdx.x - po * a.n_freq;
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const size_t n_bl = (size_t)n * (size_t)(n + 1) / 2;
    const int n_sum = a.joint ? a.n_pol : 1;
    const long long* tri = a.vis + ((size_t)f * a.n_pol + (a.joint ? 0 : po)) * n_bl * 2;
    const bool fold = a.model != nullptr;

    // ---- flags, model, start
    for (int p = tid; p < n; p += kThreads) {
        const bool flagged = a.flags && a.flags[p] != 0;
        fl[p] = flagged ? 1 : 0;
        sm[p] = fold ? a.model[(size_t)f * n + p] : cd{1.0, 0.0};
        const long long d = load_v(tri, n_bl, n_sum, p, p).x;
        gbuf[p] = cd{(!flagged && d > 0) ? sqrt((double)d) : 0.0, 0.0};
    }
    __syncthreads();
    if (RESIDENT) {
        for (int i = tid; i < n * n; i += kThreads) {
            const int p = i / n, q = i - p * n;
            const cd sp = sm[p];
            xs[i] = load_x(tri, n_bl, n_sum, p, q, fl[p] || fl[q], fold, cd{sp.re, -sp.im}, sm[q]);
        }
        __syncthreads();
    }
    // what this lane keeps for its columns q = l + 64 k
    cd sq[kTerms];
    bool flq[kTerms];
#pragma unroll
    for (int k = 0; k < kTerms; k++) {
        const int q = l + 64 * k;
        sq[k] = q < n ? sm[q] : cd{1.0, 0.0};
        flq[k] = q < n ? fl[q] != 0 : true;
    }

    int cur = 0, it = 1, status = 0;
    for (;; it++) {
        const cd* go = gbuf + cur * n;
        cd* gn = gbuf + (cur ^ 1) * n;
        cd gq[kTerms];
        double mq[kTerms];
#pragma unroll
        for (int k = 0; k < kTerms; k++) {
            const int q = l + 64 * k;
            gq[k] = q < n ? go[q] : cd{0.0, 0.0};
            mq[k] = gq[k].re * gq[k].re + gq[k].im * gq[k].im;   // (a flagged q keeps (0, 0): its m is +0.0)
        }
        for (int p = w; p < n; p += kWaves) {
            const bool flp = fl[p] != 0;
            cd spc{1.0, 0.0};
            if (!RESIDENT) {
                const cd sp = sm[p];
                spc = cd{sp.re, -sp.im};
            }
            double nr = 0.0, ni = 0.0, den = 0.0;
#pragma unroll
            for (int k = 0; k < kTerms; k++) {
                const int q = l + 64 * k;
                if (q < n) {
                    const cd x = RESIDENT ? xs[p * n + q] : load_x(tri, n_bl, n_sum, p, q, flp || flq[k], fold, spc, sq[k]);
                    const cd t = cmul(x, gq[k]);
                    nr = nr + t.re;
                    ni = ni + t.im;
                    den = den + (q != p ? mq[k] : 0.0);
                }
            }
            nr = halve(nr);
            ni = halve(ni);
            den = halve(den);
            if (l == 0) {
                cd h{0.0, 0.0};
                if (den != 0.0 && !flp) h = cd{nr / den, ni / den};
                if (!(it & 1)) {
                    const cd g = go[p];
                    h = cd{0.5 * (h.re + g.re), 0.5 * (h.im + g.im)};
                }
                gn[p] = h;
            }
        }
        __syncthreads();
        cur ^= 1;
        if (!(it & 1)) {   // every wave: the same words, the same order, the same decision
            double delta = 0.0, nu = 0.0;
#pragma unroll
            for (int k = 0; k < kTerms; k++) {
                const int p = l + 64 * k;
                if (p < n) {
                    const cd h = gn[p], g = go[p];
                    const double dr = h.re - g.re, di = h.im - g.im;
                    delta = delta + (dr * dr + di * di);
                    nu = nu + (h.re * h.re + h.im * h.im);
                }
            }
            delta = halve(delta);
            nu = halve(nu);
            if (delta <= a.tol * a.tol * nu) {
                status = 1;
                break;
            }
            if (it == a.max_iter) break;
            __syncthreads();   // the next iteration overwrites `go`
        } else if (it == a.max_iter) {
            break;
        }
    }

    // ---- the phase reference, and out
    const cd* g = gbuf + cur * n;
    int r = a.ref_ant;
    if (r < 0) {
        for (int q = 0; q < n && r < 0; q++)
            if (!fl[q]) r = q;
    }
    bool turn = false;
    cd c{1.0, 0.0};
    if (r >= 0) {
        const cd gr = g[r];
        const double m = sqrt(gr.re * gr.re + gr.im * gr.im);
        if (m > 0.0) {
            turn = true;
            c = cd{gr.re / m, -gr.im / m};
        }
    }
    cd* out = a.gains + ((size_t)po * a.n_freq + f) * n;
    for (int p = tid; p < n; p += kThreads) out[p] = turn ? cmul(g[p], c) : g[p];
    if (tid == 0) {
        int32_t* inf = a.info + 2 * ((size_t)po * a.n_freq + f);
        inf[0] = it;
        inf[1] = status;
    }
}

struct CalwArgs {
    const int8_t* __restrict__ w_in;     // [f][ant][beam]{re, im}, 4-byte aligned
    int8_t* __restrict__ w_out;
    const cd* __restrict__ gains;        // [f][ant]
    const uint8_t* __restrict__ flags;
    int n_ant, n_beams, mode;
};

constexpr int kCalwThreads = 256;
static_assert(kCalwThreads >= kCalMaxAnt, "one thread per antenna in the search for k_f");

__device__ __forceinline__ int clip_rint(double v)
{
    v = rint(v);   // half to even
    return v > 127.0 ? 127 : (v < -127.0 ? -127 : (int)v);
}

__global__ __launch_bounds__(kCalwThreads) void calw_kernel(CalwArgs a)
{
    __shared__ double red[kCalwThreads / 64];
    const int f = blockIdx.x / a.n_ant, ant = blockIdx.x - f * a.n_ant;
    const int tid = threadIdx.x;
    const cd g = a.gains[(size_t)f * a.n_ant + ant];
    const double m = sqrt(g.re * g.re + g.im * g.im);
    const bool use = m > 0.0 && !(a.flags && a.flags[ant] != 0);
    cd c{0.0, 0.0};
    if (use) c = cd{g.re / m, -g.im / m};
    if (a.mode == 1) {   // k_f: the smallest non-zero |g| among the channel's unflagged antennas (a minimum: any order)
        double mine = __builtin_inf();
        if (tid < a.n_ant && !(a.flags && a.flags[tid] != 0)) {
            const cd o = a.gains[(size_t)f * a.n_ant + tid];
            const double mo = sqrt(o.re * o.re + o.im * o.im);
            if (mo > 0.0) mine = mo;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) mine = fmin(mine, __shfl_xor(mine, s, 64));
        if ((tid & 63) == 0) red[tid >> 6] = mine;
        __syncthreads();
        double k = red[0];
#pragma unroll
        for (int i = 1; i < kCalwThreads / 64; i++) k = fmin(k, red[i]);
        if (use) {
            const double s = k / m;
            c = cd{c.re * s, c.im * s};
        }
    }
    const size_t row = (size_t)blockIdx.x * a.n_beams * 2;   // n_beams % 4 == 0: rows are whole dwords
    const uint32_t* in = reinterpret_cast<const uint32_t*>(a.w_in + row);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.w_out + row);
    for (int i = tid; i < a.n_beams / 2; i += kCalwThreads) {   // two beams per thread
        const uint32_t v = in[i];
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const double wr = (double)(int8_t)(v >> (16 * j)), wi = (double)(int8_t)(v >> (16 * j + 8));
            const int re = clip_rint(wr * c.re - wi * c.im), im = clip_rint(wr * c.im + wi * c.re);
            o |= ((uint32_t)(re & 0xFF) | ((uint32_t)(im & 0xFF) << 8)) << (16 * j);
        }
        out[i] = o;
    }
}

size_t solve_lds_bytes(int n, bool resident) { return (size_t)(3 * n + (resident ? n * n : 0)) * sizeof(cd) + (size_t)((n + 15) & ~15); }

}  // namespace

hipError_t launch_solve_gains(int n_ant, int n_freq, int n_pol, const long long* d_vis, const double* d_model, const uint8_t* d_flags, double tol,
                              int max_iter, int ref_ant, bool joint_pol, bool streamed, double* d_gains, int32_t* d_info, hipStream_t s)
{
    if (!cal_supported(n_ant) || n_freq <= 0 || n_pol <= 0 || !d_vis || !d_gains || !d_info || max_iter < 1 || !(tol >= 0.0) || ref_ant >= n_ant ||
        ((uintptr_t)d_vis & 15) || ((uintptr_t)d_model & 15) || ((uintptr_t)d_gains & 15) || ((uintptr_t)d_info & 3))
        return hipErrorInvalidValue;
    const bool resident = !streamed && n_ant <= kCalResidentMaxAnt;
    const long long grid = (long long)(joint_pol ? 1 : n_pol) * n_freq;
    if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
    CalArgs a;
    a.vis = d_vis;
    a.model = reinterpret_cast<const cd*>(d_model);
    a.flags = d_flags;
    a.gains = reinterpret_cast<cd*>(d_gains);
    a.info = d_info;
    a.tol = tol;
    a.n_ant = n_ant;
    a.n_freq = n_freq;
    a.n_pol = n_pol;
    a.max_iter = max_iter;
    a.ref_ant = ref_ant;
    a.joint = joint_pol ? 1 : 0;
    const size_t lds = solve_lds_bytes(n_ant, resident);
    auto kern = resident ? solve_kernel<true> : solve_kernel<false>;
    if (lds > 48 * 1024) {   // the resident square at 64 antennas: 64 KiB + the gains
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    (void)hipGetLastError();
    record_launch(resident ? "solve_kernel<true>" : "solve_kernel<false>");
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_calibrate_weights(int n_ant, int n_freq, int n_beams, const int8_t* d_w_in, const double* d_gains_layer, const uint8_t* d_flags,
                                    int mode, int8_t* d_w_out, hipStream_t s)
{
    if (!cal_supported(n_ant) || n_freq <= 0 || n_beams <= 0 || n_beams % 4 || !d_w_in || !d_gains_layer || !d_w_out || (mode != 0 && mode != 1) ||
        ((uintptr_t)d_w_in & 3) || ((uintptr_t)d_w_out & 3) || ((uintptr_t)d_gains_layer & 15))
        return hipErrorInvalidValue;
    const long long grid = (long long)n_freq * n_ant;
    if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
    CalwArgs a;
    a.w_in = d_w_in;
    a.w_out = d_w_out;
    a.gains = reinterpret_cast<const cd*>(d_gains_layer);
    a.flags = d_flags;
    a.n_ant = n_ant;
    a.n_beams = n_beams;
    a.mode = mode;
    (void)hipGetLastError();
    record_launch("calw_kernel");
    hipLaunchKernelGGL(calw_kernel, dim3((unsigned)grid), dim3(kCalwThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dsabf
