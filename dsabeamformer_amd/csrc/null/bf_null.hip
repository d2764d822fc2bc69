// bf_null.hip -- device code of the spatial null (include/dsabf.h: bf_null_solve_device, bf_null_weights_device; contract:
// docs/NULLING.md).
//
// null_solve_kernel: deflated power iteration, one workgroup (8 waves) per channel.  fp64 throughout, one rounding per operation (no FMA
// contraction: the library is built with -ffp-contract=off and the pragma below says so again), every sum over antennas in the OSUM order
// of docs/CALIBRATION.md section 2, with the gain solver's mapping:
//   lane l of a wave owns the columns q = l (mod 64): it adds its (up to four) terms in ascending q onto +0.0, and six butterfly
//   steps (xor 32, 16, 8, 4, 2, 1) are the six halving steps; after them every lane holds the one result.
// Streamed: wave w owns the rows p = w, w + 8, ... of the product y = x u and reduces four of them side by side (eight independent
// butterflies).  Resident (n_ant <= 64, one term per partial sum): lane p forms row p, wave w the node T(w, 8) of the halving tree, and
// no shuffle is needed.  Either way the product goes through LDS (two buffers that alternate, ONE barrier per multiplication); everything behind it -- the deflation
// against the vectors already found, the norm, the new iterate, the distance to the old one -- every wave does itself on its own
// lane-distributed copy, from the same words in the same order, so the stop decision is workgroup-uniform without a shared flag.
// x[p][q] comes from load_x() on either storage path:
//   RESIDENT   (n_ant <= 64) the fp64 square is built once in LDS (16 n^2 bytes, column by column);
//   streamed   the int64 triangle is re-read every iteration (row p below the diagonal, column p above it) and converted on the fly.
//              No scratch memory, so concurrent solves on any queues share nothing.
// null_apply_kernel: the projection of the weights, one workgroup per channel, one thread per beam column.
#include "bf_null_kernels.h"
#include "../rec/bf_launch_record.h"

#pragma clang fp contract(off)

namespace dsabf {

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTerms = kNullMaxAnt / 64;   // terms per lane of one OSUM
constexpr int kRows = 4;                   // rows of the product a wave reduces side by side

struct __attribute__((aligned(16))) cd {
    double re, im;
};
typedef long long v2ll __attribute__((ext_vector_type(2)));

__device__ __forceinline__ cd cmul(cd a, cd b) { return cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// lane `lane` (wave-uniform) of a double, through the scalar unit
__device__ __forceinline__ double readlane_d(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ cd cadd(cd a, cd b) { return cd{a.re + b.re, a.im + b.im}; }

// eight nodes T(i, 8), T(i + 1, 8), ... of OSUM's halving tree in the order of their index, or eight leaves i, i + 8, ... of one such
// node: T(i, w) = T(i, 2w) + T(i + w, 2w) pairs 0 with 4, 2 with 6, 1 with 5 and 3 with 7, then those, then the two halves
__device__ __forceinline__ cd tree8(const cd* t) { return cadd(cadd(cadd(t[0], t[4]), cadd(t[2], t[6])), cadd(cadd(t[1], t[5]), cadd(t[3], t[7]))); }

// the six halving steps of OSUM on the 64 partial sums of a wave; every lane returns the result
__device__ __forceinline__ double halve(double s)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) s = s + __shfl_xor(s, w, 64);
    return s;
}

struct SolveArgs {
    const long long* __restrict__ vis;   // [f][pol][bl]{re, im}, 16-byte aligned
    const uint8_t* __restrict__ flags;   // [ant] or NULL
    cd* __restrict__ vecs;               // [f][n_null][ant]
    double* __restrict__ eig;            // [f][n_null + 1]
    int32_t* __restrict__ info;          // [f][1 + 2 n_null]
    double tol, min_ratio;
    int n_ant, n_pol, n_null, max_iter, pol;
};

// The integer visibility (a1, a2), a2 <= a1, of this channel: one polarisation's entry, or the int64 sum over all of them.
__device__ __forceinline__ v2ll load_v(const long long* tri, size_t n_bl, int n_sum, int a1, int a2)
{
    const size_t e = (size_t)a1 * (size_t)(a1 + 1) / 2 + (size_t)a2;
    v2ll v = *reinterpret_cast<const v2ll*>(tri + 2 * e);
    for (int k = 1; k < n_sum; k++) v += *reinterpret_cast<const v2ll*>(tri + 2 * (e + (size_t)k * n_bl));
    return v;
}

// x[p][q] of the contract (step 1): Hermitian, the diagonal (re, +0.0), (0, 0) for a flagged p or q
__device__ __forceinline__ cd load_x(const long long* tri, size_t n_bl, int n_sum, int p, int q, bool dead)
{
    if (dead) return cd{0.0, 0.0};
    const v2ll v = q <= p ? load_v(tri, n_bl, n_sum, p, q) : load_v(tri, n_bl, n_sum, q, p);
    cd x{(double)v.x, (double)v.y};
    if (q > p) x.im = -x.im;
    if (q == p) x.im = 0.0;
    return x;
}

template <bool RESIDENT>
__global__ __launch_bounds__(kThreads) void null_solve_kernel(SolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = a.n_ant;
    cd* ybuf = reinterpret_cast<cd*>(smem);                       // [2][n]: the product, written and read in turn
    cd* es = ybuf + 2 * n;                                        // [kNullMaxVecs][n]: the vectors found so far
    cd* xs = es + kNullMaxVecs * n;                               // [q][p] (RESIDENT): the square, columns contiguous
    cd* pbuf = xs + (RESIDENT ? n * n : 0);                       // [2][kWaves][64] (RESIDENT): every wave's node of the product's tree
    uint8_t* fl = reinterpret_cast<uint8_t*>(pbuf + (RESIDENT ? 2 * kWaves * 64 : 0));   // [n]

    const int f = blockIdx.x;
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const size_t n_bl = (size_t)n * (size_t)(n + 1) / 2;
    const int n_sum = a.pol < 0 ? a.n_pol : 1;
    const long long* tri = a.vis + ((size_t)f * a.n_pol + (a.pol < 0 ? 0 : a.pol)) * n_bl * 2;

    for (int p = tid; p < n; p += kThreads) fl[p] = (a.flags && a.flags[p] != 0) ? 1 : 0;
    __syncthreads();
    if (RESIDENT) {
        for (int i = tid; i < n * n; i += kThreads) {
            const int q = i / n, p = i - q * n;
            xs[i] = load_x(tri, n_bl, n_sum, p, q, fl[p] || fl[q]);
        }
        __syncthreads();
    }
    auto X = [&](int p, int q, bool dead) -> cd { return RESIDENT ? xs[q * n + p] : load_x(tri, n_bl, n_sum, p, q, dead); };

    // ---- what every wave knows of the channel: its lanes' flags, the trace, the number of live antennas, the start column p*
    bool flq[kTerms];
    double dsum = 0.0, best = -__builtin_inf();
    int live = 0, star = 0x7FFFFFFF;
#pragma unroll
    for (int k = 0; k < kTerms; k++) {
        const int q = l + 64 * k;
        flq[k] = q < n ? fl[q] != 0 : true;
        if (q < n) {
            const double d = X(q, q, flq[k]).re;
            dsum = dsum + d;
            if (!flq[k]) {
                live++;
                if (d > best) {   // ascending q: the lowest index on ties
                    best = d;
                    star = q;
                }
            }
        }
    }
    const double tr = halve(dsum);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        live += __shfl_xor(live, s, 64);
        const double ob = __shfl_xor(best, s, 64);
        const int oi = __shfl_xor(star, s, 64);
        if (ob > best || (ob == best && oi < star)) {
            best = ob;
            star = oi;
        }
    }
    const bool any = star != 0x7FFFFFFF;

    cd* out = a.vecs + (size_t)f * a.n_null * n;
    double* eig = a.eig + (size_t)f * (a.n_null + 1);
    int32_t* info = a.info + (size_t)f * (1 + 2 * a.n_null);
    bool ended = false, used = true;
    int par = 0, n_used = 0;
    double rem = tr;
    for (int j = 0; j < a.n_null; j++) {
        cd u[kTerms], y[kTerms];
        double lam = 0.0;
        int it = 0, status = ended ? 2 : 0;
#pragma unroll
        for (int k = 0; k < kTerms; k++) u[k] = cd{0.0, 0.0};
        while (!ended) {
            if (it == 0) {   // the start: column p* of x
#pragma unroll
                for (int k = 0; k < kTerms; k++) {
                    const int p = l + 64 * k;
                    y[k] = (p < n && any) ? X(p, star, flq[k]) : cd{0.0, 0.0};
                }
            } else if (RESIDENT) {
                // y = x u with no shuffle (n <= 64: every partial sum of OSUM is one term, 0.0 + x[p][q] u_q): lane p forms row p.  Wave w
                // adds the leaves q = w, w + 8, ... into the node T(w, 8) of the halving tree, u_q coming from lane q through the scalar
                // unit; after the barrier every wave adds the eight nodes of its lanes' rows -- the same tree, the same bits.
                cd* pb = pbuf + par * (kWaves * 64);
                const int wu = __builtin_amdgcn_readfirstlane(w);
                cd leaf[8];
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const int q = wu + 8 * m;
                    leaf[m] = cd{0.0, 0.0};
                    if (q < n) {
                        const cd uq{readlane_d(u[0].re, q), readlane_d(u[0].im, q)};
                        if (l < n) {
                            const cd t = cmul(xs[q * n + l], uq);
                            leaf[m] = cd{0.0 + t.re, 0.0 + t.im};
                        }
                    }
                }
                pb[wu * 64 + l] = tree8(leaf);
                __syncthreads();   // the one barrier of a multiplication: the next one writes the other buffer
                cd node[8];
#pragma unroll
                for (int m = 0; m < 8; m++) node[m] = pb[m * 64 + l];
                y[0] = l < n ? tree8(node) : cd{0.0, 0.0};
#pragma unroll
                for (int k = 1; k < kTerms; k++) y[k] = cd{0.0, 0.0};
                par ^= 1;
            } else {         // y = x u: this wave's rows, four at a time
                cd* yb = ybuf + par * n;
                for (int p0 = w; p0 < n; p0 += kWaves * kRows) {
                    double sr[kRows], si[kRows];
#pragma unroll
                    for (int r = 0; r < kRows; r++) {
                        const int p = p0 + kWaves * r;
                        sr[r] = 0.0;
                        si[r] = 0.0;
                        if (p < n) {
                            const bool flp = fl[p] != 0;
#pragma unroll
                            for (int k = 0; k < kTerms; k++) {
                                const int q = l + 64 * k;
                                if (q < n) {
                                    const cd t = cmul(X(p, q, flp || flq[k]), u[k]);
                                    sr[r] = sr[r] + t.re;
                                    si[r] = si[r] + t.im;
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
                        for (int r = 0; r < kRows; r++) {
                            sr[r] = sr[r] + __shfl_xor(sr[r], s, 64);
                            si[r] = si[r] + __shfl_xor(si[r], s, 64);
                        }
                    }
                    if (l < kRows && p0 + kWaves * l < n) {
                        cd v{sr[0], si[0]};
#pragma unroll
                        for (int r = 1; r < kRows; r++)
                            if (l == r) v = cd{sr[r], si[r]};
                        yb[p0 + kWaves * l] = v;
                    }
                }
                __syncthreads();   // the one barrier of a multiplication: the next one writes the other buffer
#pragma unroll
                for (int k = 0; k < kTerms; k++) {
                    const int p = l + 64 * k;
                    y[k] = p < n ? yb[p] : cd{0.0, 0.0};
                }
                par ^= 1;
            }
            // ---- every wave: the same words, the same order, the same decisions
            for (int i = 0; i < j; i++) {   // y <- y - e_i (e_i^H y)
                cd e[kTerms];
                double cr = 0.0, ci = 0.0;
#pragma unroll
                for (int k = 0; k < kTerms; k++) {
                    const int p = l + 64 * k;
                    if (p < n) {
                        e[k] = es[i * n + p];
                        const cd t = cmul(cd{e[k].re, -e[k].im}, y[k]);
                        cr = cr + t.re;
                        ci = ci + t.im;
                    }
                }
                const cd c{halve(cr), halve(ci)};
#pragma unroll
                for (int k = 0; k < kTerms; k++) {
                    if (l + 64 * k < n) {
                        const cd t = cmul(e[k], c);
                        y[k] = cd{y[k].re - t.re, y[k].im - t.im};
                    }
                }
            }
            double s2 = 0.0;
#pragma unroll
            for (int k = 0; k < kTerms; k++)
                if (l + 64 * k < n) s2 = s2 + (y[k].re * y[k].re + y[k].im * y[k].im);
            lam = sqrt(halve(s2));
            if (lam == 0.0) {   // nothing is left in this channel: this vector and all later ones are zero
                status = 2;
                ended = true;
#pragma unroll
                for (int k = 0; k < kTerms; k++) u[k] = cd{0.0, 0.0};
                break;
            }
            double delta = 0.0;
#pragma unroll
            for (int k = 0; k < kTerms; k++) {
                if (l + 64 * k < n) {
                    const cd un{y[k].re / lam, y[k].im / lam};
                    const double dr = un.re - u[k].re, di = un.im - u[k].im;
                    delta = delta + (dr * dr + di * di);
                    u[k] = un;
                }
            }
            if (it >= 1) {
                delta = halve(delta);
                if (delta <= a.tol * a.tol) {
                    status = 1;
                    break;
                }
                if (it == a.max_iter) break;
            }
            it++;
        }
        // ---- the use rule, and out
        rem = rem - lam;
        used = used && live > j + 1 && lam > 0.0;
        if (used) {
            const double rest = rem / (double)(live - j - 1);
            used = lam >= a.min_ratio * (rest > 0.0 ? rest : 0.0);
        }
        n_used += used ? 1 : 0;
        if (w == 0) {
#pragma unroll
            for (int k = 0; k < kTerms; k++) {
                const int p = l + 64 * k;
                if (p < n) {
                    es[j * n + p] = u[k];
                    out[(size_t)j * n + p] = used ? u[k] : cd{0.0, 0.0};
                }
            }
            if (l == 0) {
                eig[j] = lam;
                info[1 + 2 * j] = it;
                info[2 + 2 * j] = status;
            }
        }
        __syncthreads();   // e_j is in LDS for the vectors that follow
    }
    if (tid == 0) {
        eig[a.n_null] = tr;
        info[0] = n_used;
    }
}

size_t solve_lds_bytes(int n, bool resident)
{
    return (size_t)((2 + kNullMaxVecs) * n + (resident ? n * n + 2 * kWaves * 64 : 0)) * sizeof(cd) + (size_t)((n + 15) & ~15);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The projection.  One workgroup per channel, thread t owns the beam columns b = t, t + 256, ...: a column's c_j = OSUM_a u_j[a] w[a][b],
// its w' and its output depend on that column alone, so the weights may be projected in place.  OSUM by one thread: the 64 partial sums
// are the leaves of the halving tree, T(i, 64) = partial i and T(i, w) = T(i, 2w) + T(i + w, 2w), the result T(0, 1); the recursion below
// is that tree.  A pass over a column forms its c_j and then its w'; the first pass (BF_NULL_SCALED only) takes
// the largest |part|, the second pass forms the same w' again -- the same operations on the same bytes, the same bits -- and writes.
constexpr int kApplyThreads = 256;

struct ApplyArgs {
    const int8_t* w_in;                  // [f][ant][beam]{re, im}, 4-byte aligned
    int8_t* w_out;                       // (may be w_in: no __restrict__ on either)
    const cd* __restrict__ vecs;         // [f][n_null][ant]
    const int32_t* __restrict__ info;    // [f][1 + 2 n_null]
    const uint8_t* __restrict__ flags;
    double* __restrict__ scale;          // [f] or NULL
    int n_ant, n_beams, n_null, mode;
};

__device__ __forceinline__ cd unpack(uint16_t v) { return cd{(double)(int8_t)(v & 0xFF), (double)(int8_t)(v >> 8)}; }

// T(i, W) of one column against one vector.  The levels below W = 8 are unrolled (eight leaves in flight), the three above are loops.
template <int W>
__device__ __forceinline__ cd osum_column(int i, const cd* u, const uint16_t* col, int n, int n_beams)
{
    if constexpr (W == 64) {
        cd s{0.0, 0.0};
        for (int ant = i; ant < n; ant += 64) {   // partial i: the terms i, i + 64, ... that exist, ascending, onto +0.0
            const cd t = cmul(u[ant], unpack(col[(size_t)ant * n_beams]));
            s = cd{s.re + t.re, s.im + t.im};
        }
        return s;
    } else if constexpr (W >= 8) {
        const cd lo = osum_column<2 * W>(i, u, col, n, n_beams), hi = osum_column<2 * W>(i + W, u, col, n, n_beams);
        return cd{lo.re + hi.re, lo.im + hi.im};
    } else {
        cd lo{0.0, 0.0};
#pragma nounroll
        for (int h = 0; h < 2; h++) {
            const cd v = osum_column<2 * W>(i + h * W, u, col, n, n_beams);
            lo = h ? cd{lo.re + v.re, lo.im + v.im} : v;
        }
        return lo;
    }
}

__device__ __forceinline__ int clip_rint(double v)
{
    v = rint(v);   // half to even
    return v > 127.0 ? 127 : (v < -127.0 ? -127 : (int)v);
}

__global__ __launch_bounds__(kApplyThreads) void null_apply_kernel(ApplyArgs a)
{
    __shared__ cd us[kNullMaxVecs * kNullMaxAnt];      // 16 KiB: the channel's vectors
    __shared__ cd cs[kNullMaxVecs][kApplyThreads];     // 16 KiB: c_j of the column a thread is working on (its own words only)
    __shared__ double red[kApplyThreads / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = a.n_ant, nb = a.n_beams;
    int nu = a.info[(size_t)f * (1 + 2 * a.n_null)];
    nu = nu < 0 ? 0 : (nu > a.n_null ? a.n_null : nu);
    const size_t slab = (size_t)f * n * nb;   // in (re, im) pairs
    const uint16_t* in = reinterpret_cast<const uint16_t*>(a.w_in) + slab;
    uint16_t* out = reinterpret_cast<uint16_t*>(a.w_out) + slab;
    if (nu == 0) {   // nothing to project: the bytes as they are, flagged antennas zeroed
        for (int i = tid; i < n * nb; i += kApplyThreads) {
            const uint16_t v = in[i];
            out[i] = (a.flags && a.flags[i / nb] != 0) ? (uint16_t)0 : v;
        }
        if (tid == 0 && a.scale) a.scale[f] = 1.0;
        return;
    }
    for (int i = tid; i < nu * n; i += kApplyThreads) us[i] = a.vecs[(size_t)f * a.n_null * n + i];
    __syncthreads();

    double big = 0.0, k = 1.0;
    for (int pass = a.mode == 0 ? 0 : 1; pass < 2; pass++) {
        for (int b = tid; b < nb; b += kApplyThreads) {
            for (int j = 0; j < nu; j++) cs[j][tid] = osum_column<1>(0, us + j * n, in + b, n, nb);
            cd c[kNullMaxVecs];
#pragma unroll
            for (int j = 0; j < kNullMaxVecs; j++) c[j] = j < nu ? cs[j][tid] : cd{0.0, 0.0};
            for (int ant = 0; ant < n; ant++) {
                const bool flagged = a.flags && a.flags[ant] != 0;
                cd r = unpack(in[(size_t)ant * nb + b]);
#pragma unroll
                for (int j = 0; j < kNullMaxVecs; j++) {   // w' = w - conj(u_0) c_0 - ... in j order
                    if (j < nu) {
                        const cd u = us[j * n + ant];
                        const cd t = cmul(cd{u.re, -u.im}, c[j]);
                        r = cd{r.re - t.re, r.im - t.im};
                    }
                }
                if (flagged) r = cd{0.0, 0.0};
                if (pass == 0) {
                    big = fmax(big, fmax(fabs(r.re), fabs(r.im)));
                } else {
                    const int re = clip_rint(k * r.re), im = clip_rint(k * r.im);
                    out[(size_t)ant * nb + b] = (uint16_t)((re & 0xFF) | ((im & 0xFF) << 8));
                }
            }
        }
        if (pass == 0) {   // k_f = min(1, 127 / M_f): a maximum has no order
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) big = fmax(big, __shfl_xor(big, s, 64));
            if ((tid & 63) == 0) red[tid >> 6] = big;
            __syncthreads();
            big = red[0];
#pragma unroll
            for (int i = 1; i < kApplyThreads / 64; i++) big = fmax(big, red[i]);
            k = 127.0 / big;   // (M_f == 0: +inf)
            k = k < 1.0 ? k : 1.0;
        }
    }
    if (tid == 0 && a.scale) a.scale[f] = k;
}

}  // namespace

hipError_t launch_null_solve(int n_ant, int n_freq, int n_pol, const long long* d_vis, const uint8_t* d_flags, int n_null, double min_ratio,
                             double tol, int max_iter, int pol, bool streamed, double* d_vecs, double* d_eig, int32_t* d_info, hipStream_t s)
{
    if (!null_supported(n_ant) || n_freq <= 0 || n_pol <= 0 || !d_vis || !d_vecs || !d_eig || !d_info || n_null < 1 || n_null > kNullMaxVecs ||
        max_iter < 1 || !(tol >= 0.0) || !(min_ratio >= 0.0) || pol < -1 || pol >= n_pol || ((uintptr_t)d_vis & 15) || ((uintptr_t)d_vecs & 15) ||
        ((uintptr_t)d_eig & 7) || ((uintptr_t)d_info & 3))
        return hipErrorInvalidValue;
    const bool resident = !streamed && n_ant <= kNullResidentMaxAnt;
    SolveArgs a;
    a.vis = d_vis;
    a.flags = d_flags;
    a.vecs = reinterpret_cast<cd*>(d_vecs);
    a.eig = d_eig;
    a.info = d_info;
    a.tol = tol;
    a.min_ratio = min_ratio;
    a.n_ant = n_ant;
    a.n_pol = n_pol;
    a.n_null = n_null;
    a.max_iter = max_iter;
    a.pol = pol;
    const size_t lds = solve_lds_bytes(n_ant, resident);
    auto kern = resident ? null_solve_kernel<true> : null_solve_kernel<false>;
    if (lds > 48 * 1024) {   // the resident square at 64 antennas: 64 KiB + the vectors
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    (void)hipGetLastError();
    record_launch(resident ? "null_solve_kernel<true>" : "null_solve_kernel<false>");
    hipLaunchKernelGGL(kern, dim3((unsigned)n_freq), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_null_weights(int n_ant, int n_freq, int n_beams, const int8_t* d_w_in, const double* d_vecs, const int32_t* d_info, int n_null,
                               const uint8_t* d_flags, int mode, int8_t* d_w_out, double* d_scale, hipStream_t s)
{
    if (!null_supported(n_ant) || n_freq <= 0 || n_beams <= 0 || !d_w_in || !d_vecs || !d_info || !d_w_out || n_null < 1 ||
        n_null > kNullMaxVecs || (mode != 0 && mode != 1) || ((uintptr_t)d_w_in & 3) || ((uintptr_t)d_w_out & 3) || ((uintptr_t)d_vecs & 15) ||
        ((uintptr_t)d_info & 3) || ((uintptr_t)d_scale & 7))
        return hipErrorInvalidValue;
    ApplyArgs a;
    a.w_in = d_w_in;
    a.w_out = d_w_out;
    a.vecs = reinterpret_cast<const cd*>(d_vecs);
    a.info = d_info;
    a.flags = d_flags;
    a.scale = d_scale;
    a.n_ant = n_ant;
    a.n_beams = n_beams;
    a.n_null = n_null;
    a.mode = mode;
    (void)hipGetLastError();
    record_launch("null_apply_kernel");
    hipLaunchKernelGGL(null_apply_kernel, dim3((unsigned)n_freq), dim3(kApplyThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dsabf
