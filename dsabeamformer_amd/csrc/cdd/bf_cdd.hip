// bf_cdd.hip -- device code of the coherent dedispersion stage (include/dsabf.h: bf_cdd_*; contract: docs/COHERENT_DEDISPERSION.md).
//
// One workgroup per (segment, channel, beam) holds the N = 2^M samples of both polarisations in LDS and runs, in place,
//   load (zero outside the series) -> forward transform -> multiply by the channel's chirp row -> inverse transform -> epilogue.
// The forward transform is radix-2 decimation in FREQUENCY (natural order in, bit-reversed order out), the inverse radix-2 decimation
// in TIME with the conjugated twiddles (bit-reversed in, natural out); the chirp rows are stored bit-reversed by the host, so nothing
// is ever permuted on the device.  The operation order is that of the plain radix-2 stage loops (docs section 2 and
// tests/support/cdd_oracle.py); a PASS here takes two or three consecutive stages of 4 or 8 elements through registers, which performs
// the same butterflies on the same operands -- every float operation is rounded on its own (__f*_rn), so the bits do not depend on it.
//
// LDS: element p of a polarisation lives at float2 index p + (p >> 5) -- one float2 of padding per 32, so that the stride-8 ... stride-
// 2048 accesses of the passes do not meet in one bank (ds_read_b64 banks on 64 dwords).  16.5 N bytes per workgroup: 66 KiB at N = 4096.
#include "bf_cdd_kernels.h"
#include "../rec/bf_launch_record.h"

#include <cmath>

namespace dsabf {

namespace {

__host__ __device__ constexpr int cdd_threads(int m) { return (1 << m) / 4 < 64 ? 64 : (1 << m) / 4 > 512 ? 512 : (1 << m) / 4; }
__host__ __device__ constexpr int cdd_stride(int m) { return (1 << m) + (1 << (m - 5)); }   // float2 per polarisation, padding included
__device__ __forceinline__ int pad(int p) { return p + (p >> 5); }

struct CddArgs {
    const float2* __restrict__ in;
    void* __restrict__ out;
    const float2* __restrict__ tw;
    const float2* __restrict__ chirp;
    int n_chan, K, n_time, n_edge, V, n_int, T;
    int out16;   // Stokes: the output is 16-byte aligned
};

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w)
{
    return make_float2(__fsub_rn(__fmul_rn(a.x, w.x), __fmul_rn(a.y, w.y)), __fadd_rn(__fmul_rn(a.x, w.y), __fmul_rn(a.y, w.x)));
}

// One pass: the R stages with half-lengths 2^LOGH ... 2^(LOGH + R - 1) -- descending for the forward transform (INV false), ascending
// for the inverse -- of both polarisations.  An item is the 2^R elements base + q 2^LOGH; it reads and writes only those, in place.
template <int M, int R, int LOGH, bool INV, bool MUL>
__device__ __forceinline__ void pass(float2* lds, const float2* __restrict__ tw, const float2* __restrict__ row)
{
    constexpr int E = 1 << R, H = 1 << LOGH, ITEMS = 1 << (M - R), NT = cdd_threads(M);
#pragma unroll
    for (int it0 = 0; it0 < 2 * ITEMS; it0 += NT) {
        const int it = it0 + (int)threadIdx.x;
        if (2 * ITEMS < NT && it >= 2 * ITEMS) break;
        const int pol = it >> (M - R), t = it & (ITEMS - 1);
        const int lo = t & (H - 1), base = ((t >> LOGH) << (LOGH + R)) + lo;
        float2* x = lds + pol * cdd_stride(M);
        float2 v[E];
#pragma unroll
        for (int q = 0; q < E; q++) v[q] = x[pad(base + (q << LOGH))];
#pragma unroll
        for (int s = 0; s < R; s++) {
            const int b = INV ? s : R - 1 - s;   // the stage of half-length H << b: register distance 1 << b
#pragma unroll
            for (int q = 0; q < E; q++) {
                if (q & (1 << b)) continue;
                const int j = lo + ((q & ((1 << b) - 1)) << LOGH);   // position within the half
                float2 w = tw[j << (M - 1 - LOGH - b)];
                const float2 lower = v[q], upper = v[q | (1 << b)];
                if (INV) {
                    w.y = -w.y;
                    const float2 tmp = cmul(upper, w);
                    v[q] = cadd(lower, tmp);
                    v[q | (1 << b)] = csub(lower, tmp);
                } else {
                    v[q] = cadd(lower, upper);
                    v[q | (1 << b)] = cmul(csub(lower, upper), w);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < E; q++) {
            const int p = base + (q << LOGH);
            x[pad(p)] = MUL ? cmul(v[q], row[p]) : v[q];
        }
    }
    __syncthreads();
}

constexpr int pass_stages(int remaining) { return remaining == 4 ? 2 : remaining < 3 ? remaining : 3; }

// forward: the stages of half-length 2^(TOP - 1) ... 1 are still to do; the last pass multiplies by the chirp row
template <int M, int TOP>
__device__ __forceinline__ void forward(float2* lds, const float2* __restrict__ tw, const float2* __restrict__ row)
{
    if constexpr (TOP > 0) {
        constexpr int R = pass_stages(TOP);
        pass<M, R, TOP - R, false, TOP - R == 0>(lds, tw, row);
        forward<M, TOP - R>(lds, tw, row);
    }
}

// inverse: the stages of half-length 1 ... 2^(DONE - 1) are done
template <int M, int DONE>
__device__ __forceinline__ void inverse(float2* lds, const float2* __restrict__ tw)
{
    if constexpr (DONE < M) {
        constexpr int R = pass_stages(M - DONE);
        pass<M, R, DONE, true, false>(lds, tw, nullptr);
        inverse<M, DONE + R>(lds, tw);
    }
}

template <int M, bool STOKES>
__global__ __launch_bounds__(cdd_threads(M)) void cdd_kernel(CddArgs a)
{
    constexpr int N = 1 << M, NT = cdd_threads(M), STRIDE = cdd_stride(M);
    __shared__ float2 lds[2 * STRIDE];
    const int tid = (int)threadIdx.x;
    // beams fastest, then channels, then segments: the workgroups in flight together write neighbouring cells of the Stokes output
    unsigned rest = blockIdx.x;
    const int k = (int)(rest % (unsigned)a.K);
    rest /= (unsigned)a.K;
    const int chan = (int)(rest % (unsigned)a.n_chan);
    const int g = (int)(rest / (unsigned)a.n_chan);
    const long long first = (long long)g * a.V;          // the segment's first output sample
    const long long start = first - a.n_edge;            // and its first input sample (may be negative)
    const size_t series = ((size_t)chan * a.K + k) * 2;

    for (int pol = 0; pol < 2; pol++) {
        const float2* src = a.in + (series + pol) * (size_t)a.n_time;
        float2* x = lds + pol * STRIDE;
        // pairs of samples that start on an even element of memory: one 16-byte load where both are there
        const int par = (int)(((long long)((uintptr_t)src >> 3) + start) & 1);
        for (int i = tid; i < N / 2 + 1; i += NT) {
            const int n0 = 2 * i - par;
            const long long gl = start + n0;
            if (n0 >= 0 && n0 + 1 < N && gl >= 0 && gl + 1 < a.n_time) {
                const float4 v = *reinterpret_cast<const float4*>(src + gl);
                x[pad(n0)] = make_float2(v.x, v.y);
                x[pad(n0 + 1)] = make_float2(v.z, v.w);
            } else {
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int n = n0 + e;
                    if (n >= 0 && n < N) x[pad(n)] = gl + e >= 0 && gl + e < a.n_time ? src[gl + e] : make_float2(0.f, 0.f);
                }
            }
        }
    }
    __syncthreads();

    forward<M, M>(lds, a.tw, a.chirp + (size_t)chan * N);
    inverse<M, 0>(lds, a.tw);

    const long long left = (long long)a.n_time - first;
    const int count = left < a.V ? (int)left : a.V;     // valid output samples of this segment: >= 1
    if (!STOKES) {
        for (int pol = 0; pol < 2; pol++) {
            float2* dst = reinterpret_cast<float2*>(a.out) + (series + pol) * (size_t)a.n_time + first;
            const float2* y = lds + pol * STRIDE;
            const int par = (int)(((uintptr_t)dst >> 3) & 1);
            for (int i = tid; i < a.V / 2 + 1; i += NT) {
                const int i0 = 2 * i - par;
                if (i0 >= 0 && i0 + 1 < count) {
                    const float2 p = y[pad(a.n_edge + i0)], q = y[pad(a.n_edge + i0 + 1)];
                    *reinterpret_cast<float4*>(dst + i0) = make_float4(p.x, p.y, q.x, q.y);
                } else {
#pragma unroll
                    for (int e = 0; e < 2; e++)
                        if (i0 + e >= 0 && i0 + e < count) dst[i0 + e] = y[pad(a.n_edge + i0 + e)];
                }
            }
        }
    } else {
        // n_int divides V and n_time: whole windows, none shared with another segment.  One lane per window, ascending sums.
        const int windows = count / a.n_int;
        const long long t0 = first / a.n_int;
        const float2 *xs = lds, *ys = lds + STRIDE;
        for (int w = tid; w < windows; w += NT) {
            float si = 0.f, sq = 0.f, su = 0.f, sv = 0.f;
            for (int s = 0; s < a.n_int; s++) {
                const int n = a.n_edge + w * a.n_int + s;
                const float2 x = xs[pad(n)], y = ys[pad(n)];
                const float px = __fadd_rn(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y)), py = __fadd_rn(__fmul_rn(y.x, y.x), __fmul_rn(y.y, y.y));
                const float uu = __fadd_rn(__fmul_rn(x.x, y.x), __fmul_rn(x.y, y.y)), vv = __fsub_rn(__fmul_rn(x.y, y.x), __fmul_rn(x.x, y.y));
                const float ci = __fadd_rn(px, py), cq = __fsub_rn(px, py), cu = __fmul_rn(2.f, uu), cv = __fmul_rn(2.f, vv);
                if (s == 0) {
                    si = ci, sq = cq, su = cu, sv = cv;
                } else {
                    si = __fadd_rn(si, ci), sq = __fadd_rn(sq, cq), su = __fadd_rn(su, cu), sv = __fadd_rn(sv, cv);
                }
            }
            float* o = reinterpret_cast<float*>(a.out) + ((((size_t)(t0 + w)) * a.n_chan + chan) * a.K + k) * 4;
            if (a.out16) {
                *reinterpret_cast<float4*>(o) = make_float4(si, sq, su, sv);
            } else {
                *reinterpret_cast<float2*>(o) = make_float2(si, sq);
                *reinterpret_cast<float2*>(o + 2) = make_float2(su, sv);
            }
        }
    }
}

template <int M>
hipError_t launch_m(const CddArgs& a, bool stokes, unsigned grid, hipStream_t s)
{
    if (stokes) {
        record_launchf("cdd_kernel<%d, true>", M);
        hipLaunchKernelGGL((cdd_kernel<M, true>), dim3(grid), dim3(cdd_threads(M)), 0, s, a);
    } else {
        record_launchf("cdd_kernel<%d, false>", M);
        hipLaunchKernelGGL((cdd_kernel<M, false>), dim3(grid), dim3(cdd_threads(M)), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace

void cdd_twiddles_host(int n_fft, float* table)
{
    const double step = -2.0 * 3.14159265358979323846 / (double)n_fft;
    for (int k = 0; k < n_fft / 2; k++) {
        table[2 * k] = (float)std::cos(step * k);
        table[2 * k + 1] = (float)std::sin(step * k);
    }
}

void cdd_permute_row_host(const float* chirp_row, int n_fft, float* row)
{
    const int m = cdd_log2(n_fft);
    for (int p = 0; p < n_fft; p++) {
        const uint32_t j = cdd_bit_reverse((uint32_t)p, m);
        row[2 * p] = chirp_row[2 * j];
        row[2 * p + 1] = chirp_row[2 * j + 1];
    }
}

hipError_t launch_cdd(const CddLaunch& l, hipStream_t s)
{
    if (!l.in || !l.out || !l.twiddles || !l.chirp || !cdd_supported(l.n_chan, l.n_fft, l.n_edge) || l.K < 1 || l.n_time < 1 || l.n_int < 0 ||
        ((uintptr_t)l.in & 7) || ((uintptr_t)l.out & 7))
        return hipErrorInvalidValue;
    CddArgs a;
    a.in = (const float2*)l.in;
    a.out = l.out;
    a.tw = (const float2*)l.twiddles;
    a.chirp = (const float2*)l.chirp;
    a.n_chan = l.n_chan;
    a.K = l.K;
    a.n_time = l.n_time;
    a.n_edge = l.n_edge;
    a.V = l.n_fft - 2 * l.n_edge;
    a.n_int = l.n_int;
    a.T = l.n_int ? l.n_time / l.n_int : 0;
    a.out16 = ((uintptr_t)l.out & 15) == 0;
    if (l.n_int && (a.V % l.n_int || l.n_time % l.n_int)) return hipErrorInvalidValue;
    const long long groups = cdd_segments(l.n_time, l.n_fft, l.n_edge) * l.n_chan * l.K;
    if (groups > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)groups;
    const bool stokes = l.n_int > 0;
    (void)hipGetLastError();
    switch (cdd_log2(l.n_fft)) {
        case 6: return launch_m<6>(a, stokes, grid, s);
        case 7: return launch_m<7>(a, stokes, grid, s);
        case 8: return launch_m<8>(a, stokes, grid, s);
        case 9: return launch_m<9>(a, stokes, grid, s);
        case 10: return launch_m<10>(a, stokes, grid, s);
        case 11: return launch_m<11>(a, stokes, grid, s);
        default: return launch_m<12>(a, stokes, grid, s);
    }
}

}  // namespace dsabf
