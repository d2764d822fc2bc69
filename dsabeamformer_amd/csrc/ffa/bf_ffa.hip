// bf_ffa.hip -- device code of the periodicity search (contract: docs/PERIODICITY.md section 1; runtime: csrc/bf_ffa.cpp).
//
// ffa_decimate_kernel: a thread owns one decimation group of four consecutive beams.  Its loads are 16 bytes per lane with the 16
// beam-lanes of a row on 256 contiguous bytes (the chunk is beam-contiguous); it adds the group's samples in ascending time, from
// the carried value if an earlier push began the group, and writes the result TRANSPOSED: the series of a slot is
// [trial][beam][time], one (trial, beam) contiguous in time, because that is the order every later step walks it in.
// ffa_detrend_kernel (opt-in, bf_ffa_set_detrend; section 1a): one workgroup = one (trial, beam) of a complete segment; block means,
// their running lower median by rank counting in LDS, and the piecewise linear trend through the block centres subtracted in place.
// ffa_octave_kernel: y_{o+1}[u] = y_o[2u] + y_o[2u + 1], elementwise over a whole octave.
// ffa_search_kernel: one workgroup = one (trial, beam) of one octave, all base periods.  The fold's working set, M rows of p bins
// <= the octave's length, lives in LDS twice (the merge cannot run in place); the first merge level reads the series from memory
// -- 4 L bytes per workgroup, re-read once per p out of the cache -- and every later level, the boxcars and the maxima stay in
// LDS.  A wave's lanes are split into 64 / pw row-lanes of pw >= p bin-lanes (pw a power of two, 64 at most) so that short periods
// do not idle a wave; a cell (row, bin) is one add per level, exactly the adds of the contract.  The maximum carries its cell
// index i * 512 + j: "larger value, or equal value and smaller index" is a total order, so the result does not depend on the
// order of the merges (lane, wave-shuffle, workgroup).
#include "bf_ffa_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

namespace {

constexpr int kBeamLanes = 16, kGroupLanes = 16;   // decimation: 16 lanes x 4 beams, 16 groups per workgroup
constexpr int kDecThreads = kBeamLanes * kGroupLanes;
constexpr int kThreads = 512, kWaves = kThreads / 64;

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__global__ __launch_bounds__(kDecThreads) void ffa_decimate_kernel(const float* __restrict__ chunk, int n_t, int n_beams, int tdec, int c0, int g0,
                                                                   int n_groups, const float* __restrict__ carry_in, float* __restrict__ carry_out,
                                                                   float* __restrict__ y0, int n_seg, int pos0)
{
    const int bgl = threadIdx.x & (kBeamLanes - 1), ul = threadIdx.x / kBeamLanes;
    const int b0 = ((int)blockIdx.x * kBeamLanes + bgl) * 4;
    const int gi = (int)blockIdx.y * kGroupLanes + ul;   // group of this launch
    const int d = (int)blockIdx.z;
    if (b0 >= n_beams || gi >= n_groups) return;
    const int g = g0 + gi;
    const int t_start = g * tdec - c0, t_end = t_start + tdec;
    const int t_stop = t_end < n_t ? t_end : n_t;
    const float* x = chunk + (size_t)d * n_t * n_beams + b0;
    const size_t db = (size_t)d * n_beams + b0;
    float4 acc;
    int t;
    if (t_start < 0) {   // (the group an earlier push began: only g == 0)
        acc = *reinterpret_cast<const float4*>(carry_in + db);
        t = 0;
    } else {
        acc = *reinterpret_cast<const float4*>(x + (size_t)t_start * n_beams);
        t = t_start + 1;
    }
    for (; t < t_stop; t++) acc = add4(acc, *reinterpret_cast<const float4*>(x + (size_t)t * n_beams));
    if (t_end > n_t) {
        *reinterpret_cast<float4*>(carry_out + db) = acc;
    } else {
        float* dst = y0 + db * (size_t)n_seg + (size_t)(pos0 + gi);
        dst[0] = acc.x;
        dst[(size_t)n_seg] = acc.y;
        dst[2 * (size_t)n_seg] = acc.z;
        dst[3 * (size_t)n_seg] = acc.w;
    }
}

__global__ __launch_bounds__(256) void ffa_octave_kernel(const float2* __restrict__ lower, float* __restrict__ upper, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float2 v = lower[i];
        upper[i] = v.x + v.y;
    }
}

// The total order of the running median (docs/PERIODICITY.md section 1a): fp32 bits as a uint32 that sorts like the value, -0 < +0.
__device__ __forceinline__ uint32_t median_key(float v)
{
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float median_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// One workgroup = one (trial, beam): the block means of its segment (a thread per block, a left fold in ascending time), their
// running lower median (a thread per block: the rank of a window's element is the keys less than its own plus the equal keys in
// front of it, so exactly one element of the window has the wanted rank, whatever order they are looked at in), then the piecewise
// linear trend through the block centres subtracted in place (a thread per sample, the series read a second time out of the cache).
// Means (as keys) and medians live in LDS, 8 nb bytes.
__global__ __launch_bounds__(kThreads) void ffa_detrend_kernel(float* __restrict__ y, int n_seg, int lb, float inv_blk, int h)
{
    extern __shared__ uint32_t det_lds[];   // keys of the block means [nb], then the medians [nb] (fp32)
    const int blk = 1 << lb, nb = n_seg >> lb;
    uint32_t* __restrict__ key = det_lds;
    float* __restrict__ med = reinterpret_cast<float*>(det_lds + nb);
    float* __restrict__ s = y + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)n_seg;

    for (int c = threadIdx.x; c < nb; c += kThreads) {
        const float* x = s + ((size_t)c << lb);
        float acc;
        if (blk >= 4) {   // (n_seg % blk == 0 and the series are 16-byte aligned: so is every block)
            const float4 v = *reinterpret_cast<const float4*>(x);
            acc = __fadd_rn(__fadd_rn(__fadd_rn(v.x, v.y), v.z), v.w);
            for (int i = 4; i < blk; i += 4) {
                const float4 w = *reinterpret_cast<const float4*>(x + i);
                acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, w.x), w.y), w.z), w.w);
            }
        } else {
            acc = x[0];
            for (int i = 1; i < blk; i++) acc = __fadd_rn(acc, x[i]);
        }
        key[c] = median_key(__fmul_rn(acc, inv_blk));
    }
    __syncthreads();

    for (int c = threadIdx.x; c < nb; c += kThreads) {
        const int lo = c - h > 0 ? c - h : 0, hi = c + h < nb - 1 ? c + h : nb - 1;
        const int want = (hi - lo) >> 1;   // rank (n - 1) >> 1: the lower median
        uint32_t sel = key[lo];
        for (int i = lo; i <= hi; i++) {
            const uint32_t ki = key[i];
            int rank = 0;
            for (int j = lo; j <= hi; j++) {
                const uint32_t kj = key[j];
                rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
            }
            if (rank == want) {
                sel = ki;
                break;
            }
        }
        med[c] = median_unkey(sel);
    }
    __syncthreads();

    for (int u = threadIdx.x; u < n_seg; u += kThreads) {
        const int k = 2 * u + 1 - blk;
        float trend;
        if (k < 0) {
            trend = med[0];
        } else {
            const int c0 = k >> (lb + 1);
            if (c0 >= nb - 1) {
                trend = med[nb - 1];
            } else {
                const float a = __fmul_rn((float)(k & (2 * blk - 1)), 0.5f * inv_blk);   // (k - 2 blk c0) / (2 blk): dyadic, exact
                const float r0 = med[c0];
                trend = __fadd_rn(r0, __fmul_rn(a, __fsub_rn(med[c0 + 1], r0)));
            }
        }
        s[u] = __fsub_rn(s[u], trend);
    }
}

__device__ __forceinline__ void peak_take(float& bv, int& bi, float v, int idx)
{
    if (v > bv || (v == bv && idx < bi)) {
        bv = v;
        bi = idx;
    }
}

// (s, c) += (x, xc): s + x exactly as a new s and its rounding error (Knuth's branch-free two-sum), the error kept in c.
__device__ __forceinline__ void two_sum(double& s, double& c, double x, double xc)
{
    const double t = s + x;
    const double bp = t - s;
    const double e = (s - (t - bp)) + (x - bp);
    c = (c + xc) + e;
    s = t;
}

// One merge level: groups of g = 2^lev rows of `in` become groups of 2 g rows of `out`.
__device__ __forceinline__ void ffa_merge(const float* __restrict__ in, float* __restrict__ out, int M, int p, int lev, int rs, int n_rs, int jl, int pw)
{
    const int g = 1 << lev;
    for (int R = rs; R < M; R += n_rs) {
        const int i = R & (2 * g - 1);
        const int a = (R - i) + (i >> 1);
        int sh = (i + 1) >> 1;
        if (sh >= p) sh %= p;
        const float* A = in + a * p;
        const float* B = in + (a + g) * p;
        float* O = out + R * p;
        for (int j = jl; j < p; j += pw) {
            int jj = j + sh;
            if (jj >= p) jj -= p;
            O[j] = A[j] + B[jj];
        }
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void ffa_search_kernel(const float* __restrict__ y, int L, int p_lo, int p_hi, int cap, int n_dm, int n_beams,
                                                              bf_ffa_peak* __restrict__ peaks, bf_ffa_stat* __restrict__ stats)
{
    extern __shared__ float work[];   // [2][cap]
    __shared__ float red_v[K][kWaves];
    __shared__ int red_i[K][kWaves];
    __shared__ double red_d[kWaves][4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n_db = (size_t)n_dm * n_beams, db = (size_t)blockIdx.y * n_beams + blockIdx.x;
    const float* __restrict__ s = y + db * (size_t)L;

    if (stats) {   // (octave 0 only)
        // Compensated: the series spans many binades with both signs, and a plain fp64 sum, whatever its order, is only good to
        // n 2^-53 of the sum of MAGNITUDES -- far more than that of a sum that cancels.
        double sum = 0.0, sum_c = 0.0, sq = 0.0, sq_c = 0.0;
        for (int u = tid; u < L; u += kThreads) {
            const double x = (double)s[u];
            two_sum(sum, sum_c, x, 0.0);
            two_sum(sq, sq_c, x * x, 0.0);   // (the square of an fp32 is exact in fp64)
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            two_sum(sum, sum_c, __shfl_xor(sum, off), __shfl_xor(sum_c, off));
            two_sum(sq, sq_c, __shfl_xor(sq, off), __shfl_xor(sq_c, off));
        }
        if (lane == 0) {
            red_d[wave][0] = sum;
            red_d[wave][1] = sum_c;
            red_d[wave][2] = sq;
            red_d[wave][3] = sq_c;
        }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0, a_c = 0.0, q = 0.0, q_c = 0.0;
            for (int w = 0; w < kWaves; w++) {
                two_sum(a, a_c, red_d[w][0], red_d[w][1]);
                two_sum(q, q_c, red_d[w][2], red_d[w][3]);
            }
            stats[db] = bf_ffa_stat{a + a_c, q + q_c};
        }
    }

    for (int p = p_lo; p < p_hi; p++) {
        const int M = ffa_rows(L, p);
        if (M < 2) continue;   // (the host has refused this; uniform)
        const int logM = 31 - __clz(M);
        const int pw_log = p >= 64 ? 6 : 32 - __clz(p - 1);
        const int pw = 1 << pw_log, jl = lane & (pw - 1);
        const int rs = wave * (64 >> pw_log) + (lane >> pw_log), n_rs = kWaves * (64 >> pw_log);

        ffa_merge(s, work, M, p, 0, rs, n_rs, jl, pw);
        __syncthreads();
        for (int lev = 1; lev < logM; lev++) {
            ffa_merge(work + ((lev - 1) & 1) * cap, work + (lev & 1) * cap, M, p, lev, rs, n_rs, jl, pw);
            __syncthreads();
        }
        int cur = (logM - 1) & 1;

        float bv[K];
        int bi[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            bv[k] = -INFINITY;
            bi[k] = 0;   // a column of NaN alone never passes peak_take: its record stays at cell (0, 0), inside M x p
        }
        if (K == 1) {
            const float* src = work + cur * cap;
            for (int R = rs; R < M; R += n_rs)
                for (int j = jl; j < p; j += pw) peak_take(bv[0], bi[0], src[R * p + j], R * 512 + j);
        }
#pragma unroll
        for (int k = 1; k < K; k++) {   // C_k from C_{k-1}; the maximum of C_{k-1} is taken from the left operand, every cell once
            const float* src = work + cur * cap;
            float* dst = work + (cur ^ 1) * cap;
            const int half = 1 << (k - 1);
            for (int R = rs; R < M; R += n_rs) {
                for (int j = jl; j < p; j += pw) {
                    int jj = j + half;
                    if (jj >= p) jj -= p;
                    const float v0 = src[R * p + j];
                    peak_take(bv[k - 1], bi[k - 1], v0, R * 512 + j);
                    const float v = v0 + src[R * p + jj];
                    if (k < K - 1)
                        dst[R * p + j] = v;
                    else
                        peak_take(bv[K - 1], bi[K - 1], v, R * 512 + j);
                }
            }
            if (k < K - 1) {
                __syncthreads();
                cur ^= 1;
            }
        }

#pragma unroll
        for (int k = 0; k < K; k++) {
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) peak_take(bv[k], bi[k], __shfl_xor(bv[k], off), __shfl_xor(bi[k], off));
            if (lane == 0) {
                red_v[k][wave] = bv[k];
                red_i[k][wave] = bi[k];
            }
        }
        __syncthreads();   // (also: every read of `work` is over before the next p writes it)
        if (tid < K) {
            float v = red_v[tid][0];
            int idx = red_i[tid][0];
            for (int w = 1; w < kWaves; w++) peak_take(v, idx, red_v[tid][w], red_i[tid][w]);
            bf_ffa_peak r;
            r.value = v;
            r.shift = (uint16_t)(idx >> 9);
            r.bin = (uint16_t)(idx & 511);
            peaks[((size_t)(p - p_lo) * K + tid) * n_db + db] = r;
        }
    }
}

template <int K>
hipError_t launch_search_octave(const float* y, int L, int p_lo, int p_hi, int n_dm, int n_beams, bf_ffa_peak* peaks, bf_ffa_stat* stats, hipStream_t stream)
{
    int cap = 0;
    for (int p = p_lo; p < p_hi; p++) cap = cap > ffa_rows(L, p) * p ? cap : ffa_rows(L, p) * p;
    cap = (cap + 3) & ~3;
    const size_t lds = 2 * (size_t)cap * sizeof(float);
    auto kern = ffa_search_kernel<K>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    record_launchf("ffa_search_kernel<%d>", K);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_beams, (unsigned)n_dm), dim3(kThreads), lds, stream, y, L, p_lo, p_hi, cap, n_dm, n_beams, peaks, stats);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ffa_decimate(const float* d_chunk, int n_dm, int n_t, int n_beams, int tdec, int c0, int g0, int n_groups, const float* carry_in,
                               float* carry_out, float* y0, int n_seg, int pos0, hipStream_t stream)
{
    if (n_dm <= 0 || n_dm > 65535 || n_t <= 0 || n_beams <= 0 || n_beams % 4 || tdec < 1 || tdec > kFfaMaxDec || c0 < 0 || c0 >= tdec || g0 < 0 ||
        n_groups <= 0 || n_groups > kFfaMaxSeg + 1 || pos0 < 0 || n_seg < 1 || n_seg > kFfaMaxSeg || ((uintptr_t)d_chunk & 15) || carry_in == carry_out)
        return hipErrorInvalidValue;
    // every group of the launch starts inside the chunk (or in the carry), and the complete ones stay inside the segment
    const long long last_start = (long long)(g0 + n_groups - 1) * tdec - c0;
    const long long n_complete = ((long long)c0 + n_t) / tdec;   // complete groups of the whole push
    const long long in_seg = (g0 + n_groups <= n_complete ? n_groups : n_complete - g0);
    if (last_start >= n_t || in_seg < 0 || pos0 + in_seg > n_seg) return hipErrorInvalidValue;
    (void)hipGetLastError();
    const dim3 grid((unsigned)((n_beams + 4 * kBeamLanes - 1) / (4 * kBeamLanes)), (unsigned)((n_groups + kGroupLanes - 1) / kGroupLanes), (unsigned)n_dm);
    record_launch("ffa_decimate_kernel");
    hipLaunchKernelGGL(ffa_decimate_kernel, grid, dim3(kDecThreads), 0, stream, d_chunk, n_t, n_beams, tdec, c0, g0, n_groups, carry_in,
                       carry_out, y0, n_seg, pos0);
    return hipGetLastError();
}

hipError_t launch_ffa_detrend(float* y0, int n_dm, int n_beams, int n_seg, int blk, int win, hipStream_t stream)
{
    if (n_dm <= 0 || n_dm > 65535 || n_beams <= 0 || n_seg < 1 || n_seg > kFfaMaxSeg || blk < 1 || blk > kFfaMaxDetrendBlk || (blk & (blk - 1)) ||
        n_seg % blk || win < 1 || win > kFfaMaxDetrendWin || !(win & 1) || ((uintptr_t)y0 & 15))
        return hipErrorInvalidValue;
    int lb = 0;
    while ((1 << lb) < blk) lb++;
    const size_t lds = 2 * (size_t)(n_seg >> lb) * sizeof(float);   // 128 KiB at most (blk 1, n_seg 16384)
    (void)hipGetLastError();
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ffa_detrend_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    record_launch("ffa_detrend_kernel");
    hipLaunchKernelGGL(ffa_detrend_kernel, dim3((unsigned)n_beams, (unsigned)n_dm), dim3(kThreads), lds, stream, y0, n_seg, lb, 1.0f / (float)blk,
                       (win - 1) / 2);
    return hipGetLastError();
}

hipError_t launch_ffa_search(float* slot, int n_dm, int n_beams, int n_seg, int n_oct, int p_lo, int p_hi, int n_widths, bf_ffa_peak* peaks,
                             bf_ffa_stat* stats, hipStream_t stream)
{
    if (n_dm <= 0 || n_dm > 65535 || n_beams <= 0 || n_beams % 4 || n_seg < 1 || n_seg > kFfaMaxSeg || n_oct < 1 || n_oct > kFfaMaxOct ||
        n_seg % (1 << (n_oct - 1)) || p_lo < kFfaMinPeriod || p_hi <= p_lo || p_hi > kFfaMaxPeriod || n_widths < 1 || n_widths > kFfaMaxWidths ||
        (1 << (n_widths - 1)) > p_lo / 2)
        return hipErrorInvalidValue;
    for (int o = 0; o < n_oct; o++)
        for (int p = p_lo; p < p_hi; p++)
            if (ffa_rows(n_seg >> o, p) < 2) return hipErrorInvalidValue;
    const size_t n_db = (size_t)n_dm * n_beams, n_rec = (size_t)(p_hi - p_lo) * n_widths * n_db;
    (void)hipGetLastError();
    for (int o = 0; o < n_oct; o++) {
        const int L = n_seg >> o;
        float* y = slot + ffa_octave_offset(o, n_seg, n_db);
        if (o > 0) {
            const size_t n = n_db * (size_t)L;
            record_launch("ffa_octave_kernel");
            hipLaunchKernelGGL(ffa_octave_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                               reinterpret_cast<const float2*>(slot + ffa_octave_offset(o - 1, n_seg, n_db)), y, n);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
        bf_ffa_peak* pk = peaks + (size_t)o * n_rec;
        bf_ffa_stat* st = o == 0 ? stats : nullptr;
        hipError_t e = hipSuccess;
        switch (n_widths) {
        case 1: e = launch_search_octave<1>(y, L, p_lo, p_hi, n_dm, n_beams, pk, st, stream); break;
        case 2: e = launch_search_octave<2>(y, L, p_lo, p_hi, n_dm, n_beams, pk, st, stream); break;
        case 3: e = launch_search_octave<3>(y, L, p_lo, p_hi, n_dm, n_beams, pk, st, stream); break;
        case 4: e = launch_search_octave<4>(y, L, p_lo, p_hi, n_dm, n_beams, pk, st, stream); break;
        case 5: e = launch_search_octave<5>(y, L, p_lo, p_hi, n_dm, n_beams, pk, st, stream); break;
        default: e = launch_search_octave<6>(y, L, p_lo, p_hi, n_dm, n_beams, pk, st, stream); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dsabf
