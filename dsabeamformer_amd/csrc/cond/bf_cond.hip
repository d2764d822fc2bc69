// bf_cond.hip -- device code of the conditioning stage in front of the DM stage (include/dsabf.h: bf_cond_*; the contract, to the
// bit: docs/CONDITIONING.md section 1).  Three kernels per push:
//   cond_totals_kernel   a workgroup per channel, lanes along b, four row groups: the segments' totals (32 rows each, fp64, ascending)
//                        into a scratch [segment][f][b]; one thread per cell adds them in ascending order into set push % W of the
//                        ring and adds the window oldest first: mu, var, mu32, r32; wave 0 forms cm[f] and cv[f] in the OSUM
//                        order (lane l owns the beams l, l + 64, ..., six butterfly steps are the six halving steps, as in
//                        cal/bf_cal.hip);
//   cond_summary_kernel  one workgroup: the mask, the two lower medians by rank counting, n_good and inv;
//   cond_apply_kernel    one thread per beam of two rows: per (t, b) the ascending fp32 sum over the unmasked channels, then the store.
// The library is built with -ffp-contract=off and the pragma below says so again: NO fused multiply-add anywhere in this file, one
// rounding per written operation.  Plain C++ with vector loads and stores; no inline assembly, no atomics.
#include "bf_cond_kernels.h"
#include "../rec/bf_launch_record.h"

#pragma clang fp contract(off)

namespace dsabf {
namespace {

constexpr int kCellThreads = 256;
constexpr int kTotalsGroups = 4;                              // row groups of the totals kernel: group g walks the segments g, g + 4, ...
constexpr int kTotalsThreads = kTotalsGroups * kCellThreads;
constexpr int kSummaryThreads = 1024;
constexpr int kSummaryWaves = kSummaryThreads / 64;
constexpr int kSummaryLdsChannels = 2048;                     // the medians' values live in LDS up to this many channels

// the six halving steps of OSUM on the 64 partial sums of a wave; every lane returns the result
__device__ __forceinline__ double halve(double s)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) s = s + __shfl_xor(s, w, 64);
    return s;
}

__global__ __launch_bounds__(kTotalsThreads) void cond_totals_kernel(const float* __restrict__ rows, int n_rows, int n_freq, int n_beams, CondBuffers b,
                                                                     int window, int cur_set, int n_sets, double n_window)
{
    const int f = blockIdx.x, bl = threadIdx.x & (kCellThreads - 1), g = threadIdx.x / kCellThreads;
    const size_t n_cells = (size_t)n_freq * n_beams;
    const int n_seg = (n_rows + kCondSegment - 1) / kCondSegment;
    // (a) a segment's sums: from +0.0 in ascending t
    for (int bm = bl; bm < n_beams; bm += kCellThreads) {
        const size_t c = (size_t)f * n_beams + bm;
        for (int sg = g; sg < n_seg; sg += kTotalsGroups) {
            const int t0 = sg * kCondSegment;
            const float* p = rows + (size_t)t0 * n_cells + c;
            double s = 0.0, q = 0.0;
            if (n_rows - t0 >= kCondSegment) {
                float v[kCondSegment];   // all 32 loads in flight before the first add
#pragma unroll
                for (int i = 0; i < kCondSegment; i++) v[i] = p[(size_t)i * n_cells];
#pragma unroll
                for (int i = 0; i < kCondSegment; i++) {
                    const double d = (double)v[i];
                    s = s + d;
                    q = q + d * d;   // (double)x (double)x is exact
                }
            } else {
                for (int i = 0; i < n_rows - t0; i++) {
                    const double d = (double)p[(size_t)i * n_cells];
                    s = s + d;
                    q = q + d * d;
                }
            }
            b.seg[(size_t)sg * n_cells + c] = CondStat{s, q};
        }
    }
    __syncthreads();   // (the segments of this channel were written by this workgroup: visible to it behind the barrier)
    if (g == 0) {
        for (int bm = bl; bm < n_beams; bm += kCellThreads) {
            const size_t c = (size_t)f * n_beams + bm;
            // the push totals: the segments in ascending order, from +0.0
            double S = 0.0, Q = 0.0;
            for (int sg = 0; sg < n_seg; sg++) {
                const CondStat w = b.seg[(size_t)sg * n_cells + c];
                S = S + w.sum;
                Q = Q + w.sumsq;
            }
            b.ring[(size_t)cur_set * n_cells + c] = CondStat{S, Q};
            // (b) the window: the n_sets most recent pushes, oldest first, this one last
            double Sw = 0.0, Qw = 0.0;
            const int oldest = (cur_set - (n_sets - 1) + window) % window;
            for (int i = 0; i < n_sets - 1; i++) {
                const CondStat w = b.ring[(size_t)((oldest + i) % window) * n_cells + c];
                Sw = Sw + w.sum;
                Qw = Qw + w.sumsq;
            }
            Sw = Sw + S;
            Qw = Qw + Q;
            const double mu = Sw / n_window;
            const double mm = mu * mu;
            const double var = Qw / n_window - mm;
            const bool live = var > mm * 0x1p-40;
            b.cell_mu[c] = mu;
            b.cell_var[c] = var > 0.0 ? var : 0.0;
            b.mr32[c] = float2{(float)mu, live ? (float)(1.0 / sqrt(var)) : 0.0f};
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // (c) cm, cv in the OSUM order: lane l owns the beams l, l + 64, ...
        double pm = 0.0, pv = 0.0;
        for (int i = threadIdx.x; i < n_beams; i += 64) {
            pm = pm + b.cell_mu[(size_t)f * n_beams + i];
            pv = pv + b.cell_var[(size_t)f * n_beams + i];
        }
        const double cm = halve(pm) / (double)n_beams, cv = halve(pv) / (double)n_beams;
        if (threadIdx.x == 0) {
            b.cm[f] = cm;
            b.cv[f] = cv;
        }
    }
}

// Lower median of the non-NaN entries of v[0 .. n): element (m - 1) / 2 of the m sorted values, found by rank counting (v_i is
// it iff #{v_j < v_i} <= r < #{v_j <= v_i}; ties write the same value).  *out stays NaN when there is none.
__device__ __forceinline__ void lower_median(const double* v, int n, double* out)
{
    if (threadIdx.x == 0) *out = __builtin_nan("");
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kSummaryThreads) {
        const double vi = v[i];
        if (!(vi == vi)) continue;
        int m = 0, lt = 0, le = 0;
#pragma unroll 8
        for (int j = 0; j < n; j++) {
            const double vj = v[j];
            m += vj == vj;
            lt += vj < vi;
            le += vj <= vi;
        }
        const int r = (m - 1) / 2;
        if (lt <= r && r < le) *out = vi;
    }
    __syncthreads();
}

// The automatic mask over q[0 .. n) (NaN: not eligible), with `dev` as room for |q - med|: high side only.
__device__ __forceinline__ void auto_mask(const double* q, double* dev, int n, double k_auto, uint8_t* mask, double* s_med, double* s_mad)
{
    lower_median(q, n, s_med);
    const double med = *s_med;
    for (int f = threadIdx.x; f < n; f += kSummaryThreads) dev[f] = fabs(q[f] - med);   // (NaN stays NaN)
    __syncthreads();
    lower_median(dev, n, s_mad);
    const double mad = *s_mad;
    if (mad > 0.0) {
        const double limit = med + k_auto * mad;
        for (int f = threadIdx.x; f < n; f += kSummaryThreads)
            if (q[f] > limit) mask[f] = 1;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kSummaryThreads) void cond_summary_kernel(int n_freq, CondBuffers b, double k_auto)
{
    __shared__ double s_q[kSummaryLdsChannels], s_dev[kSummaryLdsChannels];
    __shared__ double s_med, s_mad;
    __shared__ int s_cnt[kSummaryWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool in_lds = n_freq <= kSummaryLdsChannels;
    // the static mask and the channels without a positive mean; q of the others
    for (int f = tid; f < n_freq; f += kSummaryThreads) {
        const double cm = b.cm[f], cv = b.cv[f];
        const bool masked = b.static_mask[f] != 0 || !(cm > 0.0 && cv > 0.0);
        const double q = masked ? __builtin_nan("") : cv / (cm * cm);
        b.mask[f] = masked ? 1 : 0;
        if (in_lds)
            s_q[f] = q;
        else
            b.q[f] = q;
    }
    __syncthreads();
    if (k_auto > 0.0) {
        if (in_lds)
            auto_mask(s_q, s_dev, n_freq, k_auto, b.mask, &s_med, &s_mad);
        else
            auto_mask(b.q, b.dev, n_freq, k_auto, b.mask, &s_med, &s_mad);
    }
    int good = 0;   // (an integer count: its order does not matter)
    for (int f = tid; f < n_freq; f += kSummaryThreads) good += b.mask[f] == 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) good += __shfl_xor(good, w, 64);
    if (lane == 0) s_cnt[wave] = good;
    __syncthreads();
    if (tid == 0) {
        int n_good = 0;
        for (int w = 0; w < kSummaryWaves; w++) n_good += s_cnt[w];
        b.params->n_good = n_good;
        b.params->inv = n_good ? (float)(1.0 / (double)n_good) : 0.0f;
    }
}

// (d) + (e).  A thread owns one beam of kApplyRows consecutive rows and walks f twice: {mu32, r32} of a channel is loaded once for
// those rows; a row's slab is n_freq dwords a row of beams apart, and it is read a second time for the store (from cache where it
// still is there: docs/CONDITIONING.md section 6).  Neighbouring lanes are neighbouring beams: every load and store of a wave is one contiguous run.  No branch in either loop, so that the loads of
// sixteen channels are in flight together; a masked channel's y is dropped by a select.  Every (t, b) sum is still one register,
// ascending f, from +0.0f.
constexpr int kApplyRows = 2;
constexpr int kApplyBatch = 16;   // channels whose loads are in flight together in the store pass

template <bool ZERO_DM>
__global__ __launch_bounds__(kCellThreads) void cond_apply_kernel(float* __restrict__ rows, int n_rows, int n_freq, int n_beams,
                                                                  const float2* __restrict__ mr32, const uint8_t* __restrict__ mask,
                                                                  const CondParams* __restrict__ params)
{
    const size_t idx = (size_t)blockIdx.x * kCellThreads + threadIdx.x;
    const size_t tg = idx / (size_t)n_beams;                    // the thread's group of rows
    const int bm = (int)(idx - tg * (size_t)n_beams);
    const size_t t0 = tg * kApplyRows;
    if (t0 >= (size_t)n_rows) return;
    const size_t row_floats = (size_t)n_freq * n_beams;
    float* p[kApplyRows];
    bool has[kApplyRows];
#pragma unroll
    for (int k = 0; k < kApplyRows; k++) {
        has[k] = t0 + k < (size_t)n_rows;
        p[k] = rows + (has[k] ? t0 + k : t0) * row_floats + bm;   // (a row past the end: row t0 is read again, nothing is stored)
    }
    const float2* mr = mr32 + bm;
    float z[kApplyRows];
#pragma unroll
    for (int k = 0; k < kApplyRows; k++) z[k] = 0.0f;
    if (ZERO_DM) {
#pragma unroll 16
        for (int f = 0; f < n_freq; f++) {
            const size_t o = (size_t)f * n_beams;
            const float2 c = mr[o];
            const bool masked = mask[f] != 0;
#pragma unroll
            for (int k = 0; k < kApplyRows; k++) {
                const float y = c.y == 0.0f ? 0.0f : (p[k][o] - c.x) * c.y;
                z[k] = masked ? z[k] : z[k] + y;   // (a masked channel is not a term of the sum)
            }
        }
        const float inv = params->inv;
#pragma unroll
        for (int k = 0; k < kApplyRows; k++) z[k] = z[k] * inv;
    }
    // The store pass in batches of kApplyBatch channels: ALL of a batch's loads first, then its stores.  Written as one loop the
    // compiler must keep every load behind the store in front of it (the thread's rows are one array to it), and the pass becomes a
    // chain of n_freq memory round trips.
    int f = 0;
    for (; f + kApplyBatch <= n_freq; f += kApplyBatch) {
        float x[kApplyRows][kApplyBatch];
        float2 c[kApplyBatch];
#pragma unroll
        for (int j = 0; j < kApplyBatch; j++) {
            const size_t o = (size_t)(f + j) * n_beams;
            c[j] = mr[o];
#pragma unroll
            for (int k = 0; k < kApplyRows; k++) x[k][j] = p[k][o];
        }
#pragma unroll
        for (int j = 0; j < kApplyBatch; j++) {
            const size_t o = (size_t)(f + j) * n_beams;
            const bool masked = mask[f + j] != 0;
#pragma unroll
            for (int k = 0; k < kApplyRows; k++) {
                const float y = c[j].y == 0.0f ? 0.0f : (x[k][j] - c[j].x) * c[j].y;
                if (has[k]) p[k][o] = masked ? 0.0f : (ZERO_DM ? y - z[k] : y);
            }
        }
    }
    for (; f < n_freq; f++) {   // the ragged end
        const size_t o = (size_t)f * n_beams;
        const float2 c = mr[o];
        const bool masked = mask[f] != 0;
#pragma unroll
        for (int k = 0; k < kApplyRows; k++) {
            const float y = c.y == 0.0f ? 0.0f : (p[k][o] - c.x) * c.y;
            if (has[k]) p[k][o] = masked ? 0.0f : (ZERO_DM ? y - z[k] : y);
        }
    }
}

}  // namespace

hipError_t launch_cond_push(float* d_rows, int n_rows, int n_freq, int n_beams, const CondBuffers& buf, int window, int cur_set, int n_sets,
                            uint64_t n_window, bool zero_dm, double k_auto, hipStream_t stream)
{
    record_launch("cond_totals_kernel");
    cond_totals_kernel<<<dim3((unsigned)n_freq), dim3(kTotalsThreads), 0, stream>>>(d_rows, n_rows, n_freq, n_beams, buf, window, cur_set, n_sets,
                                                                                    (double)n_window);
    record_launch("cond_summary_kernel");
    cond_summary_kernel<<<dim3(1), dim3(kSummaryThreads), 0, stream>>>(n_freq, buf, k_auto);
    const size_t n_threads = (size_t)((n_rows + kApplyRows - 1) / kApplyRows) * n_beams;
    const dim3 grid((unsigned)((n_threads + kCellThreads - 1) / kCellThreads));
    if (zero_dm) {
        record_launch("cond_apply_kernel<true>");
        cond_apply_kernel<true><<<grid, dim3(kCellThreads), 0, stream>>>(d_rows, n_rows, n_freq, n_beams, buf.mr32, buf.mask, buf.params);
    } else {
        record_launch("cond_apply_kernel<false>");
        cond_apply_kernel<false><<<grid, dim3(kCellThreads), 0, stream>>>(d_rows, n_rows, n_freq, n_beams, buf.mr32, buf.mask, buf.params);
    }
    return hipGetLastError();
}

}  // namespace dsabf
