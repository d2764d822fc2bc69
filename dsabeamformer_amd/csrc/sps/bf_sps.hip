// bf_sps.hip -- device code of the single-pulse search stage (include/dsabf.h: bf_sps_*; contract: docs/SINGLE_PULSE.md).
//
// Input: one chunk x[d][t][b] of the DM stage.  For every boxcar width w_k = 2^k, k < K, the balanced pairwise tree
//   S_0[t] = x[t],   S_k[t] = S_{k-1}[t] + S_{k-1}[t - 2^(k-1)]          (fp32, one rounding per add)
// and per (k, d, b) the maximum of S_k over the chunk's times with the FIRST time attaining it; per (d, b) the fp64 sum and
// sum of squares of x.
//
// sps_tile_kernel: one workgroup = one trial x 128 output times x 64 beams.  A lane owns four consecutive beams (one 16-byte
// load per row: the beam-contiguous layout of the chunk), the 16 lanes of a row 256 contiguous bytes, the 16 row-lanes of the
// workgroup the rows r, r + 16, r + 32, ... of the tile -- in registers.  In front of the 128 output rows sit the 2^(K-1) - 1 halo
// rows the widest tree reaches back to: from the chunk itself or, in front of its first time, from the tail the stage carries.
// A level's partner row r - 2^(k-1) belongs to another row-lane while 2^(k-1) < 16 -- those four levels go through LDS -- and
// to the same lane from there on: levels 5 .. 7 are register adds.  Every chunk element is loaded once per tile that needs it
// (once, plus the halo rows of the next tile).
// sps_finish_kernel: combines the tiles' records in ascending tile order (a later tile wins only with a LARGER value: ties keep
// the first time), sums the tiles' statistics, and writes the tail for the next push.
#include "bf_sps_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

namespace {

constexpr int kT = kSpsTileTimes;
constexpr int kRowLanes = 16;   // row-lanes of a workgroup: thread (tl, bgl) owns rows tl, tl + 16, ...
constexpr int kBeamLanes = 16;  // 16 lanes x 4 beams = 64 beams per workgroup
constexpr int kThreads = kRowLanes * kBeamLanes;

// first occurrence of the maximum: a record without a time (t < 0) loses to any; a later time wins only with a larger value
__device__ __forceinline__ void peak_take(float& bv, int& bt, float v, int t)
{
    if (bt < 0 || v > bv) {
        bv = v;
        bt = t;
    }
}
// the same for two records of unordered times: equal values keep the smaller time
__device__ __forceinline__ void peak_merge(float& bv, int& bt, float v, int t)
{
    if (t >= 0 && (bt < 0 || v > bv || (v == bv && t < bt))) {
        bv = v;
        bt = t;
    }
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// Level k of the tree for the rows a lane owns (v: S_{k-1} on entry, S_k on return), then the lane's peak of S_k -- and, at level 0,
// its share of the statistics.  A template over k (not a loop): every register index below is a compile-time constant.
template <int K, int k>
__device__ __forceinline__ void sps_level(float4 (&v)[(kT + (1 << (K - 1)) - 1 + kRowLanes - 1) / kRowLanes], float4 (&bv)[K], int4 (&bt)[K],
                                          double (&sum)[4], double (&sq)[4], float4* lds, int tl, int bgl, int t_first, int n_t,
                                          unsigned long long seen)
{
    constexpr int H = (1 << (K - 1)) - 1;
    constexpr int ROWS = kT + H;
    constexpr int NI = (ROWS + kRowLanes - 1) / kRowLanes;
    constexpr int dist = (1 << k) >> 1;   // 2^(k-1); 0 at level 0
    if constexpr (k > 0 && dist < kRowLanes) {   // the partner row is another row-lane's: through LDS
        if (k > 1) __syncthreads();              // (the reads of the level before)
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int r = tl + kRowLanes * i;
            if (r < ROWS) lds[r * kBeamLanes + bgl] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int r = tl + kRowLanes * i;
            if (r < ROWS && r >= dist) v[i] = add4(v[i], lds[(r - dist) * kBeamLanes + bgl]);
        }
    } else if constexpr (k > 0) {                // ... this lane's own, dist / 16 registers back (descending: v[i - m] is still level k - 1)
        constexpr int m = dist / kRowLanes;
#pragma unroll
        for (int i = NI - 1; i >= m; i--) v[i] = add4(v[i], v[i - m]);
    }
    // rows of the tile's output times that the chunk has and at which S_k exists; ascending: ties keep the first
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int r = tl + kRowLanes * i, t = t_first + r;
        if (r >= H && r < ROWS && t < n_t && seen + (unsigned long long)t >= (1ull << k) - 1) {
            peak_take(bv[k].x, bt[k].x, v[i].x, t);
            peak_take(bv[k].y, bt[k].y, v[i].y, t);
            peak_take(bv[k].z, bt[k].z, v[i].z, t);
            peak_take(bv[k].w, bt[k].w, v[i].w, t);
            if constexpr (k == 0) {
                const double x[4] = {(double)v[i].x, (double)v[i].y, (double)v[i].z, (double)v[i].w};
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    sum[c] += x[c];
                    sq[c] += x[c] * x[c];
                }
            }
        }
    }
    if constexpr (k + 1 < K) sps_level<K, k + 1>(v, bv, bt, sum, sq, lds, tl, bgl, t_first, n_t, seen);
}

template <int K>
__global__ __launch_bounds__(kThreads) void sps_tile_kernel(const float* __restrict__ chunk, const float* __restrict__ tail_in, int n_dm,
                                                            int n_t, int n_beams, unsigned long long seen,
                                                            bf_sps_peak* __restrict__ part_peaks, bf_sps_stat* __restrict__ part_stats)
{
    constexpr int H = (1 << (K - 1)) - 1;
    constexpr int ROWS = kT + H;
    constexpr int NI = (ROWS + kRowLanes - 1) / kRowLanes;
    extern __shared__ float4 lds[];   // [ROWS][16] float4 while the levels run, the workgroup's reduction afterwards

    const int tid = threadIdx.x, bgl = tid & (kBeamLanes - 1), tl = tid / kBeamLanes;
    const int b0 = (blockIdx.x * kBeamLanes + bgl) * 4;
    const bool ok = b0 < n_beams;   // (n_beams is a multiple of 4: a lane's four beams are all inside or all outside)
    const int ti = blockIdx.y, d = blockIdx.z;
    const int t_first = ti * kT - H;   // chunk time of row 0

    float4 v[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int r = tl + kRowLanes * i, t = t_first + r;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && r < ROWS) {
            if (t >= 0) {
                if (t < n_t) v[i] = *reinterpret_cast<const float4*>(chunk + ((size_t)d * n_t + t) * n_beams + b0);
            } else if (H > 0) {
                v[i] = *reinterpret_cast<const float4*>(tail_in + ((size_t)d * H + (H + t)) * n_beams + b0);
            }
        }
    }

    float4 bv[K];
    int4 bt[K];
    double sum[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < K; k++) {
        bv[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        bt[k] = make_int4(-1, -1, -1, -1);
    }

    sps_level<K, 0>(v, bv, bt, sum, sq, lds, tl, bgl, t_first, n_t, seen);

    // the four row-lanes of a wave: lanes l, l ^ 16, l ^ 32, l ^ 48 share the beams
#pragma unroll
    for (int off = kBeamLanes; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            peak_merge(bv[k].x, bt[k].x, __shfl_xor(bv[k].x, off), __shfl_xor(bt[k].x, off));
            peak_merge(bv[k].y, bt[k].y, __shfl_xor(bv[k].y, off), __shfl_xor(bt[k].y, off));
            peak_merge(bv[k].z, bt[k].z, __shfl_xor(bv[k].z, off), __shfl_xor(bt[k].z, off));
            peak_merge(bv[k].w, bt[k].w, __shfl_xor(bv[k].w, off), __shfl_xor(bt[k].w, off));
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            sum[c] += __shfl_xor(sum[c], off);
            sq[c] += __shfl_xor(sq[c], off);
        }
    }
    // ... and the workgroup's four waves through LDS
    constexpr int kWaves = kThreads / 64;
    float4* red_v = lds;                                                   // [K][4 waves][16]
    int4* red_t = reinterpret_cast<int4*>(lds + K * kWaves * kBeamLanes);  // [K][4 waves][16]
    double* red_s = reinterpret_cast<double*>(lds + 2 * K * kWaves * kBeamLanes);   // [4 waves][16][4 beams]{sum, sumsq}
    const int wave = tid / 64;
    __syncthreads();   // (the level reads)
    if ((tid & 63) < kBeamLanes) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            red_v[(k * kWaves + wave) * kBeamLanes + bgl] = bv[k];
            red_t[(k * kWaves + wave) * kBeamLanes + bgl] = bt[k];
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            red_s[((wave * kBeamLanes + bgl) * 4 + c) * 2 + 0] = sum[c];
            red_s[((wave * kBeamLanes + bgl) * 4 + c) * 2 + 1] = sq[c];
        }
    }
    __syncthreads();
    if (!ok) return;
    if (tid < K * kBeamLanes) {
        const int k = tid / kBeamLanes;
        float4 a = red_v[(k * kWaves) * kBeamLanes + bgl];
        int4 at = red_t[(k * kWaves) * kBeamLanes + bgl];
        for (int w = 1; w < kWaves; w++) {
            const float4 o = red_v[(k * kWaves + w) * kBeamLanes + bgl];
            const int4 ot = red_t[(k * kWaves + w) * kBeamLanes + bgl];
            peak_merge(a.x, at.x, o.x, ot.x);
            peak_merge(a.y, at.y, o.y, ot.y);
            peak_merge(a.z, at.z, o.z, ot.z);
            peak_merge(a.w, at.w, o.w, ot.w);
        }
        bf_sps_peak* dst = part_peaks + (((size_t)ti * K + k) * n_dm + d) * n_beams + b0;
        dst[0] = bf_sps_peak{a.x, at.x};
        dst[1] = bf_sps_peak{a.y, at.y};
        dst[2] = bf_sps_peak{a.z, at.z};
        dst[3] = bf_sps_peak{a.w, at.w};
    } else if (tid >= kThreads - kBeamLanes) {   // (K <= 8: the last 16 threads are never among the K * 16 above)
        bf_sps_stat* dst = part_stats + ((size_t)ti * n_dm + d) * n_beams + b0;
        for (int c = 0; c < 4; c++) {
            double s = 0, q = 0;
            for (int w = 0; w < kWaves; w++) {
                s += red_s[((w * kBeamLanes + bgl) * 4 + c) * 2 + 0];
                q += red_s[((w * kBeamLanes + bgl) * 4 + c) * 2 + 1];
            }
            dst[c] = bf_sps_stat{s, q};
        }
    }
}

// Flat index space: [0, n_peak) records (k, d, b); then n_stat statistics (d, b); then n_tail float4s of the next push's tail.
__global__ __launch_bounds__(256) void sps_finish_kernel(const float* __restrict__ chunk, const float* __restrict__ tail_in,
                                                         float* __restrict__ tail_out, const bf_sps_peak* __restrict__ part_peaks,
                                                         const bf_sps_stat* __restrict__ part_stats, bf_sps_peak* __restrict__ peaks,
                                                         bf_sps_stat* __restrict__ stats, int n_tiles, int n_dm, int n_t, int n_beams, int K,
                                                         int H)
{
    const size_t n_stat = (size_t)n_dm * n_beams, n_peak = (size_t)K * n_stat, n_tail = (size_t)n_dm * H * (n_beams / 4);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_peak) {
        bf_sps_peak best{-INFINITY, -1};
        for (int ti = 0; ti < n_tiles; ti++) {   // ascending times: a later tile wins only with a larger value
            const bf_sps_peak p = part_peaks[(size_t)ti * n_peak + i];
            if (p.t_end >= 0 && (best.t_end < 0 || p.value > best.value)) best = p;
        }
        peaks[i] = best;
        return;
    }
    i -= n_peak;
    if (i < n_stat) {
        double s = 0, q = 0;
        for (int ti = 0; ti < n_tiles; ti++) {
            s += part_stats[(size_t)ti * n_stat + i].sum;
            q += part_stats[(size_t)ti * n_stat + i].sumsq;
        }
        stats[i] = bf_sps_stat{s, q};
        return;
    }
    i -= n_stat;
    if (i < n_tail) {   // tail row j of the next push = time n_t - H + j of this one: from the chunk, or further back from this push's tail
        const int b4 = (int)(i % (size_t)(n_beams / 4));
        const int j = (int)((i / (size_t)(n_beams / 4)) % (size_t)H), d = (int)(i / ((size_t)(n_beams / 4) * H));
        const int t = n_t - H + j;   // >= -H + 1
        const float4 x = t >= 0 ? *reinterpret_cast<const float4*>(chunk + ((size_t)d * n_t + t) * n_beams + 4 * b4)
                                : *reinterpret_cast<const float4*>(tail_in + ((size_t)d * H + (H + t)) * n_beams + 4 * b4);
        *reinterpret_cast<float4*>(tail_out + ((size_t)d * H + j) * n_beams + 4 * b4) = x;
    }
}

template <int K>
hipError_t launch_tile(const float* d_chunk, int n_dm, int n_t, int n_beams, uint64_t seen, const SpsBuffers& buf, hipStream_t stream)
{
    constexpr int ROWS = kT + (1 << (K - 1)) - 1;
    const dim3 grid((unsigned)((n_beams + 4 * kBeamLanes - 1) / (4 * kBeamLanes)), (unsigned)sps_tiles(n_t), (unsigned)n_dm);
    record_launchf("sps_tile_kernel<%d>", K);
    hipLaunchKernelGGL(sps_tile_kernel<K>, grid, dim3(kThreads), ROWS * kBeamLanes * sizeof(float4), stream, d_chunk, buf.tail_in, n_dm, n_t,
                       n_beams, (unsigned long long)seen, buf.part_peaks, buf.part_stats);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sps_push(const float* d_chunk, int n_dm, int n_t, int n_beams, int n_widths, uint64_t seen, const SpsBuffers& buf,
                           hipStream_t stream)
{
    if (n_dm <= 0 || n_dm > 65535 || n_t <= 0 || n_beams <= 0 || n_beams % 4 || n_widths < 1 || n_widths > kSpsMaxWidths)
        return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    switch (n_widths) {
    case 1: e = launch_tile<1>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    case 2: e = launch_tile<2>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    case 3: e = launch_tile<3>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    case 4: e = launch_tile<4>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    case 5: e = launch_tile<5>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    case 6: e = launch_tile<6>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    case 7: e = launch_tile<7>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    default: e = launch_tile<8>(d_chunk, n_dm, n_t, n_beams, seen, buf, stream); break;
    }
    if (e != hipSuccess) return e;
    const int H = sps_halo(n_widths);
    const size_t items = (size_t)(n_widths + 1) * n_dm * n_beams + (size_t)n_dm * H * (n_beams / 4);
    record_launch("sps_finish_kernel");
    hipLaunchKernelGGL(sps_finish_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, d_chunk, buf.tail_in, buf.tail_out,
                       buf.part_peaks, buf.part_stats, buf.peaks, buf.stats, sps_tiles(n_t), n_dm, n_t, n_beams, n_widths, H);
    return hipGetLastError();
}

}  // namespace dsabf
