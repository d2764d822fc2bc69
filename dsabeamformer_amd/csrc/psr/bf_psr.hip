// bf_psr.hip -- device code of the pulsar fold (contract: docs/PULSAR_FOLDING.md section 1; runtime: csrc/bf_psr.cpp).
//
// One thread owns one (channel, beam) column of the pushed rows and walks the rows in ascending order; lanes are consecutive
// beams, so a wave's load of one row is 256 contiguous bytes.  The bin of a (row, channel) is the same for every beam: the
// oscillator -- phase, step, step of the step, all 64-bit integers -- depends on blockIdx only and advances by two adds per row.
// The cell the column is in lives in a register while the bin does not change; a bin change stores it with a plain vector store and
// loads the next cell.  A cell therefore receives its adds in row order, in fp64, one rounding per add, from whatever it held when
// the launch began: no atomics, no partial sums.  The pulsars of a stage share one read of the rows.
// The rows come in batches of kBatch independent loads in front of the dependent adds: with one wave per (channel, 64 beams) that
// is the parallelism the memory system sees.
#include "bf_psr_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

constexpr int kBatch = 16;

template <int NPSR>
__global__ __launch_bounds__(256) void psr_fold_kernel(const float* __restrict__ rows, int n_rows, PsrFoldArgs a)
{
    const int f = (int)blockIdx.x;
    const int b = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    if (b >= a.n_beams) return;
    const bool counts = b == 0;   // the one thread of a channel that keeps hits[k][f][*]
    const size_t row_floats = (size_t)a.n_freq * (size_t)a.n_beams;
    const float* src = rows + (size_t)f * (size_t)a.n_beams + (size_t)b;

    uint64_t ph[NPSR], st[NPSR], dd[NPSR];
    double* cells[NPSR];
    unsigned long long* hits[NPSR];
    int cur[NPSR];
    double acc[NPSR];
    unsigned long long cnt[NPSR];
#pragma unroll
    for (int k = 0; k < NPSR; k++) {
        const PsrOsc& o = a.osc[k];
        const int64_t n = o.n_first - (int64_t)a.delays[(size_t)k * a.n_freq + f];   // |n| < 2^31: n (n - 1) / 2 is exact in int64
        dd[k] = (uint64_t)o.ddphase;
        ph[k] = o.phase0 + (uint64_t)n * o.dphase + (uint64_t)(n * (n - 1) / 2) * dd[k];
        st[k] = o.dphase + (uint64_t)n * dd[k];                                       // phase(n + 1) - phase(n)
        const size_t kf = (size_t)k * (size_t)a.n_freq + (size_t)f;
        cells[k] = a.profile + kf * (size_t)a.n_bins * (size_t)a.n_beams + (size_t)b;
        hits[k] = a.hits + kf * (size_t)a.n_bins;
        cur[k] = -1;
        acc[k] = 0.0;
        cnt[k] = 0;
    }

    auto put_back = [&](int k) {
        cells[k][(size_t)cur[k] * (size_t)a.n_beams] = acc[k];
        if (counts) hits[k][cur[k]] += cnt[k];
    };
    auto add_row = [&](float x) {
#pragma unroll
        for (int k = 0; k < NPSR; k++) {
            const int bin = psr_bin(ph[k], a.n_bins);
            if (bin != cur[k]) {
                if (cur[k] >= 0) put_back(k);
                cur[k] = bin;
                acc[k] = cells[k][(size_t)bin * (size_t)a.n_beams];
                cnt[k] = 0;
            }
            acc[k] = acc[k] + (double)x;
            cnt[k]++;
            ph[k] += st[k];
            st[k] += dd[k];
        }
    };

    int r = 0;
    for (; r + kBatch <= n_rows; r += kBatch) {
        float x[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++) x[i] = src[(size_t)(r + i) * row_floats];
#pragma unroll
        for (int i = 0; i < kBatch; i++) add_row(x[i]);
    }
    for (; r < n_rows; r++) add_row(src[(size_t)r * row_floats]);
#pragma unroll
    for (int k = 0; k < NPSR; k++)
        if (cur[k] >= 0) put_back(k);
}

hipError_t launch_psr_fold(const float* rows, int n_rows, const PsrFoldArgs& a, hipStream_t stream)
{
    if (n_rows <= 0) return hipSuccess;
    const int block = a.n_beams >= 256 ? 256 : (a.n_beams + 63) / 64 * 64;
    const dim3 grid((unsigned)a.n_freq, (unsigned)((a.n_beams + block - 1) / block));
    (void)hipGetLastError();   // clear what earlier, unrelated calls left behind: return this launch's own status
    switch (a.n_psr) {
        case 1: record_launch("psr_fold_kernel<1>"); psr_fold_kernel<1><<<grid, block, 0, stream>>>(rows, n_rows, a); break;
        case 2: record_launch("psr_fold_kernel<2>"); psr_fold_kernel<2><<<grid, block, 0, stream>>>(rows, n_rows, a); break;
        case 3: record_launch("psr_fold_kernel<3>"); psr_fold_kernel<3><<<grid, block, 0, stream>>>(rows, n_rows, a); break;
        case 4: record_launch("psr_fold_kernel<4>"); psr_fold_kernel<4><<<grid, block, 0, stream>>>(rows, n_rows, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dsabf
