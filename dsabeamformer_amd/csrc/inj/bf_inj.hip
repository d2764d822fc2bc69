// bf_inj.hip -- device code of the pulse injector (contract: docs/INJECTION.md section 1; runtime: csrc/bf_inj.cpp).
//
// Both kernels add fl(profile * response[beam]) to cells of the detected rows [row][freq][beam] where they lie.  A workgroup is one
// wave; blockIdx.y is the channel, blockIdx.x a tile of kInjRowTile rows, blockIdx.z a group of 256 beams.  A lane owns four
// consecutive beams as one 16-byte access, so a wave's access to a row of 256 beams is 1 KiB contiguous, and the pulses' responses
// for its four beams stay in registers for the whole workgroup.  Everything else -- which rows of the tile a pulse covers, the
// index into its profile, a train's 64-bit phase, step and step of the step -- depends on blockIdx, the kernel arguments and the
// loop counter only: the same in every lane, no per-lane bin.  All table reads come before the first store of the workgroup.
// The multiply and the add are two roundings (__fmul_rn, __fadd_rn), in the order of the argument arrays: ascending id.
// No atomics, no LDS, nothing carried from one launch to the next.
#include "bf_inj_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

__device__ inline float4 inj_add(float4 x, float v, float4 resp)
{
    x.x = __fadd_rn(x.x, __fmul_rn(v, resp.x));
    x.y = __fadd_rn(x.y, __fmul_rn(v, resp.y));
    x.z = __fadd_rn(x.z, __fmul_rn(v, resp.z));
    x.w = __fadd_rn(x.w, __fmul_rn(v, resp.w));
    return x;
}

template <int NB>
__global__ __launch_bounds__(64) void inj_burst_kernel(float* __restrict__ rows, int n_rows, InjBurstArgs a)
{
    const int f = (int)blockIdx.y;
    const int quad = (int)(blockIdx.z * 64 + threadIdx.x);
    // start[k]: the row of the apply that holds sample 0 of burst k in this channel; [lo, hi): from the first to the last row of the
    // apply that any burst of the launch touches here
    int64_t start[NB];
    int64_t lo = INT64_MAX, hi = INT64_MIN;
#pragma unroll
    for (int k = 0; k < NB; k++) {
        start[k] = a.b[k].rel + (int64_t)a.b[k].delay[f];
        lo = start[k] < lo ? start[k] : lo;
        hi = start[k] + a.b[k].W > hi ? start[k] + a.b[k].W : hi;
    }
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_rows ? n_rows : hi;
    const int64_t r0 = lo + (int64_t)blockIdx.x * kInjRowTile;
    if (r0 >= hi) return;
    if (4 * quad >= a.n_beams) return;   // (n_beams % 4 == 0: a lane has its four beams or none)
    float4 resp[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) resp[k] = reinterpret_cast<const float4*>(a.b[k].response)[quad];
    const size_t row_quads = (size_t)a.n_freq * (size_t)a.n_beams / 4;
    float4* col = reinterpret_cast<float4*>(rows) + (size_t)f * (size_t)(a.n_beams / 4) + (size_t)quad;

    float v[kInjRowTile][NB];
    unsigned covers[kInjRowTile];        // bit k: burst k covers row r0 + j of this channel
    float4 x[kInjRowTile];
#pragma unroll
    for (int j = 0; j < kInjRowTile; j++) {
        const int64_t r = r0 + j;
        covers[j] = 0;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const int64_t i = r - start[k];
            const bool in = r < hi && i >= 0 && i < (int64_t)a.b[k].W;
            v[j][k] = in ? a.b[k].profile[(size_t)f * (size_t)a.b[k].W + (size_t)i] : 0.0f;
            covers[j] |= in ? 1u << k : 0u;
        }
        if (covers[j]) x[j] = col[(size_t)r * row_quads];
    }
#pragma unroll
    for (int j = 0; j < kInjRowTile; j++) {
        if (!covers[j]) continue;        // a row no burst touches here: neither read nor written
#pragma unroll
        for (int k = 0; k < NB; k++)
            if (covers[j] >> k & 1u) x[j] = inj_add(x[j], v[j][k], resp[k]);
        col[(size_t)(r0 + j) * row_quads] = x[j];
    }
}

template <int NT>
__global__ __launch_bounds__(64) void inj_train_kernel(float* __restrict__ rows, InjTrainArgs a)
{
    const int f = (int)blockIdx.y;
    const int quad = (int)(blockIdx.z * 64 + threadIdx.x);
    const int r0 = a.row_lo + (int)blockIdx.x * kInjRowTile;
    if (4 * quad >= a.n_beams) return;
    // the oscillators at row r0, as psr_fold_kernel starts them
    uint64_t ph[NT], st[NT], dd[NT];
    float4 resp[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) {
        const InjTrain& t = a.t[k];
        const int64_t n = t.n_first + (int64_t)r0 - (int64_t)t.delay[f];   // |n| < 2^31 + kInjMaxRows: n (n - 1) / 2 is exact in int64
        dd[k] = (uint64_t)t.ddphase;
        ph[k] = t.phase0 + (uint64_t)n * t.dphase + (uint64_t)(n * (n - 1) / 2) * dd[k];
        st[k] = t.dphase + (uint64_t)n * dd[k];
        resp[k] = reinterpret_cast<const float4*>(t.response)[quad];
    }
    const size_t row_quads = (size_t)a.n_freq * (size_t)a.n_beams / 4;
    float4* col = reinterpret_cast<float4*>(rows) + (size_t)f * (size_t)(a.n_beams / 4) + (size_t)quad;

    float v[kInjRowTile][NT];
    unsigned covers[kInjRowTile];
    float4 x[kInjRowTile];
#pragma unroll
    for (int j = 0; j < kInjRowTile; j++) {
        const int r = r0 + j;
        covers[j] = 0;
#pragma unroll
        for (int k = 0; k < NT; k++) {
            const bool in = r < a.row_hi && r >= a.t[k].lo && r < a.t[k].hi;
            const int bin = psr_bin(ph[k], a.t[k].n_bins);
            v[j][k] = in ? a.t[k].profile[(size_t)f * (size_t)a.t[k].n_bins + (size_t)bin] : 0.0f;
            covers[j] |= in ? 1u << k : 0u;
            ph[k] += st[k];
            st[k] += dd[k];
        }
        if (covers[j]) x[j] = col[(size_t)r * row_quads];
    }
#pragma unroll
    for (int j = 0; j < kInjRowTile; j++) {
        if (!covers[j]) continue;
#pragma unroll
        for (int k = 0; k < NT; k++)
            if (covers[j] >> k & 1u) x[j] = inj_add(x[j], v[j][k], resp[k]);
        col[(size_t)(r0 + j) * row_quads] = x[j];
    }
}

static dim3 inj_grid(int rows, int n_freq, int n_beams)
{
    return dim3((unsigned)((rows + kInjRowTile - 1) / kInjRowTile), (unsigned)n_freq, (unsigned)((n_beams + 255) / 256));
}

hipError_t launch_inj_bursts(float* rows, int n_rows, const InjBurstArgs& a, int max_span, hipStream_t stream)
{
    if (n_rows <= 0 || max_span <= 0) return hipSuccess;
    if (max_span > n_rows || a.n_freq < 1 || a.n_freq > 65535 || a.n_beams < 4 || a.n_beams % 4) return hipErrorInvalidValue;
    const dim3 grid = inj_grid(max_span, a.n_freq, a.n_beams);
    (void)hipGetLastError();   // clear what earlier, unrelated calls left behind: return this launch's own status
    switch (a.n) {
        case 1: record_launch("inj_burst_kernel<1>"); inj_burst_kernel<1><<<grid, 64, 0, stream>>>(rows, n_rows, a); break;
        case 2: record_launch("inj_burst_kernel<2>"); inj_burst_kernel<2><<<grid, 64, 0, stream>>>(rows, n_rows, a); break;
        case 3: record_launch("inj_burst_kernel<3>"); inj_burst_kernel<3><<<grid, 64, 0, stream>>>(rows, n_rows, a); break;
        case 4: record_launch("inj_burst_kernel<4>"); inj_burst_kernel<4><<<grid, 64, 0, stream>>>(rows, n_rows, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_inj_trains(float* rows, const InjTrainArgs& a, hipStream_t stream)
{
    if (a.row_hi <= a.row_lo) return hipSuccess;
    if (a.row_lo < 0 || a.n_freq < 1 || a.n_freq > 65535 || a.n_beams < 4 || a.n_beams % 4) return hipErrorInvalidValue;
    const dim3 grid = inj_grid(a.row_hi - a.row_lo, a.n_freq, a.n_beams);
    (void)hipGetLastError();
    switch (a.n) {
        case 1: record_launch("inj_train_kernel<1>"); inj_train_kernel<1><<<grid, 64, 0, stream>>>(rows, a); break;
        case 2: record_launch("inj_train_kernel<2>"); inj_train_kernel<2><<<grid, 64, 0, stream>>>(rows, a); break;
        case 3: record_launch("inj_train_kernel<3>"); inj_train_kernel<3><<<grid, 64, 0, stream>>>(rows, a); break;
        case 4: record_launch("inj_train_kernel<4>"); inj_train_kernel<4><<<grid, 64, 0, stream>>>(rows, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dsabf
