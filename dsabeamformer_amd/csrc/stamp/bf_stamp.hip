// bf_stamp.hip -- the stamp cut: dedispersed dynamic spectra of single beams, read out of the DM stage's ring (docs/EVENTS.md
// section 2; include/dsabf.h: bf_dm_stream_cut).
//
// One beam out of a beam-contiguous row [f][b]: neighbouring elements of a stamp lie a whole channel (n_beams floats) or a
// whole row apart, so every element is a memory transaction of its own.  That is inherent in the layout; the kernel is bound
// by transactions in flight, not by bytes or arithmetic.  Each lane owns one output time tau and walks f, then i, in the
// contract's order; the loads of kStampUnroll consecutive (f, i) terms are issued before the first add of the batch, so a lane
// has that many independent loads outstanding.  f, i and the delays are the same in every lane of a wave: the loop control and
// the delay loads are scalar.  The window starts at a physical row < cap_rows and runs on through the ring's second mapping: no
// wrap test in the loop.  Row offsets are 64-bit.
#include "bf_stamp_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

constexpr int kStampUnroll = 8;
constexpr int kStampLanes = 64;    // output times per workgroup: one wave each ...
constexpr int kStampGroups = 4;    // ... for this many frequency groups

__global__ __launch_bounds__(kStampLanes * kStampGroups) void stamp_cut_kernel(const float* __restrict__ ring, size_t row_floats, int n_freq,
                                                                                int n_beams, const int32_t* __restrict__ delays,
                                                                                const StampBatch batch, int n_tau, int tbin, int fbin,
                                                                                float* __restrict__ out)
{
    const StampItem it = batch.item[blockIdx.z];
    const int n_g = n_freq / fbin;
    const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * kStampGroups + threadIdx.y));   // (a wave has one threadIdx.y)
    const size_t tau = (size_t)blockIdx.x * kStampLanes + threadIdx.x;
    if (g >= n_g || tau >= (size_t)n_tau) return;
    const int f0 = g * fbin, f_end = f0 + fbin;
    const int32_t* __restrict__ dl = delays + (size_t)it.dm * n_freq;
    const float* __restrict__ base = ring + ((size_t)it.row + tau * (size_t)tbin) * row_floats + it.beam;
    float acc = 0.0f, s = 0.0f;
    int lf = f0, li = 0;   // the term the next load takes
    int af = f0, ai = 0;   // the term the next add takes
    while (af < f_end) {
        float v[kStampUnroll];
#pragma unroll
        for (int u = 0; u < kStampUnroll; u++) {
            if (lf < f_end) {
                v[u] = base[(size_t)(dl[lf] + li) * row_floats + (size_t)lf * n_beams];
                if (++li == tbin) {
                    li = 0;
                    lf++;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kStampUnroll; u++) {
            if (af < f_end) {
                s = ai == 0 ? v[u] : s + v[u];               // the sum over i starts from its first element ...
                if (++ai == tbin) {
                    acc = af == f0 ? s : acc + s;             // ... and so does the sum over f
                    ai = 0;
                    af++;
                }
            }
        }
    }
    out[((size_t)it.slot * n_g + g) * (size_t)n_tau + tau] = acc;
}

hipError_t launch_stamp_cut(const float* ring, size_t row_floats, int n_freq, int n_beams, const int32_t* d_delays, const StampBatch& batch,
                            int n_items, int n_tau, int tbin, int fbin, float* out, hipStream_t stream)
{
    if (n_items <= 0) return hipSuccess;
    const int n_g = n_freq / fbin;
    const dim3 block(kStampLanes, kStampGroups);
    const dim3 grid((unsigned)(((size_t)n_tau + kStampLanes - 1) / kStampLanes), (unsigned)((n_g + kStampGroups - 1) / kStampGroups), (unsigned)n_items);
    record_launch("stamp_cut_kernel");
    hipLaunchKernelGGL(stamp_cut_kernel, grid, block, 0, stream, ring, row_floats, n_freq, n_beams, d_delays, batch, n_tau, tbin, fbin, out);
    return hipGetLastError();
}

}  // namespace dsabf
