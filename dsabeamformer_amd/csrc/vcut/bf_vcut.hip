// bf_vcut.hip -- the voltage cut: dedispersed gemm-units in the input layout, read out of the voltage history's ring
// (docs/VOLTAGE_CUTS.md; include/dsabf.h: bf_vhist_cut).
//
// One output RUN is channel f of output unit u of request r: S samples of B bytes, contiguous on both sides.  Its first sample is
// s0 = t0 + u S + delays[dm][f] of the series; it comes from at most two source runs, the tail of channel f of unit s0 / S from
// sample j0 = s0 % S and the first j0 samples of channel f of the unit behind it -- either of which may be the ring's last physical
// unit followed by its first.  r, u and f are the workgroup's grid coordinates, so s0, the two physical units, j0 and the delay are
// the same in every lane: the divisions (32-bit: the host splits t0 into whole units and a rest) and the delay load run on the scalar
// unit, once per workgroup.  A run is split over grid.x in fixed pieces of kUnroll chunks of kThreads words; a word comes from the
// first source run or the second: one compare and one select per lane, on a 32-bit offset.  A lane issues the kUnroll loads of its piece
// unconditionally (a lane beyond the run's end loads the run's last word, and stores nothing) before the first store.  The word is 16
// bytes where every boundary is 16-byte aligned on both sides (B % 16 == 0, `out` aligned), 4 bytes otherwise.  Unit and output
// offsets are 64-bit; offsets inside a run are 32-bit (S B < 2^31).
// Plain C++, vector loads and stores, no LDS, no atomics; every output byte is written exactly once and nothing else is written.
#include "bf_vcut_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 8;
typedef unsigned v4u __attribute__((ext_vector_type(4)));   // one 16-byte load / store

template <typename W>
__global__ __launch_bounds__(kThreads) void vcut_kernel(const VcutRing ring, const int32_t* __restrict__ delays, const VcutBatch batch,
                                                        int n_units_out, uint8_t* __restrict__ out)
{
    constexpr uint32_t kChunk = kThreads * sizeof(W);   // bytes one load instruction of the workgroup covers
    // uniform: everything down to the two source offsets.  The host has split t0 into whole units and a rest (VcutItem), so the
    // divisions here are 32-bit: rest + delay < 2^32, every physical unit < cap_units < 2^31.
    const VcutItem it = batch.item[blockIdx.z];
    const uint32_t f = blockIdx.y % ring.n_freq, u = blockIdx.y / ring.n_freq;
    const uint32_t run_bytes = ring.S * ring.B;
    const uint64_t unit_bytes = (uint64_t)run_bytes * ring.n_freq;
    const uint32_t e = it.rest + (uint32_t)delays[(size_t)it.dm * ring.n_freq + f];
    const uint32_t k = e / ring.S, j0 = e % ring.S;
    const uint32_t cap = (uint32_t)ring.cap_units;
    uint32_t phys0 = (it.phys + u) % cap + k % cap;
    phys0 = phys0 >= cap ? phys0 - cap : phys0;
    const uint32_t phys1 = phys0 + 1 == cap ? 0 : phys0 + 1;
    const uint32_t head = (ring.S - j0) * ring.B;   // bytes of the run that come from the first unit (all of them where j0 == 0)
    // byte x of the run lies at ring.base + (x < head ? off0 : off1) + x  (off1: unsigned arithmetic, used from x = head on only)
    const uint64_t off0 = phys0 * unit_bytes + (uint64_t)f * run_bytes + (uint64_t)j0 * ring.B;
    const uint64_t off1 = phys1 * unit_bytes + (uint64_t)f * run_bytes - head;
    const uint8_t* __restrict__ src0 = ring.base + off0;
    const uint8_t* __restrict__ src1 = ring.base + off1;
    uint8_t* __restrict__ dst = out + (((uint64_t)it.slot * (uint32_t)n_units_out + u) * ring.n_freq + f) * run_bytes;

    const uint32_t x0 = (blockIdx.x * (kUnroll * kThreads) + threadIdx.x) * (uint32_t)sizeof(W);   // (run_bytes < 2^31: no overflow)
    const uint32_t last = run_bytes - (uint32_t)sizeof(W);   // the run's last word: what a lane beyond the run loads, and does not store
    W v[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {
        const uint32_t x = x0 + i * kChunk, xl = x < last ? x : last;
        v[i] = *reinterpret_cast<const W*>((xl < head ? src0 : src1) + xl);
    }
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {
        const uint32_t x = x0 + i * kChunk;
        if (x < run_bytes) *reinterpret_cast<W*>(dst + x) = v[i];
    }
}

}  // namespace

hipError_t launch_vcut(const VcutRing& ring, const int32_t* d_delays, const VcutBatch& batch, int n_items, int n_units_out, uint8_t* out,
                       hipStream_t stream)
{
    if (n_items <= 0) return hipSuccess;
    const bool vec = ring.B % 16 == 0 && ((uintptr_t)out & 15) == 0;
    const uint32_t run_bytes = ring.S * ring.B, piece = (uint32_t)kThreads * kUnroll * (vec ? 16 : 4);
    const dim3 grid((unsigned)((run_bytes + piece - 1) / piece), (unsigned)(ring.n_freq * (uint32_t)n_units_out), (unsigned)n_items);
    if (vec) {
        record_launch("vcut_kernel<unsigned int __vector(4)>");
        hipLaunchKernelGGL(vcut_kernel<v4u>, grid, dim3(kThreads), 0, stream, ring, d_delays, batch, n_units_out, out);
    } else {
        record_launch("vcut_kernel<unsigned int>");
        hipLaunchKernelGGL(vcut_kernel<uint32_t>, grid, dim3(kThreads), 0, stream, ring, d_delays, batch, n_units_out, out);
    }
    return hipGetLastError();
}

}  // namespace dsabf
