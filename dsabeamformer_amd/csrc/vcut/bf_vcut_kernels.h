// bf_vcut_kernels.h -- launcher of the voltage cut's device code (vcut/bf_vcut.hip; contract: docs/VOLTAGE_CUTS.md section 1).
// Lives in a directory of its own, like stamp/, sps/, ib/, corr/, cal/ and cond/: the kernel build id (build.kernel_build_id) identifies
// the kernels that bench.py and the counter summaries under profiles/ time, and this one is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kVcutBatch = 32;          // requests per launch: they travel as kernel arguments (no staging buffer, nothing to keep alive)
constexpr unsigned kVcutMaxRuns = 65535;   // (channel, unit) pairs of one request: the grid's y axis

struct VcutItem {
    uint32_t phys;    // physical unit of the window's first sample: (t0 / S) mod cap_units
    uint32_t rest;    // ... and that sample's place in it: t0 % S
    int32_t dm;       // row of `delays`
    int32_t slot;     // index of the request in the caller's array: where its units go in `out`
};
struct VcutBatch {
    VcutItem item[kVcutBatch];
};

// The ring and the geometry of a unit in it: [cap_units][n_freq][S][B] bytes, B = n_pol n_ant (a multiple of 4).
struct VcutRing {
    const uint8_t* base;
    uint64_t cap_units;
    uint32_t n_freq, S, B;
};

// n_items <= kVcutBatch requests, one launch on `stream`:
//   out[slot][u][f][j][0 .. B) = sample (t0 + u S + j + delays[dm][f]) of channel f,  u < n_units_out, j < S,
// where sample s lies in physical unit (s / S) mod cap_units at sample s % S and t0 = (a multiple of cap_units S) + phys S + rest.
// Bytes are moved, nothing else.  The caller has checked that every sample read lies in a unit the ring holds, every index inside its
// array, n_freq * n_units_out <= kVcutMaxRuns, cap_units < 2^31, S B < 2^31 and that `out` is 4-byte aligned; 16-byte accesses are taken where B % 16 == 0 and `out` is 16-byte aligned (the ring's base always is).
hipError_t launch_vcut(const VcutRing& ring, const int32_t* d_delays, const VcutBatch& batch, int n_items, int n_units_out, uint8_t* out,
                       hipStream_t stream);

}  // namespace dsabf
