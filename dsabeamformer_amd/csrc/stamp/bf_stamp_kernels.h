// bf_stamp_kernels.h -- launcher of the stamp cut's device code (stamp/bf_stamp.hip; contract: docs/EVENTS.md section 2).
// Lives in a directory of its own, like sps/, ib/, corr/, cal/ and cond/: the kernel build id (build.kernel_build_id) identifies
// the kernels that bench.py and the counter summaries under profiles/ time, and this one is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kStampBatch = 32;   // requests per launch: they travel as kernel arguments (no staging buffer, nothing to keep alive)

struct StampItem {
    uint64_t row;     // physical row of the window's first row (< cap_rows): the rows continue through the ring's second mapping
    int32_t dm;       // local trial: row of `delays`
    int32_t beam;
    int32_t slot;     // index of the request in the caller's array: where its stamp goes in `out`
    int32_t pad;
};
struct StampBatch {
    StampItem item[kStampBatch];
};

// n_items <= kStampBatch stamps, one launch on `stream`:
//   out[slot][g][tau] = sum_f ( sum_i ring[row + tau tbin + i + delays[dm][f]][f][beam] ), f = g fbin + 0 .. fbin - 1, i = 0 .. tbin - 1,
// both sums fp32, sequential, ascending, from their first element.  The caller has checked that every row read lies inside the
// ring's double mapping (row + n_tau tbin + max delay <= 2 cap_rows) and every index inside its array.
hipError_t launch_stamp_cut(const float* ring, size_t row_floats, int n_freq, int n_beams, const int32_t* d_delays, const StampBatch& batch,
                            int n_items, int n_tau, int tbin, int fbin, float* out, hipStream_t stream);

}  // namespace dsabf
