// bf_sps_kernels.h -- launcher of the single-pulse search stage's device code (sps/bf_sps.hip; contract: docs/SINGLE_PULSE.md).
// Lives in a directory of its own: the kernel build id (build.kernel_build_id) identifies the kernels that bench.py and the
// counter summaries under profiles/ time, and the search stage is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dsabf.h"

namespace dsabf {

constexpr int kSpsMaxWidths = 8;    // boxcar widths 1, 2, ..., 2^(K-1), K <= 8
constexpr int kSpsTileTimes = 128;  // output times per workgroup (plus a halo of 2^(K-1) - 1 rows in front of them)

inline int sps_halo(int n_widths) { return (1 << (n_widths - 1)) - 1; }
inline int sps_tiles(int n_t) { return (n_t + kSpsTileTimes - 1) / kSpsTileTimes; }

// What one push works with (all device memory, owned by the stage).
struct SpsBuffers {
    const float* tail_in;     // [n_dm][halo][n_beams]: the halo samples in front of this push (zeros where the stream had none)
    float* tail_out;          // the same for the next push (a different buffer: tiles of this push still read tail_in)
    bf_sps_peak* part_peaks;  // [tiles][K][n_dm][n_beams]
    bf_sps_stat* part_stats;  // [tiles][n_dm][n_beams]
    bf_sps_peak* peaks;       // [K][n_dm][n_beams]
    bf_sps_stat* stats;       // [n_dm][n_beams]
};

// One push: the tile kernel (reads every chunk element once, leaves per-tile peaks and statistics) and the finishing pass
// (combines the tiles in ascending order, writes the tail of the next push).  d_chunk [n_dm][n_t][n_beams]; `seen`: samples of
// the series in front of this push (S_k exists for seen + t >= 2^k - 1).
hipError_t launch_sps_push(const float* d_chunk, int n_dm, int n_t, int n_beams, int n_widths, uint64_t seen, const SpsBuffers& buf,
                           hipStream_t stream);

}  // namespace dsabf
