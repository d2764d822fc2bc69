// bf_cond_kernels.h -- launcher of the conditioning stage's device code (cond/bf_cond.hip; contract: docs/CONDITIONING.md).
// Lives in a directory of its own, like sps/, ib/, corr/ and cal/: the kernel build id (build.kernel_build_id) identifies the
// kernels that bench.py and the counter summaries under profiles/ time, and this stage is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kCondSegment = 32;     // rows per segment of the push totals
constexpr int kCondMaxWindow = 64;   // baseline_pushes <= 64

struct CondStat {
    double sum, sumsq;
};
struct CondParams {
    float inv;      // (float)(1.0 / n_good)
    int n_good;     // unmasked channels
};

// What one push works with (all device memory, owned by the stage).
struct CondBuffers {
    CondStat* seg;               // [ceil(max_rows / 32)][f][b]: the segments' totals of the push that is running
    CondStat* ring;              // [window][f][b]: the totals of the last `window` pushes, push j in set j % window
    double* cell_mu;             // [f][b]: the window's mu ...
    double* cell_var;            // ... and max(var, 0), for the channel summary
    float2* mr32;                // [f][b]: {mu32, r32}, r32 = (float)(1 / sigma), +0.0f = dead cell
    double* cm;                  // [f]: the channel's mean of mu ...
    double* cv;                  // ... and of max(var, 0), in the OSUM order
    double* q;                   // [f]: cv / cm^2 of the channels still unmasked, NaN elsewhere (bands too wide for the summary's LDS)
    double* dev;                 // [f]: |q - med|, NaN elsewhere (the same)
    const uint8_t* static_mask;  // [f]
    uint8_t* mask;               // [f]: the mask of this push
    CondParams* params;
};

// One push, three kernels on `stream`: totals (per cell: the push totals into set cur_set, the window's sums -- the n_sets most
// recent sets, oldest first, n_window rows in all -- mu32 and r32; per channel: cm, cv), summary (the mask, the medians, inv) and
// apply (in place).  k_auto = auto_threshold * 1.4826, <= 0: no automatic mask.
hipError_t launch_cond_push(float* d_rows, int n_rows, int n_freq, int n_beams, const CondBuffers& buf, int window, int cur_set, int n_sets,
                            uint64_t n_window, bool zero_dm, double k_auto, hipStream_t stream);

}  // namespace dsabf
