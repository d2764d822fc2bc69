// bf_inj_kernels.h -- launchers of the pulse injector's device code (inj/bf_inj.hip; contract: docs/INJECTION.md section 1).
// Lives in a directory of its own, like sps/, cond/, psr/ and ffa/: the kernel build id (build.kernel_build_id) identifies the
// kernels that bench.py and the counter summaries under profiles/ time, and these are not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../psr/bf_psr_kernels.h"   // psr_bin, kPsrMinBins / kPsrMaxBins: a train's bins are the folder's

namespace dsabf {

constexpr int kInjBatch = 4;         // bursts one launch takes as arguments; more live ones go into further launches, in id order
constexpr int kInjMaxTrains = 4;     // trains alive at a time: they share one read of the rows
constexpr int kInjMaxPulses = 4096, kInjMaxWidth = 4096;
constexpr int kInjRowTile = 8;       // rows one wave takes: that many independent 16-byte loads per lane in front of the adds
constexpr int kInjMaxRows = 1 << 24; // max_rows_per_push: keeps n (n - 1) inside int64 on rows of an apply that a train's gate leaves out

// One pulse's tables on the device, one allocation written once, before the pulse's first launch, and never again while it is alive:
// response float [n_beams] (16-byte aligned), delay int32 [n_freq], profile float [n_freq][W or n_bins].
struct InjBurst {
    const float* profile;
    const float* response;
    const int32_t* delay;
    int64_t rel;                     // t0 - (first row of the apply): the burst's sample i of channel f lies in row rel + delay[f] + i of the apply
    int W;
};
struct InjBurstArgs {
    InjBurst b[kInjBatch];           // ascending id
    int n, n_freq, n_beams;
};
struct InjTrain {
    const float* profile;
    const float* response;
    const int32_t* delay;
    uint64_t phase0, dphase;         // bf_psr_model, as PsrOsc carries it
    int64_t ddphase;
    int64_t n_first;                 // (first row of the apply) - epoch_row
    int lo, hi;                      // the rows [lo, hi) of the apply that lie inside the train's [first_row, first_row + n_rows)
    int n_bins;
};
struct InjTrainArgs {
    InjTrain t[kInjMaxTrains];       // ascending id
    int n, n_freq, n_beams;
    int row_lo, row_hi;              // hull of the trains' [lo, hi): the rows the grid covers
};

// rows: [n_rows][n_freq][n_beams] fp32, 16-byte aligned, n_beams % 4 == 0, rewritten in place.  max_span: the largest count over the
// channels of rows between the first and the last row of the apply that a burst of `a` touches in that channel (host arithmetic on
// the same delays): the grid covers that many rows per channel, and a row inside it that no burst touches is neither read nor written.
// Every touched cell: x = fl(x + fl(profile * response)) once per covering burst, in the order of a.b[].
hipError_t launch_inj_bursts(float* rows, int n_rows, const InjBurstArgs& a, int max_span, hipStream_t stream);
// The same for trains, over rows [a.row_lo, a.row_hi): one read and one write of every row some train covers.
hipError_t launch_inj_trains(float* rows, const InjTrainArgs& a, hipStream_t stream);

}  // namespace dsabf
