// bf_psr_kernels.h -- launcher of the pulsar fold's device code (psr/bf_psr.hip; contract: docs/PULSAR_FOLDING.md section 1).
// Lives in a directory of its own, like sps/, ib/, corr/, cal/, cond/ and stamp/: the kernel build id (build.kernel_build_id)
// identifies the kernels that bench.py and the counter summaries under profiles/ time, and this one is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kPsrMaxPulsars = 4;
constexpr int kPsrMinBins = 2, kPsrMaxBins = 4096;

// One pulsar's oscillator as the kernel takes it (bf_psr_model, with the push's first row already subtracted from the epoch):
// for channel f and row i of the push, n = n_first - delay[f] + i, all inside (-2^31, 2^31) -- the host has checked that.
struct PsrOsc {
    uint64_t phase0, dphase;
    int64_t ddphase;
    int64_t n_first;             // (push's first row) - epoch_row
};
struct PsrFoldArgs {
    PsrOsc osc[kPsrMaxPulsars];
    const int32_t* delays;       // device, [n_psr][n_freq]
    double* profile;             // device, [n_psr][n_freq][n_bins][n_beams]
    unsigned long long* hits;    // device, [n_psr][n_freq][n_bins]
    int n_psr, n_freq, n_bins, n_beams;
};

// The bin of a phase: ((phase >> 32) * n_bins) >> 32 -- the one statement of the rule on the device and in the launcher's callers.
__host__ __device__ inline int psr_bin(uint64_t phase, int n_bins) { return (int)(((phase >> 32) * (uint64_t)n_bins) >> 32); }

// Folds n_rows rows at `rows` ([row][freq][beam] fp32, row stride n_freq * n_beams floats) into a.profile / a.hits, one launch on
// `stream`.  Every cell's adds happen in ascending row order, in one thread, from the value the cell holds when the launch starts:
// launches that share accumulators must be ordered by the caller.
hipError_t launch_psr_fold(const float* rows, int n_rows, const PsrFoldArgs& a, hipStream_t stream);

}  // namespace dsabf
