// bf_corr_kernels.h -- launcher of the correlator's device code (corr/bf_corr.hip; contract: docs/CORRELATOR.md).
// Lives in a directory of its own, like sps/ and ib/: the kernel build id (build.kernel_build_id) identifies the kernels that
// bench.py and the counter summaries under profiles/ time, and this one is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kCorrMaxAnt = 256;                 // the output grows as n_ant^2
// Columns per polarisation in one call: a column contributes at most 128 to either part, the sums of a launch live in the MFMA's
// int32 accumulators, so 128 * N <= 2^31 - 1, i.e. N < 2^24.
constexpr long long kCorrMaxColumns = (1ll << 24) - 1;
static_assert(128ll * kCorrMaxColumns <= 2147483647ll, "the largest sum of a launch must fit the int32 accumulators");

__host__ __device__ inline size_t corr_baselines(int n_ant) { return (size_t)n_ant * (size_t)(n_ant + 1) / 2; }
inline bool corr_supported(int n_ant, long long columns_per_pol)
{
    return n_ant > 0 && n_ant % 4 == 0 && n_ant <= kCorrMaxAnt && columns_per_pol > 0 && columns_per_pol <= kCorrMaxColumns;
}

// d_vis[((f * n_pol + p) * n_ant (n_ant + 1) / 2 + a1 (a1 + 1) / 2 + a2) * 2 + {0, 1}] (int64) = (accumulate ? what is there : 0) +
// re, im of the sum over the n_units * n_cols columns c = p (mod n_pol) of v[u][f][c][a1] * conj(v[u][f][c][a2]), a2 <= a1.
// d_packed [unit][freq][n_cols * n_pol][ant], 4-byte aligned; d_vis 8-byte aligned.  One launch, no atomics.
hipError_t launch_correlate(int n_ant, int n_freq, int n_pol, int n_cols, const void* d_packed, int n_units, long long* d_vis,
                            bool accumulate, hipStream_t s);

}  // namespace dsabf
