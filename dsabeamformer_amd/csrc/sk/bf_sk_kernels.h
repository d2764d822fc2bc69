// bf_sk_kernels.h -- launcher of the voltage-moment kernel (sk/bf_sk.hip; contract: docs/SPECTRAL_KURTOSIS.md).
// Lives in a directory of its own, like sps/, ib/ and corr/: the kernel build id (build.kernel_build_id) identifies the kernels that
// bench.py and the counter summaries under profiles/ time, and this one is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kSkMaxAnt = 2048;                  // the output is linear in n_ant: the beamformer's own limit
constexpr int kSkMaxPol = 64;                    // a workgroup holds one row of lanes per polarisation at least (bf_sk.hip)
// Columns per polarisation in one call: the correlator's bound, for which M1 <= 128 * N fits int32.
constexpr long long kSkMaxColumns = (1ll << 24) - 1;
static_assert(128ll * kSkMaxColumns <= 2147483647ll, "M1 of a call fits int32");

inline bool sk_supported(int n_ant, int n_pol, long long columns_per_pol)
{
    return n_ant > 0 && n_ant % 4 == 0 && n_ant <= kSkMaxAnt && n_pol > 0 && n_pol <= kSkMaxPol && columns_per_pol > 0 &&
           columns_per_pol <= kSkMaxColumns;
}

// d_moments[((f * n_pol + p) * n_ant + a) * 2 + {0, 1}] (int64) = (accumulate ? what is there : 0) + the sums over the
// n_units * n_cols columns c = p (mod n_pol) of antenna a in channel f of {P, P * P}, P = re^2 + im^2 of the packed byte.
// d_packed [unit][freq][n_cols * n_pol][ant], 4-byte aligned; d_moments 8-byte aligned.  accumulate == false: a memset of the
// output, then the kernel, on the same queue; the workgroups add their partial sums with 64-bit integer atomics.
hipError_t launch_moments(int n_ant, int n_freq, int n_pol, int n_cols, const void* d_packed, int n_units, long long* d_moments,
                          bool accumulate, int n_cus, hipStream_t s);

}  // namespace dsabf
