// bf_null_kernels.h -- launchers of the spatial null's device code (null/bf_null.hip; contract: docs/NULLING.md).
// Lives in a directory of its own, like sps/, ib/, corr/, cal/, cond/, sk/ and stokes/: the kernel build id (build.kernel_build_id)
// identifies the kernels that bench.py and the counter summaries under profiles/ time, and these are not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kNullMaxAnt = 256;          // four terms per lane of a wave64: the OSUM of docs/CALIBRATION.md section 2
constexpr int kNullResidentMaxAnt = 64;   // up to here the fp64 square x of a channel lives in LDS (16 n^2 bytes: 64 KiB at 64 antennas)
constexpr int kNullMaxVecs = 4;           // BF_NULL_MAX

inline bool null_supported(int n_ant) { return n_ant > 0 && n_ant % 4 == 0 && n_ant <= kNullMaxAnt; }

// One workgroup per channel: deflated power iteration on the packed lower triangle d_vis [freq][pol][bl]{re, im} (int64), diagonal kept.
// pol -1: the polarisations' integers are added first; 0 ... n_pol - 1: that polarisation.  d_flags [ant] or NULL.
// d_vecs [freq][n_null][ant]{re, im} (unused vectors exact zeros), d_eig [freq][n_null + 1] (the lambdas, then the trace),
// d_info [freq][1 + 2 n_null] (n_used, then {iterations, status} per vector).
// `streamed` forces the path that re-reads the triangle from global memory every iteration (a test and measurement switch: the
// bits do not depend on it); above kNullResidentMaxAnt it is the only path.
hipError_t launch_null_solve(int n_ant, int n_freq, int n_pol, const long long* d_vis, const uint8_t* d_flags, int n_null, double min_ratio,
                             double tol, int max_iter, int pol, bool streamed, double* d_vecs, double* d_eig, int32_t* d_info, hipStream_t s);

// d_w_out[f][a][b] = clip(rint(k_f (w - sum_j conj(u_j[a]) (u_j^T w)[b])), -127, 127) per part for the channels with n_used > 0
// (mode 0: k_f = min(1, 127 / max |part|); mode 1: k_f = 1); the other channels are copied; flagged antennas are zeroed in both.
// d_scale [freq] or NULL receives k_f.
hipError_t launch_null_weights(int n_ant, int n_freq, int n_beams, const int8_t* d_w_in, const double* d_vecs, const int32_t* d_info, int n_null,
                               const uint8_t* d_flags, int mode, int8_t* d_w_out, double* d_scale, hipStream_t s);

}  // namespace dsabf
