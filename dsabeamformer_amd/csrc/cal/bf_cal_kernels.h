// bf_cal_kernels.h -- launchers of the gain solver's device code (cal/bf_cal.hip; contract: docs/CALIBRATION.md).
// Lives in a directory of its own, like sps/, ib/ and corr/: the kernel build id (build.kernel_build_id) identifies the kernels that
// bench.py and the counter summaries under profiles/ time, and these are not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kCalMaxAnt = 256;          // four terms per lane of a wave64: the OSUM of the contract
constexpr int kCalResidentMaxAnt = 64;   // up to here the fp64 square x of a problem lives in LDS (16 n^2 bytes: 64 KiB at 64 antennas)

inline bool cal_supported(int n_ant) { return n_ant > 0 && n_ant % 4 == 0 && n_ant <= kCalMaxAnt; }

// One workgroup per (polarisation layer, channel): StEFCal on the packed lower triangle d_vis [freq][pol][bl]{re, im} (int64).
// d_model [freq][ant]{re, im} or NULL (all ones), d_flags [ant] or NULL, ref_ant -1: the first unflagged antenna.
// d_gains [pol_out][freq][ant]{re, im}, d_info [pol_out][freq]{iterations, status}; pol_out = joint_pol ? 1 : n_pol.
// `streamed` forces the path that re-reads the triangle from global memory every iteration (a test and measurement switch: the
// bits do not depend on it); above kCalResidentMaxAnt it is the only path.
hipError_t launch_solve_gains(int n_ant, int n_freq, int n_pol, const long long* d_vis, const double* d_model, const uint8_t* d_flags,
                              double tol, int max_iter, int ref_ant, bool joint_pol, bool streamed, double* d_gains, int32_t* d_info,
                              hipStream_t s);

// d_w_out[f][a][b] = clip(rint(d_w_in[f][a][b] * c[f][a]), -127, 127) per part; c = conj(g) / |g| (mode 0), times k_f / |g| (mode 1).
hipError_t launch_calibrate_weights(int n_ant, int n_freq, int n_beams, const int8_t* d_w_in, const double* d_gains_layer,
                                    const uint8_t* d_flags, int mode, int8_t* d_w_out, hipStream_t s);

}  // namespace dsabf
