// bf_stokes_kernels.h -- launchers of the full-Stokes follow-up beams (stokes/bf_stokes.hip; contract: docs/STOKES.md).
// Lives in a directory of its own, like sps/, ib/, corr/ and sk/: the kernel build id (build.kernel_build_id) identifies the kernels
// that bench.py and the counter summaries under profiles/ time, and these are not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kStokesMaxBeams = 16;    // one 16-wide MFMA tile of beams (BF_STOKES_MAX_BEAMS)
constexpr int kStokesMaxAnt = 256;     // |Xr|, |Xi| <= 2048 * n_ant <= 2^19: the MFMA's int32 accumulator, and 2^40 per int64 term
constexpr int kStokesKStep = 64;       // antennas of one v_mfma_i32_16x16x64_i8
constexpr int kStokesWindows = 8;      // integration windows of one span (the work item of a wave)

inline int stokes_ksteps(int n_ant) { return (n_ant + kStokesKStep - 1) / kStokesKStep; }
// The compact weights of one stage: [freq][k-step][plane: re, im][lane 0 .. 63][16 bytes], the bytes of lane l being the weights of
// beam column (l & 15) for the antennas 64 * kstep + 16 * (l >> 4) + 0 ... 15 -- the B operand of the MFMA as the lane loads it.
// Beam columns >= n_sel and antennas >= n_ant hold zero.
inline size_t stokes_weight_bytes(int n_ant, int n_freq) { return (size_t)n_freq * (size_t)stokes_ksteps(n_ant) * 2 * 64 * 16; }

inline bool stokes_supported(int n_ant, int n_pol, int n_cols, int n_sel, int n_int)
{
    return n_pol == 2 && n_ant > 0 && n_ant % 4 == 0 && n_ant <= kStokesMaxAnt && n_sel >= 1 && n_sel <= kStokesMaxBeams && n_cols > 0 && n_cols <= (1 << 20) &&
           n_int >= 1 && n_cols % n_int == 0;
}

// The same image built on the host (bf_stokes_set_weights): w [freq][ant][beam]{re, im} int8, beams[n_sel] already checked.
void stokes_gather_host(const int8_t* w, const int* beams, int n_sel, int n_ant, int n_freq, int n_beams, int8_t* image);

// d_image (stokes_weight_bytes) from d_w [freq][ant][beam]{re, im} int8 (device) and beams[n_sel] (HOST: read during the call and
// passed to the kernel by value), asynchronously on s.
hipError_t launch_stokes_gather(const int8_t* d_w, const int* beams, int n_sel, int n_ant, int n_freq, int n_beams, int8_t* d_image,
                                hipStream_t s);

// d_out [unit][t][freq][k]{I, Q, U, V} (int64, every cell written once, no atomics to global memory) from d_packed
// [unit][freq][2 * n_cols][ant] (n_cols = S samples per unit, 4-byte aligned) and the compact weights; t = S / n_int windows per unit.
hipError_t launch_stokes(int n_ant, int n_freq, int n_cols, int n_sel, int n_int, const void* d_packed, int n_units, const int8_t* d_image,
                         long long* d_out, int n_cus, hipStream_t s);

// The beam samples themselves, the work split of n_int = 1: d_out [freq][k][pol][n_units * n_cols]{re, im} float (8-byte aligned; the
// exact integers of the accumulators, |.| <= 2^19), n_units * n_cols < 2^31.  16-byte stores where a lane's pair of samples starts on
// a 16-byte address, 8-byte ones otherwise.
hipError_t launch_stokes_voltages(int n_ant, int n_freq, int n_cols, int n_sel, const void* d_packed, int n_units, const int8_t* d_image,
                                  float* d_out, int n_cus, hipStream_t s);

}  // namespace dsabf
