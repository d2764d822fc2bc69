// bf_ffa_kernels.h -- launchers of the periodicity search's device code (ffa/bf_ffa.hip; contract: docs/PERIODICITY.md section 1).
// Lives in a directory of its own, like sps/ and psr/: the kernel build id (build.kernel_build_id) identifies the kernels that
// bench.py and the counter summaries under profiles/ time, and these are not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dsabf.h"

namespace dsabf {

constexpr int kFfaMaxDec = 256, kFfaMaxSeg = 16384, kFfaMaxOct = 6, kFfaMaxWidths = 6;
constexpr int kFfaMinPeriod = 8, kFfaMaxPeriod = 512;
constexpr int kFfaMaxDetrendBlk = 256, kFfaMaxDetrendWin = 129;

// The rows M of the fold of an octave of `len` samples at base period p: the largest power of two <= len / p (0: none fits).
__host__ __device__ inline int ffa_rows(int len, int p)
{
    const int q = p > 0 ? len / p : 0;
    int m = 0;
    for (int b = 1; b <= q && b > 0; b <<= 1) m = b;
    return m;
}

// Floats of one series slot: the octaves one behind the other, each [n_dm][n_beams][n_seg >> o] -- the samples of one (trial, beam)
// contiguous in time, which is what the fold reads.
inline size_t ffa_octave_offset(int o, int n_seg, size_t n_db)
{
    size_t off = 0;
    for (int i = 0; i < o; i++) off += n_db * (size_t)(n_seg >> i);
    return off;
}

// Decimates chunk times into decimated samples: groups [g0, g0 + n_groups) of this push, group g being chunk times
// [g tdec - c0, (g + 1) tdec - c0), c0 the samples the group in progress already holds (in carry_in, [n_dm][n_beams]).  A group
// the chunk completes goes to y0[(d, beam)][pos0 + g - g0] (octave 0 of a slot); the one it leaves open goes to carry_out.
// chunk: [n_dm][n_t][n_beams] fp32, 16-byte aligned, n_beams % 4 == 0.  carry_in and carry_out must differ.
hipError_t launch_ffa_decimate(const float* d_chunk, int n_dm, int n_t, int n_beams, int tdec, int c0, int g0, int n_groups, const float* carry_in,
                               float* carry_out, float* y0, int n_seg, int pos0, hipStream_t stream);

// The running-median detrend of one full segment, in place (docs/PERIODICITY.md section 1a): y0 is octave 0 of a slot,
// [n_dm][n_beams][n_seg], 16-byte aligned; blk a power of two 1 .. 256 that divides n_seg, win odd 1 .. 129.  Behind the decimation
// launch that closes the segment and in front of launch_ffa_search, on the same queue.
hipError_t launch_ffa_detrend(float* y0, int n_dm, int n_beams, int n_seg, int blk, int win, hipStream_t stream);

// One full segment in `slot` (octave 0 filled): the higher octaves, then per octave every base period p_lo <= p < p_hi folded, its
// K boxcar widths, and the records peaks[o][p - p_lo][k][d][beam]; stats[d][beam] over octave 0.
hipError_t launch_ffa_search(float* slot, int n_dm, int n_beams, int n_seg, int n_oct, int p_lo, int p_hi, int n_widths, bf_ffa_peak* peaks,
                             bf_ffa_stat* stats, hipStream_t stream);

}  // namespace dsabf
