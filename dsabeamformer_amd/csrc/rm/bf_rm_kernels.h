// bf_rm_kernels.h -- launcher of the Faraday synthesis stage (rm/bf_rm.hip; contract: docs/FARADAY.md).
// Lives in a directory of its own, like cdd/ and stokes/: the kernel build id (build.kernel_build_id) identifies the kernels that
// bench.py and the counter summaries under profiles/ time, and this one is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kRmMaxChan = 4096, kRmMaxPhi = 4096;
// The launch shape: a workgroup of kRmWaves waves takes kRmRows (row, beam) pairs; in one pass every wave holds kRmTiles tiles of
// 32 depths in its accumulators, so a pass covers kRmPass depths and depth tile T = pass * 16 + tt * 4 + wave.
constexpr int kRmRows = 32, kRmWaves = 4, kRmTiles = 4, kRmPass = 32 * kRmWaves * kRmTiles;

inline bool rm_supported(int n_chan, int n_phi) { return n_chan >= 1 && n_chan <= kRmMaxChan && n_phi >= 1 && n_phi <= kRmMaxPhi; }
inline int rm_passes(int n_phi) { return (n_phi + kRmPass - 1) / kRmPass; }
// floats of the table as the kernel reads it: per channel and pass, per wave and lane, the lane's eight operands
inline size_t rm_table_floats(int n_chan, int n_phi) { return (size_t)n_chan * rm_passes(n_phi) * kRmWaves * 64 * kRmTiles * 2; }

// rot[p][c]{r, s} -> the B operands of v_mfma_f32_32x32x2_f32, in the order the waves load them:
//   out[c][pass][wave][lane][tt]{re, im},  depth p = (pass * 16 + tt * 4 + wave) * 32 + (lane & 31),  k = lane >> 5:
//   re = k ? -s : r   (F_re takes q r, then u (-s)),   im = k ? r : s   (F_im takes q s, then u r);  0 where p >= n_phi.
void rm_permute_table_host(const float* rot, int n_chan, int n_phi, float* out);

struct RmLaunch {
    const void* stokes;   // s [t][chan][k]{I, Q, U, V} float
    const void* base;     // [chan][k]{I, Q, U, V} float, or NULL
    const void* table;    // rm_permute_table_host's
    const void* wn;       // [chan] float
    void* spec;           // [t][k][p]{re, im} float, or NULL
    void* peaks;          // [t][k] 32-byte records, or NULL
    int n_chan, n_phi, K, n_rows;
};
// hipErrorInvalidValue and nothing launched where a bound of the contract does not hold (the stage reports them with a message first).
hipError_t launch_rm(const RmLaunch& a, hipStream_t s);

}  // namespace dsabf
