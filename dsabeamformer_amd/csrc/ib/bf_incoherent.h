// bf_incoherent.h -- launcher of the incoherent beam's device code (ib/bf_incoherent.hip; contract: docs/INCOHERENT_BEAM.md).
// Lives in a directory of its own, like sps/: the kernel build id (build.kernel_build_id) identifies the kernels that bench.py and
// the counter summaries under profiles/ time, and this one is not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

// 128 * n_ant * n_ipo <= 2^24: the largest sum a window can reach converts to float exactly (a sample contributes at most 128)
constexpr long long kIbMaxSum = 1ll << 24;
inline bool incoherent_supported(int n_ant, int n_ipo) { return 128ll * n_ant * n_ipo <= kIbMaxSum; }

// Lanes that share one output, chosen by the span's size in load words (16-byte words if every span is 16-byte aligned, 4-byte
// words otherwise): 1, 4, 16 or 64.  Host arithmetic; tools/ib_time.py and the tests name the classes through it.
int incoherent_lanes(size_t span_bytes, bool vec16);

// d_out[(((u * n_out + o) * n_freq + f) * stride)] = (float) sum over the n_ipo * n_ant bytes of window (u, f, o) of re^2 + im^2.
// d_packed [unit][freq][n_out * n_ipo][ant], 4-byte aligned (16-byte aligned pointers and spans take 16-byte loads).
hipError_t launch_incoherent(int n_ant, int n_freq, int n_ipo, int n_out, const void* d_packed, int n_units, float* d_out, size_t stride,
                             int n_cus, hipStream_t s);

}  // namespace dsabf
