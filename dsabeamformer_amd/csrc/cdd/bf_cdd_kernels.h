// bf_cdd_kernels.h -- launcher of the coherent dedispersion stage (cdd/bf_cdd.hip; contract: docs/COHERENT_DEDISPERSION.md).
// Lives in a directory of its own, like stokes/ and vcut/: the kernel build id (build.kernel_build_id) identifies the kernels that
// bench.py and the counter summaries under profiles/ time, and these are not among them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dsabf {

constexpr int kCddMinLog = 6, kCddMaxLog = 12;   // FFT lengths 64 ... 4096

// log2 of n_fft if it is one of the seven lengths, else -1
inline int cdd_log2(int n_fft)
{
    for (int m = kCddMinLog; m <= kCddMaxLog; m++)
        if (n_fft == 1 << m) return m;
    return -1;
}
inline bool cdd_supported(int n_chan, int n_fft, int n_edge) { return n_chan >= 1 && cdd_log2(n_fft) >= 0 && n_edge >= 0 && n_edge <= n_fft / 4; }
inline uint32_t cdd_bit_reverse(uint32_t p, int m)
{
    uint32_t r = 0;
    for (int b = 0; b < m; b++) r |= ((p >> b) & 1u) << (m - 1 - b);
    return r;
}

// The twiddle table of length n_fft: n_fft / 2 entries {cos, -sin}(2 pi k / n_fft), computed in double and rounded to float.
void cdd_twiddles_host(int n_fft, float* table);
// One channel row of the chirp as the kernel reads it: row[p] = chirp[bit_reverse(p)] (the forward transform leaves its bins in
// bit-reversed order, so the multiply needs no permutation on the device).
void cdd_permute_row_host(const float* chirp_row, int n_fft, float* row);

struct CddLaunch {
    const void* in;        // x [chan][k][pol][n_time] {re, im} float
    void* out;             // voltages: the same shape; Stokes: [t][chan][k]{I, Q, U, V} float
    const void* twiddles;  // n_fft / 2 float2
    const void* chirp;     // [chan][n_fft] float2, every row bit-reversed
    int n_chan, K, n_time, n_fft, n_edge;
    int n_int;             // 0: the voltage epilogue; >= 1: the Stokes epilogue
};
// hipErrorInvalidValue and nothing launched where a bound of the contract does not hold (the stage reports them with a message first).
hipError_t launch_cdd(const CddLaunch& a, hipStream_t s);
// segments of a series, and whether n_seg * n_chan * K fits one grid axis
inline long long cdd_segments(int n_time, int n_fft, int n_edge)
{
    const long long V = n_fft - 2 * n_edge;
    return (n_time + V - 1) / V;
}

}  // namespace dsabf
