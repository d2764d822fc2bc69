// bf_incoherent.hip -- device code of the incoherent beam (include/dsabf.h: bf_incoherent_device, bf_set_incoherent_beam;
// contract: docs/INCOHERENT_BEAM.md).
//
// Per output (unit u, output time o, channel f): S = sum over the n_ipo * n_ant packed bytes of its window of re^2 + im^2, an exact
// integer, written as (float)S.  In the packed layout [unit][freq][n_out * n_ipo][ant] the window of (u, f, o) is ONE contiguous span
// of n_ipo * n_ant bytes, and the spans follow each other without gaps in (u, f, o) order: the input is a flat array of spans, read
// once, in address order.
//
// incoherent_kernel<L, W>: L lanes share a span (1, 4, 16 or 64, by the span's size), every lane loads words of W (16-byte words
// where every span is 16-byte aligned, 4-byte words otherwise); the lanes of a group take consecutive words, so a group reads
// L * sizeof(W) contiguous bytes per load and neighbouring groups of a wave neighbouring spans.  Four bytes at a time:
//   x = w & 0xF0F0F0F0 = 16 re as four int8,  y = (w << 4) & 0xF0F0F0F0 = 16 im,  acc = dot4(x, x, acc), acc = dot4(y, y, acc)
// accumulates 256 (re^2 + im^2).  A lane's share of a span stays below 2^23 in units of S (incoherent_lanes sees to it), so the
// x256 fits int32; it is shifted out BEFORE the lanes of the group are summed (the group's total may reach 2^24).  Integer sums:
// the result does not depend on L, W or the launch.  No LDS, no atomics: lane 0 of a group stores its output.
#include "bf_incoherent.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ int ib_word(unsigned w, int acc)
{
    const int x = (int)(w & 0xF0F0F0F0u), y = (int)((w << 4) & 0xF0F0F0F0u);
    acc = __builtin_amdgcn_sdot4(x, x, acc, false);
    return __builtin_amdgcn_sdot4(y, y, acc, false);
}
__device__ __forceinline__ int ib_add(unsigned w, int acc) { return ib_word(w, acc); }
__device__ __forceinline__ int ib_add(uint4 w, int acc) { return ib_word(w.w, ib_word(w.z, ib_word(w.y, ib_word(w.x, acc)))); }

template <int L, class W>
__global__ __launch_bounds__(kThreads) void incoherent_kernel(const uint8_t* __restrict__ packed, float* __restrict__ out, long long n_spans,
                                                              int words, int n_out, int n_freq, size_t stride)
{
    const int j = threadIdx.x % L;   // this lane's place in its group
    const long long groups = (long long)gridDim.x * (kThreads / L);
    for (long long s = (long long)blockIdx.x * (kThreads / L) + threadIdx.x / L; s < n_spans; s += groups) {
        const W* p = reinterpret_cast<const W*>(packed) + (size_t)s * (size_t)words;
        int acc = 0, i = j;
        for (; i + 3 * L < words; i += 4 * L) {   // four loads in flight per lane
            const W a = p[i], b = p[i + L], c = p[i + 2 * L], d = p[i + 3 * L];
            acc = ib_add(d, ib_add(c, ib_add(b, ib_add(a, acc))));
        }
        for (; i < words; i += L) acc = ib_add(p[i], acc);
        unsigned v = (unsigned)acc >> 8;
#pragma unroll
        for (int off = 1; off < L; off <<= 1) v += __shfl_xor(v, off);
        if (j == 0) {   // span s = (u * n_freq + f) * n_out + o  ->  out[((u * n_out + o) * n_freq + f) * stride]
            const long long t = s / n_out, o = s - t * n_out, u = t / n_freq, f = t - u * n_freq;
            out[(size_t)((u * n_out + o) * n_freq + f) * stride] = (float)v;
        }
    }
}

template <int L, class W>
hipError_t launch(const void* d_packed, float* d_out, long long n_spans, size_t span_bytes, int n_out, int n_freq, size_t stride, int n_cus,
                  hipStream_t s)
{
    // a group per span up to 8 workgroups per CU; beyond that the groups stride on to further spans
    const long long per_block = kThreads / L, want = (n_spans + per_block - 1) / per_block, cap = (long long)(n_cus > 0 ? n_cus : 256) * 8;
    record_launchf("incoherent_kernel<%d, %s>", L, sizeof(W) == 16 ? "HIP_vector_type<unsigned int, 4u> " : "unsigned int");
    hipLaunchKernelGGL((incoherent_kernel<L, W>), dim3((unsigned)(want < cap ? want : cap)), dim3(kThreads), 0, s, (const uint8_t*)d_packed, d_out,
                       n_spans, (int)(span_bytes / sizeof(W)), n_out, n_freq, stride);
    return hipGetLastError();
}

template <class W>
hipError_t launch_words(int lanes, const void* d_packed, float* d_out, long long n_spans, size_t span_bytes, int n_out, int n_freq, size_t stride,
                        int n_cus, hipStream_t s)
{
    switch (lanes) {
    case 1: return launch<1, W>(d_packed, d_out, n_spans, span_bytes, n_out, n_freq, stride, n_cus, s);
    case 4: return launch<4, W>(d_packed, d_out, n_spans, span_bytes, n_out, n_freq, stride, n_cus, s);
    case 16: return launch<16, W>(d_packed, d_out, n_spans, span_bytes, n_out, n_freq, stride, n_cus, s);
    default: return launch<64, W>(d_packed, d_out, n_spans, span_bytes, n_out, n_freq, stride, n_cus, s);
    }
}

}  // namespace

// At least two words per lane where the span has them (one lane per span below 8 words: neighbouring lanes then read neighbouring
// spans), at most 8 before the next class.  A lane's share in units of S is at most 128 * span_bytes / L: with span_bytes <= 2^17
// (incoherent_supported) one lane could reach 2^24, four lanes stay at 2^22 -- and a span that large has 64.
int incoherent_lanes(size_t span_bytes, bool vec16)
{
    const size_t words = span_bytes / (vec16 ? 16 : 4);
    return words >= 512 ? 64 : words >= 32 ? 16 : words >= 8 ? 4 : 1;
}

hipError_t launch_incoherent(int n_ant, int n_freq, int n_ipo, int n_out, const void* d_packed, int n_units, float* d_out, size_t stride, int n_cus,
                             hipStream_t s)
{
    if (n_ant <= 0 || n_ant % 4 || n_freq <= 0 || n_ipo <= 0 || n_out <= 0 || n_units <= 0 || !stride || !incoherent_supported(n_ant, n_ipo) ||
        ((uintptr_t)d_packed & 3) || ((uintptr_t)d_out & 3))
        return hipErrorInvalidValue;
    const size_t span_bytes = (size_t)n_ipo * (size_t)n_ant;
    const long long n_spans = (long long)n_units * n_freq * n_out;
    const bool vec16 = span_bytes % 16 == 0 && ((uintptr_t)d_packed & 15) == 0;
    const int lanes = incoherent_lanes(span_bytes, vec16);
    return vec16 ? launch_words<uint4>(lanes, d_packed, d_out, n_spans, span_bytes, n_out, n_freq, stride, n_cus, s)
                 : launch_words<unsigned>(lanes, d_packed, d_out, n_spans, span_bytes, n_out, n_freq, stride, n_cus, s);
}

}  // namespace dsabf
