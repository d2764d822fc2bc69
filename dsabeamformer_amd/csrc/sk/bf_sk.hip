// bf_sk.hip -- device code of the voltage moments (include/dsabf.h: bf_sk_device, bf_sk_*; contract: docs/SPECTRAL_KURTOSIS.md).
//
// Per channel f, polarisation p and antenna a:  M1 = sum of P, M2 = sum of P * P over the columns c = p (mod n_pol) of every unit,
// P = re^2 + im^2 of the packed byte (0 ... 128).  Exact integers, so the order of the sums is free.
//
// The input [unit][freq][time][ant] is read once.  A column is n_ant contiguous bytes; a lane loads one word of it (16 bytes where
// n_ant is a multiple of 16 and the array is 16-byte aligned, 4 bytes otherwise) and so owns 16 or 4 consecutive antennas.  A
// workgroup is TX lanes across a column (or across a chunk of it, `achunks` chunks of at most 1024 / n_pol antennas) by `rows`
// columns; rows is a multiple of n_pol, so a lane that steps on by `rows` columns stays in one polarisation and keeps one
// accumulator pair per byte in registers.  Per byte, in integers: the word masked to that byte, dotted with the whole word as eight
// signed nibbles (v_dot8_i32_i4) is P = re * re + im * im of that byte alone; m1 += P; m2 += P * P as a dot of unsigned bytes
// (v_dot4_u32_u8, P <= 128 is one byte).  Four or five VALU operations per sample and no multiply; nothing is summed across bytes.
//
// Work: the row-blocks (rows columns of one unit, channel and antenna chunk) in the order (f, chunk, unit, row-block), cut into
// one contiguous range per workgroup -- whatever the geometry, the launch fills the chip and a workgroup crosses from one (f, chunk)
// to the next at most a few times.  At such a crossing, at the end of its range and after kMaxIters row-blocks (the int32 m2 of a
// lane holds 2^17 columns; it is widened at 2^16) the lanes add their registers to an int64 image of the (f, chunk) in LDS with LDS
// atomics, and the image's non-zero entries go to the output with 64-bit global atomics.  accumulate == false is a memset of the
// output in front of the kernel, on the same queue.
#include "bf_sk_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

namespace {

constexpr int kThreads = 256;
constexpr int kImage = 1024;          // antennas x polarisations of the LDS image (two int64 each: 16 KiB)
constexpr int kMaxIters = 1 << 16;    // row-blocks a lane accumulates in int32: m2 <= 2^16 * 2^14
typedef unsigned long long u64;

struct SkArgs {
    const uint8_t* __restrict__ in;   // [unit][f][T][ant]
    u64* __restrict__ out;            // [f][p][ant]{m1, m2}
    int n_ant, n_freq, n_pol, n_units;
    int T;                            // columns of one unit and channel (n_cols * n_pol)
    int wpc;                          // words per column
    int TX, rows, achunks, RB;        // lanes across a chunk, columns per row-block, chunks per column, row-blocks per unit
    long long items, per;             // row-blocks of the launch, and of one workgroup
};

template <int B> struct Acc {
    int m1[B], m2[B];
};

__device__ __forceinline__ void sk_word(unsigned w, int* m1, int* m2)
{
#pragma unroll
    for (int b = 0; b < 4; b++) {
        // the word masked to byte b, dotted with the word as eight signed nibbles: re * re + im * im of that byte alone
        const int p = __builtin_amdgcn_sdot8((int)(w & (0xFFu << (8 * b))), (int)w, 0, false);
        m1[b] += p;
        m2[b] = (int)__builtin_amdgcn_udot4((unsigned)p, (unsigned)p, (unsigned)m2[b], false);   // p <= 128: one byte
    }
}
__device__ __forceinline__ void sk_add(unsigned w, Acc<4>& a) { sk_word(w, a.m1, a.m2); }
__device__ __forceinline__ void sk_add(const uint4& w, Acc<16>& a)
{
    sk_word(w.x, a.m1, a.m2);
    sk_word(w.y, a.m1 + 4, a.m2 + 4);
    sk_word(w.z, a.m1 + 8, a.m2 + 8);
    sk_word(w.w, a.m1 + 12, a.m2 + 12);
}
__device__ __forceinline__ unsigned sk_zero(unsigned) { return 0u; }
__device__ __forceinline__ uint4 sk_zero(uint4) { return make_uint4(0u, 0u, 0u, 0u); }

template <class W>
__global__ __launch_bounds__(kThreads, 4) void moments_kernel(SkArgs a)
{
    constexpr int B = (int)sizeof(W);
    __shared__ u64 image[2 * kImage];   // [pol][TX * B antennas]{m1, m2}
    const int chunk_ants = a.TX * B, n_image = 2 * a.n_pol * chunk_ants;
    for (int i = threadIdx.x; i < n_image; i += kThreads) image[i] = 0;
    __syncthreads();

    const int tx = (int)threadIdx.x % a.TX, row = (int)threadIdx.x / a.TX;
    const int pol = row % a.n_pol;
    const long long per_key = (long long)a.n_units * a.RB;
    long long i = (long long)blockIdx.x * a.per;
    const long long end = i + a.per < a.items ? i + a.per : a.items;
    while (i < end) {   // (every condition of this loop is the same for all lanes of the workgroup)
        const long long key = i / per_key, r = i - key * per_key;
        const int f = (int)(key / a.achunks), ac = (int)(key - (long long)f * a.achunks);
        int u = (int)(r / a.RB), rb = (int)(r - (long long)u * a.RB);
        long long run = end - i < per_key - r ? end - i : per_key - r;
        if (run > kMaxIters) run = kMaxIters;

        const int word = ac * a.TX + tx;
        const bool live = row < a.rows && word < a.wpc;
        const uint8_t* base = a.in + (size_t)word * B + (size_t)row * (size_t)a.n_ant;
        long long left = run;   // row-blocks of the run not yet loaded
        auto next = [&]() -> W {   // the lane's word of the next row-block; zero bytes (which add nothing) past the run or the unit
            W w = sk_zero(W());
            if (left <= 0) return w;
            left--;
            if (live && rb * a.rows + row < a.T)
                w = *reinterpret_cast<const W*>(base + (((size_t)u * a.n_freq + f) * a.T + (size_t)rb * a.rows) * (size_t)a.n_ant);
            if (++rb == a.RB) {
                rb = 0;
                u++;
            }
            return w;
        };
        Acc<B> acc;
#pragma unroll
        for (int b = 0; b < B; b++) acc.m1[b] = acc.m2[b] = 0;
        // a batch of loads per lane (32 bytes at least), issued one batch ahead of the arithmetic on the batch before
        constexpr int N = B == 16 ? 2 : 8;
        W cur[N], nxt[N];
#pragma unroll
        for (int j = 0; j < N; j++) cur[j] = next();
        for (long long k = 0; k < run; k += N) {
#pragma unroll
            for (int j = 0; j < N; j++) nxt[j] = next();
#pragma unroll
            for (int j = 0; j < N; j++) sk_add(cur[j], acc);
#pragma unroll
            for (int j = 0; j < N; j++) cur[j] = nxt[j];
        }

        if (live) {
            u64* dst = image + 2 * ((size_t)pol * chunk_ants + (size_t)tx * B);
#pragma unroll
            for (int b = 0; b < B; b++)
                if (acc.m1[b]) {
                    atomicAdd(dst + 2 * b, (u64)acc.m1[b]);
                    atomicAdd(dst + 2 * b + 1, (u64)acc.m2[b]);
                }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < n_image; e += kThreads) {
            const u64 v = image[e];
            if (!v) continue;
            image[e] = 0;
            const int cell = e >> 1, p = cell / chunk_ants, ant = ac * chunk_ants + (cell - p * chunk_ants);
            if (ant < a.n_ant) atomicAdd(a.out + (((size_t)f * a.n_pol + p) * a.n_ant + ant) * 2 + (e & 1), v);
        }
        __syncthreads();
        i += run;
    }
}

template <class W>
hipError_t launch(SkArgs a, int n_cus, hipStream_t s)
{
    constexpr int B = (int)sizeof(W);
    a.wpc = a.n_ant / B;
    const int limit = kImage / (B * a.n_pol) < kThreads / a.n_pol ? kImage / (B * a.n_pol) : kThreads / a.n_pol;   // >= 1: n_pol <= kSkMaxPol
    a.achunks = (a.wpc + limit - 1) / limit;
    a.TX = (a.wpc + a.achunks - 1) / a.achunks;
    a.rows = kThreads / a.TX / a.n_pol * a.n_pol;   // >= n_pol: TX <= kThreads / n_pol
    a.RB = (a.T + a.rows - 1) / a.rows;
    a.items = (long long)a.n_freq * a.achunks * a.n_units * a.RB;
    // four row-blocks per workgroup at least; at most the 4 workgroups per CU that are resident at 4 waves per SIMD
    const long long want = (a.items + 3) / 4, cap = (long long)(n_cus > 0 ? n_cus : 256) * 4;
    const long long groups = want < cap ? want : cap;
    a.per = (a.items + groups - 1) / groups;
    record_launchf("moments_kernel<%s>", sizeof(W) == 16 ? "HIP_vector_type<unsigned int, 4u> " : "unsigned int");
    hipLaunchKernelGGL((moments_kernel<W>), dim3((unsigned)((a.items + a.per - 1) / a.per)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_moments(int n_ant, int n_freq, int n_pol, int n_cols, const void* d_packed, int n_units, long long* d_moments, bool accumulate,
                          int n_cus, hipStream_t s)
{
    if (n_freq <= 0 || n_cols <= 0 || n_units <= 0 || !d_packed || !d_moments || !sk_supported(n_ant, n_pol, (long long)n_units * n_cols) ||
        ((uintptr_t)d_packed & 3) || ((uintptr_t)d_moments & 7))
        return hipErrorInvalidValue;
    SkArgs a;
    a.in = (const uint8_t*)d_packed;
    a.out = (u64*)d_moments;
    a.n_ant = n_ant;
    a.n_freq = n_freq;
    a.n_pol = n_pol;
    a.n_units = n_units;
    a.T = n_cols * n_pol;
    (void)hipGetLastError();
    if (!accumulate) {
        const hipError_t e = hipMemsetAsync(d_moments, 0, (size_t)n_freq * n_pol * n_ant * 2 * sizeof(long long), s);
        if (e != hipSuccess) return e;
    }
    return n_ant % 16 == 0 && ((uintptr_t)d_packed & 15) == 0 ? launch<uint4>(a, n_cus, s) : launch<unsigned>(a, n_cus, s);
}

}  // namespace dsabf
