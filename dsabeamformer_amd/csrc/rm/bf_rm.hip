// bf_rm.hip -- device code of the Faraday synthesis stage (include/dsabf.h: bf_rm_*; contract: docs/FARADAY.md).
//
// F[m][p] = sum_c (q + i u)[m][c] (r + i s)[p][c] over the (row, beam) pairs m = t K + k is a complex GEMM in float32, and each part
// of it is defined as ONE fmaf chain over ascending channels, two fused operations per channel.  v_mfma_f32_32x32x2_f32 performs
// exactly that pair for a 32 x 32 tile: with A = (q_c, u_c) on the two k-lanes and B = (r, -s) it adds q r, then u (-s), to the
// accumulator, each with one rounding; with B = (s, r) it is the imaginary part.  One channel of the chain = two instructions.
//
// A workgroup of four waves takes 32 pairs.  The cells of 64 channels at a time go through LDS -- read from memory once, the baseline
// subtracted there, Q and U laid out as the A operand (lds[c][k * 32 + i]: one conflict-free ds_read_b32 per channel and wave).  Every
// wave holds four tiles of 32 depths (2 x 4 x 16 accumulator registers) and reads its B operands straight from the table, which the
// host has laid out per (channel, pass, wave, lane) so that they are two 16-byte loads; the next channel's are in flight while this
// channel's eight instructions run.  512 depths are one pass; a longer grid takes further passes over the same pairs.
// The peaks are reduced where the accumulators are: the first maximum of a lane's tiles, of the 32 lanes of a row (shuffles), of the
// four waves (LDS), of the passes (a running record in LDS); then the lanes that hold depth p - 1, p, p + 1 of a row write their part
// of its record.  Nothing but the 32-byte record goes to memory when no spectrum is asked for.
#include "bf_rm_kernels.h"
#include "../rec/bf_launch_record.h"

#include <climits>

namespace dsabf {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kChunk = 64;                      // channels staged at a time
constexpr int kThreads = 64 * kRmWaves;

struct RmArgs {
    const float* __restrict__ s;
    const float* __restrict__ base;
    const float4* __restrict__ table;
    const float* __restrict__ wn;
    float2* __restrict__ spec;
    float* __restrict__ peaks;
    int n_chan, n_phi, K, M, n_pass;
    int in16, base16, peaks16;
};

__device__ __forceinline__ float4 load_cell(const float* p, int wide)
{
    if (wide) return *reinterpret_cast<const float4*>(p);
    const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
    return make_float4(a.x, a.y, b.x, b.y);
}

// (pow, p) of another lane or wave beats ours: a larger power, or the same power at a smaller depth
__device__ __forceinline__ bool beats(float op, int oi, float bp, int bi) { return op > bp || (op == bp && oi < bi); }

template <bool SPEC, bool PEAKS>
__global__ __launch_bounds__(kThreads, 2) void rm_kernel(RmArgs a)
{
    __shared__ float qu_lds[kChunk][64];                 // [c][k * 32 + i]: q (k = 0), u (k = 1) of pair i
    __shared__ float i_lds[PEAKS ? kChunk : 1][32];
    __shared__ float wave_pow[kRmWaves][32];
    __shared__ int wave_p[kRmWaves][32];
    __shared__ float best_pow[32], rec_lo[32], rec_hi[32], rec_re[32], rec_im[32], last_pow[32];
    __shared__ int best_p[32];

    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 31, hk = lane >> 5;
    const long long m0 = (long long)blockIdx.x * kRmRows;   // (64 bits: the last tile of 2^31 - 1 pairs ends beyond an int)
    // staging: this thread always loads pair si, channels sc, sc + 8, ... of the chunk
    const int si = tid & 31, sc = tid >> 5;
    const long long sm = m0 + si;
    const bool s_in = sm < a.M;
    const int st = s_in ? (int)(sm / a.K) : 0, sk = s_in ? (int)(sm - (long long)st * a.K) : 0;
    const float* cell0 = a.s + ((size_t)st * a.n_chan * a.K + sk) * 4;     // + c K 4
    const float* base0 = a.base ? a.base + (size_t)sk * 4 : nullptr;
    float isum = 0.f;

    for (int pass = 0; pass < a.n_pass; pass++) {
        bool valid[kRmTiles];
#pragma unroll
        for (int tt = 0; tt < kRmTiles; tt++) valid[tt] = ((pass * 16 + tt * 4 + w) * 32) < a.n_phi;
        f32x16 re[kRmTiles], im[kRmTiles];
#pragma unroll
        for (int tt = 0; tt < kRmTiles; tt++)
#pragma unroll
            for (int r = 0; r < 16; r++) re[tt][r] = 0.f, im[tt][r] = 0.f;

        const size_t chan_stride = (size_t)a.n_pass * kRmWaves * 64 * 2;   // float4 per channel of the table
        const float4* tb = a.table + (((size_t)pass * kRmWaves + w) * 64 + lane) * 2;

        for (int c0 = 0; c0 < a.n_chan; c0 += kChunk) {
            const int nc = a.n_chan - c0 < kChunk ? a.n_chan - c0 : kChunk;
            __syncthreads();   // the chunk before this one has been read
            for (int cl = sc; cl < nc; cl += kThreads / 32) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s_in) {
                    const size_t off = (size_t)(c0 + cl) * a.K * 4;
                    v = load_cell(cell0 + off, a.in16);
                    if (base0) {
                        const float4 b = load_cell(base0 + off, a.base16);
                        v.x = __fsub_rn(v.x, b.x), v.y = __fsub_rn(v.y, b.y), v.z = __fsub_rn(v.z, b.z);
                    }
                }
                qu_lds[cl][si] = v.y;
                qu_lds[cl][32 + si] = v.z;
                if (PEAKS) i_lds[cl][si] = v.x;
            }
            __syncthreads();

            if (PEAKS && pass == 0 && tid < 32)
                for (int cl = 0; cl < nc; cl++) isum = __fmaf_rn(i_lds[cl][tid], a.wn[c0 + cl], isum);

            const float4* tc = tb + (size_t)c0 * chan_stride;
            float4 b0 = tc[0], b1 = tc[1];
            for (int cl = 0; cl < nc; cl++) {
                const float av = qu_lds[cl][lane];
                const int nx = cl + 1 < nc ? cl + 1 : cl;
                const float4 n0 = tc[(size_t)nx * chan_stride], n1 = tc[(size_t)nx * chan_stride + 1];
                if (valid[0]) {
                    re[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0.x, re[0], 0, 0, 0);
                    im[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0.y, im[0], 0, 0, 0);
                }
                if (valid[1]) {
                    re[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0.z, re[1], 0, 0, 0);
                    im[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0.w, im[1], 0, 0, 0);
                }
                if (valid[2]) {
                    re[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1.x, re[2], 0, 0, 0);
                    im[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1.y, im[2], 0, 0, 0);
                }
                if (valid[3]) {
                    re[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1.z, re[3], 0, 0, 0);
                    im[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1.w, im[3], 0, 0, 0);
                }
                b0 = n0, b1 = n1;
            }
        }

        // accumulator register r of lane (j, hk) is pair (r & 3) + 8 (r >> 2) + 4 hk, depth tile * 32 + j
        if (SPEC) {
#pragma unroll
            for (int tt = 0; tt < kRmTiles; tt++) {
                const int p = (pass * 16 + tt * 4 + w) * 32 + j;
                if (p >= a.n_phi) continue;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const long long m = m0 + (r & 3) + 8 * (r >> 2) + 4 * hk;
                    if (m < a.M) a.spec[(size_t)m * a.n_phi + p] = make_float2(re[tt][r], im[tt][r]);
                }
            }
        }
        if (PEAKS) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float bp = -1.f;
                int bi = INT_MAX;
#pragma unroll
                for (int tt = 0; tt < kRmTiles; tt++) {
                    const int p = (pass * 16 + tt * 4 + w) * 32 + j;
                    if (p >= a.n_phi) continue;
                    const float pw = __fadd_rn(__fmul_rn(re[tt][r], re[tt][r]), __fmul_rn(im[tt][r], im[tt][r]));
                    if (pw > bp) bp = pw, bi = p;   // ascending depths: the first maximum stays
                }
#pragma unroll
                for (int off = 1; off < 32; off <<= 1) {
                    const float op = __shfl_xor(bp, off);
                    const int oi = __shfl_xor(bi, off);
                    if (beats(op, oi, bp, bi)) bp = op, bi = oi;
                }
                if (j == 0) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * hk;
                    wave_pow[w][row] = bp;
                    wave_p[w][row] = bi;
                }
            }
            __syncthreads();
            if (tid < 32) {
                float bp = wave_pow[0][tid];
                int bi = wave_p[0][tid];
                for (int ww = 1; ww < kRmWaves; ww++)
                    if (beats(wave_pow[ww][tid], wave_p[ww][tid], bp, bi)) bp = wave_pow[ww][tid], bi = wave_p[ww][tid];
                if (pass == 0 || bp > best_pow[tid]) {   // a later pass must be larger: the first maximum stays
                    best_pow[tid] = bp;
                    best_p[tid] = bi;
                    rec_lo[tid] = pass > 0 && bi == pass * kRmPass ? last_pow[tid] : 0.f;   // (its left neighbour was in the pass before)
                    rec_hi[tid] = 0.f;
                    rec_re[tid] = 0.f;
                    rec_im[tid] = 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hk;
                const int bpr = best_p[row];
#pragma unroll
                for (int tt = 0; tt < kRmTiles; tt++) {
                    const int p = (pass * 16 + tt * 4 + w) * 32 + j;
                    if (p >= a.n_phi) continue;
                    const bool last = p == pass * kRmPass + kRmPass - 1;
                    if (p != bpr && p + 1 != bpr && p - 1 != bpr && !last) continue;
                    const float pw = __fadd_rn(__fmul_rn(re[tt][r], re[tt][r]), __fmul_rn(im[tt][r], im[tt][r]));
                    if (p == bpr) rec_re[row] = re[tt][r], rec_im[row] = im[tt][r];
                    if (p + 1 == bpr) rec_lo[row] = pw;
                    if (p - 1 == bpr) rec_hi[row] = pw;
                    if (last) last_pow[row] = pw;
                }
            }
            // (the next pass's first barrier stands between these writes and its reads)
        }
    }

    if (PEAKS) {
        __syncthreads();
        if (tid < 32 && m0 + tid < a.M) {
            float* o = a.peaks + (size_t)(m0 + tid) * 8;
            const int p = best_p[tid] == INT_MAX ? 0 : best_p[tid];   // (no finite power in the row: outside the contract)
            const float4 x = make_float4(__int_as_float(p), rec_lo[tid], best_pow[tid], rec_hi[tid]);
            const float4 y = make_float4(rec_re[tid], rec_im[tid], isum, __int_as_float(0));
            if (a.peaks16) {
                *reinterpret_cast<float4*>(o) = x;
                *reinterpret_cast<float4*>(o + 4) = y;
            } else {
                *reinterpret_cast<float2*>(o) = make_float2(x.x, x.y);
                *reinterpret_cast<float2*>(o + 2) = make_float2(x.z, x.w);
                *reinterpret_cast<float2*>(o + 4) = make_float2(y.x, y.y);
                *reinterpret_cast<float2*>(o + 6) = make_float2(y.z, y.w);
            }
        }
    }
}

}  // namespace

void rm_permute_table_host(const float* rot, int n_chan, int n_phi, float* out)
{
    const int n_pass = rm_passes(n_phi);
    for (int c = 0; c < n_chan; c++)
        for (int pass = 0; pass < n_pass; pass++)
            for (int w = 0; w < kRmWaves; w++)
                for (int lane = 0; lane < 64; lane++) {
                    float* o = out + ((((size_t)c * n_pass + pass) * kRmWaves + w) * 64 + lane) * kRmTiles * 2;
                    for (int tt = 0; tt < kRmTiles; tt++) {
                        const int p = (pass * 16 + tt * 4 + w) * 32 + (lane & 31);
                        float r = 0.f, s = 0.f;
                        if (p < n_phi) r = rot[((size_t)p * n_chan + c) * 2], s = rot[((size_t)p * n_chan + c) * 2 + 1];
                        o[tt * 2] = lane >> 5 ? -s : r;
                        o[tt * 2 + 1] = lane >> 5 ? r : s;
                    }
                }
}

hipError_t launch_rm(const RmLaunch& l, hipStream_t s)
{
    if (!l.stokes || !l.table || !l.wn || (!l.spec && !l.peaks) || !rm_supported(l.n_chan, l.n_phi) || l.K < 1 || l.n_rows < 1 ||
        (long long)l.n_rows * l.K > 0x7fffffffLL)
        return hipErrorInvalidValue;
    if (((uintptr_t)l.stokes & 7) || ((uintptr_t)l.base & 7) || ((uintptr_t)l.spec & 7) || ((uintptr_t)l.peaks & 7) || ((uintptr_t)l.table & 15))
        return hipErrorInvalidValue;
    RmArgs a;
    a.s = (const float*)l.stokes;
    a.base = (const float*)l.base;
    a.table = (const float4*)l.table;
    a.wn = (const float*)l.wn;
    a.spec = (float2*)l.spec;
    a.peaks = (float*)l.peaks;
    a.n_chan = l.n_chan;
    a.n_phi = l.n_phi;
    a.K = l.K;
    a.M = l.n_rows * l.K;
    a.n_pass = rm_passes(l.n_phi);
    a.in16 = ((uintptr_t)l.stokes & 15) == 0;
    a.base16 = ((uintptr_t)l.base & 15) == 0;
    a.peaks16 = ((uintptr_t)l.peaks & 15) == 0;
    const unsigned grid = (unsigned)(((long long)a.M + kRmRows - 1) / kRmRows);   // (64 bits: M + 31 can pass 2^31)
    (void)hipGetLastError();
    if (l.spec && l.peaks) {
        record_launch("rm_kernel<true, true>");
        hipLaunchKernelGGL((rm_kernel<true, true>), dim3(grid), dim3(kThreads), 0, s, a);
    } else if (l.peaks) {
        record_launch("rm_kernel<false, true>");
        hipLaunchKernelGGL((rm_kernel<false, true>), dim3(grid), dim3(kThreads), 0, s, a);
    } else {
        record_launch("rm_kernel<true, false>");
        hipLaunchKernelGGL((rm_kernel<true, false>), dim3(grid), dim3(kThreads), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dsabf
