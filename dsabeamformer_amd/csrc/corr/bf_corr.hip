// bf_corr.hip -- device code of the correlator (include/dsabf.h: bf_correlate_device, bf_corr_*; contract: docs/CORRELATOR.md).
//
// Per channel f and polarisation p:  V[a1][a2] = sum over the columns c = p (mod n_pol) of v[c][a1] * conj(v[c][a2]),  a2 <= a1,
// exact integers: an int8 GEMM with TIME as the K axis, on v_mfma_i32_16x16x64_i8 (operand maps: bf_fused16.hpp).
//
// A workgroup (4 waves) owns one (f, p, 64 x 64 antenna super-tile) over every column of the launch -- no atomics, no reduction
// across workgroups; only super-tiles on or below the diagonal exist (Hermitian symmetry), and on a diagonal super-tile only the
// 16 x 16 tiles on or below it are computed.  Wave w owns row tile w against the (up to) four column tiles: 4 x 3 accumulators.
//
// Per chunk of 128 columns:
//   stage   every thread loads 4 x 4 blocks (4 antennas = one dword, of 4 consecutive columns), sign-extends the nibbles into an
//           re and an im dword each (true int8 values -8 ... 7: a 16 x nibble operand pair would cost 8 bits of the accumulator),
//           transposes the 4 x 4 bytes in registers and writes one dword per antenna into the LDS image [re | im][antenna][column]
//           (rows of 128 + 16 bytes: the dword writes of a wave and the 16-byte fragment reads both spread over all banks);
//   MFMA    K = 64 consecutive columns of one plane: lane l reads bytes 16 (l >> 4) ... of row (l & 15) of a tile, for A (rows a1) and
//           B (columns a2) alike, so any mistake in the K order would be the same permutation on both sides.  Per tile and K step
//             re += A_re . B_re + A_im . B_im        mr += A_im . B_re        rm += A_re . B_im        im = mr - rm
//           (four MFMAs per 64 columns, as the (r | m) form over 32 columns would need, and no negated plane).
// The next chunk's global loads are issued before the MFMAs of the current one.  Columns past the end and antennas past n_ant are
// zero bytes.  Epilogue: int32 -> int64, stored or added (accumulate) with plain vector stores.
#include "bf_corr_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kSuper = 64;                    // antennas per super-tile side
constexpr int kChunk = 128;                   // columns per LDS image
constexpr int kRow = kChunk + 16;             // bytes per antenna row of a plane
constexpr int kPlane = kSuper * kRow;         // one plane (re or im) of one antenna set
constexpr int kSet = 2 * kPlane;              // re | im
static_assert(kRow % 16 == 0 && (kRow / 4) % 8 == 4, "16-byte aligned rows, four rows apart = half the banks");
static_assert(2 * kSet <= 64 * 1024, "two antenna sets of LDS");

struct CorrArgs {
    const uint8_t* __restrict__ in;   // [unit][f][n_cols * n_pol][ant]
    long long* __restrict__ vis;      // [f][p][bl]{re, im}
    int n_ant, n_freq, n_pol, n_cols; // n_cols: columns per polarisation and unit
    int S;                            // columns per polarisation in the launch
    int n_super;                      // super-tiles per side
    int accumulate;
};

// four nibbles 0 ... 15, one per byte -> four int8 -8 ... 7 ((x ^ 8) - 8 per byte; bit 7 keeps the borrow inside the byte)
__device__ __forceinline__ unsigned sext4(unsigned x) { return ((x ^ 0x88888888u) - 0x08080808u) ^ 0x80808080u; }

// a[c] = bytes (antenna 0 ... 3) of column c  ->  b[i] = bytes (column 0 ... 3) of antenna i
__device__ __forceinline__ void transpose4(const unsigned (&a)[4], unsigned (&b)[4])
{
    const unsigned t0 = (a[0] & 0x00FF00FFu) | ((a[1] & 0x00FF00FFu) << 8), t1 = ((a[0] >> 8) & 0x00FF00FFu) | (a[1] & 0xFF00FF00u);
    const unsigned u0 = (a[2] & 0x00FF00FFu) | ((a[3] & 0x00FF00FFu) << 8), u1 = ((a[2] >> 8) & 0x00FF00FFu) | (a[3] & 0xFF00FF00u);
    b[0] = (t0 & 0xFFFFu) | (u0 << 16);
    b[1] = (t1 & 0xFFFFu) | (u1 << 16);
    b[2] = (t0 >> 16) | (u0 & 0xFFFF0000u);
    b[3] = (t1 >> 16) | (u1 & 0xFFFF0000u);
}

__global__ __launch_bounds__(kThreads) void corr_kernel(CorrArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kSet];
    // blockIdx -> (f, p, super-tile): the low 3 bits select f % 8, so the workgroups of one channel -- which read the same lines
    // (the polarisations interleave within them) -- land on the same XCD
    int bid = blockIdx.x;
    const int lo = bid & 7;
    bid >>= 3;
    const int p = bid % a.n_pol;
    bid /= a.n_pol;
    const int n_pairs = a.n_super * (a.n_super + 1) / 2;
    int pair = bid % n_pairs;
    const int f = (bid / n_pairs) * 8 + lo;
    if (f >= a.n_freq) return;
    int sr = 0;
    while (pair > sr) pair -= ++sr;   // pair = sr (sr + 1) / 2 + sc, sc <= sr
    const int sc = pair;
    const bool diag = sr == sc;
    const int n_sets = diag ? 1 : 2;

    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int aq = (l >> 4) + 4 * w;              // this thread's antenna quad within a set
    const int ant0[2] = {sr * kSuper + 4 * aq, sc * kSuper + 4 * aq};
    const size_t col_bytes = (size_t)a.n_ant;     // one column of one channel
    const int T = a.n_cols * a.n_pol;

    unsigned raw[2][2][4];   // [set][half][column of the block]
    auto load_chunk = [&](int k) {
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int s0 = k * kChunk + 4 * ((l & 15) + 16 * half);
            int u = s0 / a.n_cols, r = s0 - u * a.n_cols;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const size_t off = ((size_t)((size_t)u * a.n_freq + f) * T + (size_t)r * a.n_pol + p) * col_bytes;
                const bool in_time = s0 + j < a.S;
#pragma unroll
                for (int set = 0; set < 2; set++) {
                    unsigned v = 0;
                    if (set < n_sets && in_time && ant0[set] < a.n_ant) v = *reinterpret_cast<const unsigned*>(a.in + off + ant0[set]);
                    raw[set][half][j] = v;
                }
                if (++r == a.n_cols) {
                    r = 0;
                    u++;
                }
            }
        }
    };
    auto stage_chunk = [&]() {
#pragma unroll
        for (int set = 0; set < 2; set++) {
            if (set >= n_sets) break;
#pragma unroll
            for (int half = 0; half < 2; half++) {
                unsigned re[4], im[4], tr[4], ti[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    re[j] = sext4((raw[set][half][j] >> 4) & 0x0F0F0F0Fu);
                    im[j] = sext4(raw[set][half][j] & 0x0F0F0F0Fu);
                }
                transpose4(re, tr);
                transpose4(im, ti);
                uint8_t* dst = lds + set * kSet + (4 * aq) * kRow + 4 * ((l & 15) + 16 * half);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    *reinterpret_cast<unsigned*>(dst + i * kRow) = tr[i];
                    *reinterpret_cast<unsigned*>(dst + kPlane + i * kRow) = ti[i];
                }
            }
        }
    };

    v4i acc_re[4], acc_mr[4], acc_rm[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc_re[ct] = acc_mr[ct] = acc_rm[ct] = v4i{0, 0, 0, 0};
    // wave-uniform: does this wave's row tile / column tile ct hold an antenna, and is the tile on or below the diagonal?
    const bool row_live = sr * kSuper + 16 * w < a.n_ant;
    const uint8_t* rowset = lds;
    const uint8_t* colset = lds + (diag ? 0 : kSet);
    const int frag = (l & 15) * kRow + 16 * (l >> 4);

    const int n_chunks = (a.S + kChunk - 1) / kChunk;
    load_chunk(0);
    for (int k = 0; k < n_chunks; k++) {
        stage_chunk();
        __syncthreads();
        if (k + 1 < n_chunks) load_chunk(k + 1);
        if (row_live) {
#pragma unroll
            for (int ks = 0; ks < kChunk / 64; ks++) {
                const v4i a_re = *reinterpret_cast<const v4i*>(rowset + 16 * w * kRow + frag + 64 * ks);
                const v4i a_im = *reinterpret_cast<const v4i*>(rowset + kPlane + 16 * w * kRow + frag + 64 * ks);
#pragma unroll
                for (int ct = 0; ct < 4; ct++) {
                    if ((diag && ct > w) || sc * kSuper + 16 * ct >= a.n_ant) continue;
                    const v4i b_re = *reinterpret_cast<const v4i*>(colset + 16 * ct * kRow + frag + 64 * ks);
                    const v4i b_im = *reinterpret_cast<const v4i*>(colset + kPlane + 16 * ct * kRow + frag + 64 * ks);
                    acc_re[ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_re, b_re, acc_re[ct], 0, 0, 0);
                    acc_re[ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_im, b_im, acc_re[ct], 0, 0, 0);
                    acc_mr[ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_im, b_re, acc_mr[ct], 0, 0, 0);
                    acc_rm[ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_re, b_im, acc_rm[ct], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // D tile: lane l holds column (l & 15), rows 4 (l >> 4) ... + 3 -- row = a1, column = a2
    if (!row_live) return;
    const size_t n_bl = corr_baselines(a.n_ant);
    long long* out = a.vis + ((size_t)f * a.n_pol + p) * n_bl * 2;
#pragma unroll
    for (int ct = 0; ct < 4; ct++) {
        if ((diag && ct > w) || sc * kSuper + 16 * ct >= a.n_ant) continue;
        const int a2 = sc * kSuper + 16 * ct + (l & 15);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int a1 = sr * kSuper + 16 * w + 4 * (l >> 4) + r;
            if (a1 >= a.n_ant || a2 > a1) continue;   // (a2 <= a1 < n_ant: the lower triangle, diagonal included)
            long long* dst = out + ((size_t)a1 * (size_t)(a1 + 1) / 2 + (size_t)a2) * 2;
            long long re = acc_re[ct][r], im = (long long)acc_mr[ct][r] - (long long)acc_rm[ct][r];
            if (a.accumulate) {
                re += dst[0];
                im += dst[1];
            }
            dst[0] = re;
            dst[1] = im;
        }
    }
}

}  // namespace

hipError_t launch_correlate(int n_ant, int n_freq, int n_pol, int n_cols, const void* d_packed, int n_units, long long* d_vis, bool accumulate,
                            hipStream_t s)
{
    if (n_freq <= 0 || n_pol <= 0 || n_cols <= 0 || n_units <= 0 || !d_packed || !d_vis || !corr_supported(n_ant, (long long)n_units * n_cols) ||
        ((uintptr_t)d_packed & 3) || ((uintptr_t)d_vis & 7))
        return hipErrorInvalidValue;
    CorrArgs a;
    a.in = (const uint8_t*)d_packed;
    a.vis = d_vis;
    a.n_ant = n_ant;
    a.n_freq = n_freq;
    a.n_pol = n_pol;
    a.n_cols = n_cols;
    a.S = n_units * n_cols;
    a.n_super = (n_ant + kSuper - 1) / kSuper;
    a.accumulate = accumulate ? 1 : 0;
    const long long grid = (long long)((n_freq + 7) / 8) * 8 * n_pol * (a.n_super * (a.n_super + 1) / 2);
    if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
    (void)hipGetLastError();
    record_launch("corr_kernel");
    hipLaunchKernelGGL(corr_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dsabf
