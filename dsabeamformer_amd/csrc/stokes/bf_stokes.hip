// bf_stokes.hip -- device code of the full-Stokes follow-up beams (include/dsabf.h: bf_stokes_*; contract: docs/STOKES.md).
//
// Per unit u, channel f, selected beam k and sample j (the column pair (2j, 2j + 1) = (X, Y)):
//   n[c][k] = sum over antennas of v[u][f][c][a] * w[f][a][beam_k]      (complex, exact integers, no conjugation)
//   I = |X|^2 + |Y|^2   Q = |X|^2 - |Y|^2   U = 2 Re(X conj Y)   V = 2 Im(X conj Y),   summed over windows of n_int samples, int64.
//
// The GEMM runs on v_mfma_i32_16x16x64_i8 (operand maps: bf_fused16.hpp) with TIME as the M axis, the K <= 16 selected beams as the one
// N tile and the antennas as the MFMA's K axis, so the input needs no transpose: lane l loads 16 consecutive packed bytes -- the
// antennas 64 ks + 16 (l >> 4) ... of column (l & 15) of a 16-column tile -- and expands them in registers to the planes re, im and -im
// (the ((x ^ 8) - 8) trick of corr/bf_corr.hip on whole dwords; -im is 8 - (x ^ 8), -7 ... 8, always an int8).  Four MFMAs per 64
// antennas: re = A_re B_wr + A_-im B_wi, im = A_im B_wr + A_re B_wi; the weights are never negated, so -128 is exact.  The B operands
// come from the stage's compact image (bf_stokes_kernels.h), one channel of it in LDS per workgroup, read as one 16-byte word per lane.
//
// In the 16 x 16 accumulator lane l holds beam column (l & 15) and the rows 4 (l >> 4) ... + 3: two whole (X, Y) pairs, so the eight
// products of a pair are formed in the lane, as 32 x 32 -> 64-bit multiply-adds.
//
// Work: a SPAN is 8 integration windows of one (unit, channel) -- 8 n_int samples, n_int whole tiles -- or what is left of them at the
// end of the unit.  The spans in the order (channel, unit, span) are cut into one contiguous range per workgroup, whatever n_freq is; a
// workgroup walks its range channel by channel (one reload of the LDS weights per channel), its four waves taking one span each.
// Where that would leave the chip idle (fewer spans than 8 waves per CU, n_int > 1) the launch is COOPERATIVE instead: a span is the
// smallest run of whole windows that is whole tiles (lcm(n_int, 8) samples), a WORKGROUP takes one span, its four waves take the tiles in
// turn and meet in one image -- four times the waves per window and up to eight times the spans; a lane then finds the window of a tile by
// one division per tile.
// n_int == 1: a lane stores its two samples itself.  n_int > 1: a lane sums consecutive samples of one window in registers and adds the
// sum to the wave's own int64 image of the span's windows in LDS (LDS atomics: the four lane groups of a beam meet there); at the end
// of the span the wave stores the image with plain 8-byte vector stores and zeroes it.  Every output cell is written exactly once.
#include "bf_stokes_kernels.h"
#include "../rec/bf_launch_record.h"

namespace dsabf {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kImage = kStokesWindows * 16 * 4;   // int64 entries of one wave's image: [window][beam column][I, Q, U, V]
typedef int v4i __attribute__((ext_vector_type(4)));
typedef long long i64;
typedef unsigned long long u64;

struct StokesArgs {
    const uint8_t* __restrict__ in;   // [unit][f][2 S][ant]
    const v4i* __restrict__ w;        // the compact weights
    i64* __restrict__ out;            // [unit][t][f][k]{I, Q, U, V}
    int n_ant, n_freq, n_units;
    int S, K, n_int, T;               // samples per unit, beams, window, windows per unit
    int wps, spans;                   // windows per span (8; cooperative: 8 / gcd(n_int, 8)), spans per (unit, channel)
    long long items, per;             // spans of the launch, and of one workgroup
    int mode;                         // kDirect, kPerWave, kCooperative or kVoltages
};

struct GatherArgs {
    const int8_t* __restrict__ w;     // [f][ant][beam]{re, im}
    int8_t* __restrict__ image;
    int beams[kStokesMaxBeams];
    int n_sel, n_ant, n_freq, n_beams, nks;
};

// each byte of x holds a nibble 0 ... 15: the bytes of the result are its two's complement value -8 ... 7, and its negative -7 ... 8
__device__ __forceinline__ unsigned sext4(unsigned x) { return ((x ^ 0x88888888u) - 0x08080808u) ^ 0x80808080u; }
__device__ __forceinline__ unsigned neg4(unsigned x) { return (0x88888888u - (x ^ 0x08080808u)) ^ 0x80808080u; }

__host__ __device__ inline int stokes_weight(const int8_t* w, const int* beams, int n_sel, int n_ant, int n_beams, size_t idx, int nks)
{
    const int j = (int)(idx & 15), l = (int)((idx >> 4) & 63), plane = (int)((idx >> 10) & 1);
    const size_t rest = idx >> 11;
    const int ks = (int)(rest % (size_t)nks);
    const size_t f = rest / (size_t)nks;
    const int ant = kStokesKStep * ks + 16 * (l >> 4) + j, k = l & 15;
    if (k >= n_sel || ant >= n_ant) return 0;
    return w[((f * (size_t)n_ant + (size_t)ant) * (size_t)n_beams + (size_t)beams[k]) * 2 + (size_t)plane];
}

__global__ __launch_bounds__(kThreads) void stokes_gather_kernel(GatherArgs a)
{
    const size_t n = (size_t)a.n_freq * (size_t)a.nks * 2048;
    for (size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (size_t)gridDim.x * kThreads)
        a.image[idx] = (int8_t)stokes_weight(a.w, a.beams, a.n_sel, a.n_ant, a.n_beams, idx, a.nks);
}

// The lane's 16 packed bytes per k-step of one column; zero bytes (a voltage of 0) for an absent column or antenna.
template <int NKS, bool VEC>
__device__ __forceinline__ void load_column(const uint8_t* p, bool valid, int n_ant, int ant0, uint4 (&raw)[NKS])
{
#pragma unroll
    for (int ks = 0; ks < NKS; ks++) {
        const int a0 = ant0 + kStokesKStep * ks;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (VEC) {   // n_ant % 16 == 0 and a 16-byte aligned array: the 16 antennas are there or not, as one
            if (valid && a0 < n_ant) v = *reinterpret_cast<const uint4*>(p + kStokesKStep * ks);
        } else {
            const unsigned* q = reinterpret_cast<const unsigned*>(p + kStokesKStep * ks);
            if (valid && a0 < n_ant) v.x = q[0];
            if (valid && a0 + 4 < n_ant) v.y = q[1];
            if (valid && a0 + 8 < n_ant) v.z = q[2];
            if (valid && a0 + 12 < n_ant) v.w = q[3];
        }
        raw[ks] = v;
    }
}

// n_int == 1; a span per wave; a span per workgroup; the beam samples themselves (the work split of kDirect, out is float2
// [f][k][pol][n_units S]: bf_stokes_voltages_device, docs/COHERENT_DEDISPERSION.md section 1)
enum { kDirect = 0, kPerWave = 1, kCooperative = 2, kVoltages = 3 };

template <int NKS, bool VEC, int MODE>
__global__ __launch_bounds__(kThreads) void stokes_kernel(StokesArgs a)
{
    constexpr bool VOLT = MODE == kVoltages, DIRECT = MODE == kDirect || VOLT, COOP = MODE == kCooperative;
    constexpr int kStep = COOP ? kWaves : 1;              // tiles from one of a wave's tiles to its next
    __shared__ v4i wlds[NKS * 2 * 64];                    // [k-step][re, im][lane]
    __shared__ u64 image[DIRECT ? 1 : kWaves * kImage];   // per wave (cooperative: the first, for all): [window][beam column][I, Q, U, V]
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int k = lane & 15, g = lane >> 4;
    u64* img = image + (MODE == kPerWave ? wave * kImage : 0);
    if (!DIRECT)
        for (int e = threadIdx.x; e < kWaves * kImage; e += kThreads) image[e] = 0;

    const long long per_f = (long long)a.n_units * a.spans;
    const size_t col_bytes = (size_t)a.n_ant, uf_bytes = 2 * (size_t)a.S * col_bytes;
    long long i = (long long)blockIdx.x * a.per;
    const long long end = i + a.per < a.items ? i + a.per : a.items;
    while (i < end) {   // (every condition of the loops around a barrier is the same for all lanes of the workgroup)
        const int f = (int)(i / per_f);
        const long long r = i - (long long)f * per_f;
        const long long seg = end - i < per_f - r ? end - i : per_f - r;   // the spans of this range in channel f
        __syncthreads();   // the channel before is done with the weights
        for (int e = threadIdx.x; e < NKS * 128; e += kThreads) wlds[e] = a.w[(size_t)f * (NKS * 128) + e];
        __syncthreads();

        const int mine = COOP ? 0 : wave;   // the span of the round this wave works on
        for (long long s0 = 0; s0 < seg; s0 += COOP ? 1 : kWaves) {
            const bool live = s0 + mine < seg;
            if (live) {
                const long long it = r + s0 + mine;
                const int u = (int)(it / a.spans), sp = (int)(it - (long long)u * a.spans);
                const int nwin = a.T - a.wps * sp < a.wps ? a.T - a.wps * sp : a.wps;
                const int ntiles = (nwin * a.n_int + 7) >> 3;
                const int tile0 = (sp * a.wps * a.n_int) >> 3;   // the span's first 16-column tile of the (unit, channel): wps * n_int % 8 == 0
                const int tl0 = COOP ? wave : 0;                 // the wave's first tile of the span
                const uint8_t* base = a.in + ((size_t)u * a.n_freq + f) * uf_bytes + (size_t)(16 * g);
                const int n_cols = 2 * a.S;

                // general path: the window and the offset in it of the lane's next sample, the window being summed, and its sums
                int win = (8 * tl0 + 2 * g) / a.n_int, pos = 8 * tl0 + 2 * g - win * a.n_int, cur = win;
                i64 s_px = 0, s_py = 0, s_u = 0, s_v = 0;
                auto flush = [&]() {
                    if (k < a.K && cur < nwin) {
                        u64* d = img + (cur * 16 + k) * 4;
                        atomicAdd(d, (u64)(s_px + s_py));
                        atomicAdd(d + 1, (u64)(s_px - s_py));
                        atomicAdd(d + 2, (u64)(2 * s_u));
                        atomicAdd(d + 3, (u64)(2 * s_v));
                    }
                };

                uint4 raw[NKS], nxt[NKS];
                {
                    const int col = 16 * (tile0 + tl0) + k;
                    load_column<NKS, VEC>(base + (size_t)col * col_bytes, tl0 < ntiles && col < n_cols, a.n_ant, 16 * g, raw);
                }
                for (int tl = tl0; tl < ntiles; tl += kStep) {
                    {   // the wave's next tile's bytes, one tile ahead of the arithmetic
                        const int col = 16 * (tile0 + tl + kStep) + k;
                        load_column<NKS, VEC>(base + (size_t)col * col_bytes, tl + kStep < ntiles && col < n_cols, a.n_ant, 16 * g, nxt);
                    }
                    if (COOP && tl != tl0) {   // the window of the lane's first sample of this tile
                        win = (8 * tl + 2 * g) / a.n_int;
                        pos = 8 * tl + 2 * g - win * a.n_int;
                    }
                    v4i acc_re = {0, 0, 0, 0}, acc_im = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < NKS; ks++) {
                        const unsigned p[4] = {raw[ks].x, raw[ks].y, raw[ks].z, raw[ks].w};
                        v4i a_re, a_im, a_nim;
#pragma unroll
                        for (int d = 0; d < 4; d++) {
                            const unsigned lo = p[d] & 0x0F0F0F0Fu, hi = (p[d] >> 4) & 0x0F0F0F0Fu;
                            a_re[d] = (int)sext4(hi);
                            a_im[d] = (int)sext4(lo);
                            a_nim[d] = (int)neg4(lo);
                        }
                        const v4i b_wr = wlds[(ks * 2 + 0) * 64 + lane], b_wi = wlds[(ks * 2 + 1) * 64 + lane];
                        acc_re = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_re, b_wr, acc_re, 0, 0, 0);
                        acc_re = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_nim, b_wi, acc_re, 0, 0, 0);
                        acc_im = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_im, b_wr, acc_im, 0, 0, 0);
                        acc_im = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_re, b_wi, acc_im, 0, 0, 0);
                    }
                    // rows 4 g ... + 3 of the tile: the samples 8 (tile0 + tl) + 2 g + {0, 1} of the unit, each as (X, Y)
                    if (VOLT) {   // two consecutive samples of X and of Y: 16 bytes each where the pair starts on an even element of memory
                        const int j = 8 * (tile0 + tl) + 2 * g;
                        if (j < a.S && k < a.K) {
                            const size_t nt = (size_t)a.n_units * (size_t)a.S;
                            float2* ox = reinterpret_cast<float2*>(a.out) + ((size_t)f * a.K + k) * 2 * nt + (size_t)u * a.S + j;
                            float2* oy = ox + nt;
                            const bool two = j + 1 < a.S;
                            if (two && !((uintptr_t)ox & 15)) {
                                *reinterpret_cast<float4*>(ox) = make_float4((float)acc_re[0], (float)acc_im[0], (float)acc_re[2], (float)acc_im[2]);
                            } else {
                                ox[0] = make_float2((float)acc_re[0], (float)acc_im[0]);
                                if (two) ox[1] = make_float2((float)acc_re[2], (float)acc_im[2]);
                            }
                            if (two && !((uintptr_t)oy & 15)) {
                                *reinterpret_cast<float4*>(oy) = make_float4((float)acc_re[1], (float)acc_im[1], (float)acc_re[3], (float)acc_im[3]);
                            } else {
                                oy[0] = make_float2((float)acc_re[1], (float)acc_im[1]);
                                if (two) oy[1] = make_float2((float)acc_re[3], (float)acc_im[3]);
                            }
                        }
                    }
#pragma unroll
                    for (int pr = 0; pr < 2 && !VOLT; pr++) {
                        const int xr = acc_re[2 * pr], xi = acc_im[2 * pr], yr = acc_re[2 * pr + 1], yi = acc_im[2 * pr + 1];
                        if (DIRECT) {
                            const int j = 8 * (tile0 + tl) + 2 * g + pr;
                            if (j < a.S && k < a.K) {
                                const i64 px = (i64)xr * xr + (i64)xi * xi, py = (i64)yr * yr + (i64)yi * yi;
                                const i64 uu = (i64)xr * yr + (i64)xi * yi, vv = (i64)xi * yr + (i64)(-xr) * yi;
                                longlong2* o = reinterpret_cast<longlong2*>(a.out + ((((size_t)u * a.T + j) * a.n_freq + f) * a.K + k) * 4);
                                o[0] = make_longlong2(px + py, px - py);
                                o[1] = make_longlong2(2 * uu, 2 * vv);
                            }
                        } else {
                            if (win != cur) {
                                flush();
                                cur = win;
                                s_px = s_py = s_u = s_v = 0;
                            }
                            s_px = (i64)xr * xr + s_px;
                            s_px = (i64)xi * xi + s_px;
                            s_py = (i64)yr * yr + s_py;
                            s_py = (i64)yi * yi + s_py;
                            s_u = (i64)xr * yr + s_u;
                            s_u = (i64)xi * yi + s_u;
                            s_v = (i64)xi * yr + s_v;
                            s_v = (i64)(-xr) * yi + s_v;
                            if (++pos == a.n_int) {
                                pos = 0;
                                win++;
                            }
                        }
                    }
                    if (MODE == kPerWave) {   // on to the lane's first sample of the next tile: 6 samples further
                        pos += 6;
                        while (pos >= a.n_int) {
                            pos -= a.n_int;
                            win++;
                        }
                    }
#pragma unroll
                    for (int ks = 0; ks < NKS; ks++) raw[ks] = nxt[ks];
                }
                if (!DIRECT) flush();
            }
            if (!DIRECT) {
                __syncthreads();   // the LDS atomics are done before the image is read
                if (live) {
                    const long long it = r + s0 + mine;
                    const int u = (int)(it / a.spans), sp = (int)(it - (long long)u * a.spans);
                    const int nwin = a.T - a.wps * sp < a.wps ? a.T - a.wps * sp : a.wps;
                    for (int e = COOP ? (int)threadIdx.x : lane; e < nwin * 64; e += COOP ? kThreads : 64) {
                        const int c = e >> 6, kk = (e >> 2) & 15, s = e & 3;
                        if (kk < a.K) {
                            a.out[((((size_t)u * a.T + (size_t)(a.wps * sp + c)) * a.n_freq + f) * a.K + kk) * 4 + s] = (i64)img[e];
                            img[e] = 0;
                        }
                    }
                }
                __syncthreads();
            }
        }
        i += seg;
    }
}

template <int NKS, bool VEC>
hipError_t launch_n(const StokesArgs& a, unsigned grid, hipStream_t s)
{
    if (a.mode == kDirect) {
        record_launchf("stokes_kernel<%d, %s, %d>", NKS, VEC ? "true" : "false", (int)kDirect);
        hipLaunchKernelGGL((stokes_kernel<NKS, VEC, kDirect>), dim3(grid), dim3(kThreads), 0, s, a);
    } else if (a.mode == kVoltages) {
        record_launchf("stokes_kernel<%d, %s, %d>", NKS, VEC ? "true" : "false", (int)kVoltages);
        hipLaunchKernelGGL((stokes_kernel<NKS, VEC, kVoltages>), dim3(grid), dim3(kThreads), 0, s, a);
    } else if (a.mode == kPerWave) {
        record_launchf("stokes_kernel<%d, %s, %d>", NKS, VEC ? "true" : "false", (int)kPerWave);
        hipLaunchKernelGGL((stokes_kernel<NKS, VEC, kPerWave>), dim3(grid), dim3(kThreads), 0, s, a);
    } else {
        record_launchf("stokes_kernel<%d, %s, %d>", NKS, VEC ? "true" : "false", (int)kCooperative);
        hipLaunchKernelGGL((stokes_kernel<NKS, VEC, kCooperative>), dim3(grid), dim3(kThreads), 0, s, a);
    }
    return hipGetLastError();
}

template <bool VEC>
hipError_t launch_v(const StokesArgs& a, unsigned grid, hipStream_t s)
{
    switch (stokes_ksteps(a.n_ant)) {
        case 1: return launch_n<1, VEC>(a, grid, s);
        case 2: return launch_n<2, VEC>(a, grid, s);
        case 3: return launch_n<3, VEC>(a, grid, s);
        default: return launch_n<4, VEC>(a, grid, s);
    }
}

}  // namespace

void stokes_gather_host(const int8_t* w, const int* beams, int n_sel, int n_ant, int n_freq, int n_beams, int8_t* image)
{
    const int nks = stokes_ksteps(n_ant);
    const size_t n = stokes_weight_bytes(n_ant, n_freq);
    for (size_t idx = 0; idx < n; idx++) image[idx] = (int8_t)stokes_weight(w, beams, n_sel, n_ant, n_beams, idx, nks);
}

hipError_t launch_stokes_gather(const int8_t* d_w, const int* beams, int n_sel, int n_ant, int n_freq, int n_beams, int8_t* d_image, hipStream_t s)
{
    if (!d_w || !beams || !d_image || n_sel < 1 || n_sel > kStokesMaxBeams || n_ant <= 0 || n_ant > kStokesMaxAnt || n_freq <= 0 || n_beams <= 0)
        return hipErrorInvalidValue;
    GatherArgs a;
    a.w = d_w;
    a.image = d_image;
    for (int i = 0; i < kStokesMaxBeams; i++) {
        a.beams[i] = i < n_sel ? beams[i] : 0;
        if (a.beams[i] < 0 || a.beams[i] >= n_beams) return hipErrorInvalidValue;
    }
    a.n_sel = n_sel;
    a.n_ant = n_ant;
    a.n_freq = n_freq;
    a.n_beams = n_beams;
    a.nks = stokes_ksteps(n_ant);
    const size_t n = stokes_weight_bytes(n_ant, n_freq);
    const size_t blocks = (n + kThreads - 1) / kThreads;
    (void)hipGetLastError();
    record_launch("stokes_gather_kernel");
    hipLaunchKernelGGL(stokes_gather_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

namespace {
hipError_t launch_any(int n_ant, int n_freq, int n_cols, int n_sel, int n_int, const void* d_packed, int n_units, const int8_t* d_image,
                      long long* d_out, int n_cus, hipStream_t s, bool voltages);
}

hipError_t launch_stokes(int n_ant, int n_freq, int n_cols, int n_sel, int n_int, const void* d_packed, int n_units, const int8_t* d_image,
                         long long* d_out, int n_cus, hipStream_t s)
{
    if ((uintptr_t)d_out & 15) return hipErrorInvalidValue;
    return launch_any(n_ant, n_freq, n_cols, n_sel, n_int, d_packed, n_units, d_image, d_out, n_cus, s, false);
}

hipError_t launch_stokes_voltages(int n_ant, int n_freq, int n_cols, int n_sel, const void* d_packed, int n_units, const int8_t* d_image,
                                  float* d_out, int n_cus, hipStream_t s)
{
    if (((uintptr_t)d_out & 7) || n_units <= 0 || (long long)n_units * n_cols > 0x7fffffffLL) return hipErrorInvalidValue;
    return launch_any(n_ant, n_freq, n_cols, n_sel, 1, d_packed, n_units, d_image, reinterpret_cast<long long*>(d_out), n_cus, s, true);
}

namespace {
hipError_t launch_any(int n_ant, int n_freq, int n_cols, int n_sel, int n_int, const void* d_packed, int n_units, const int8_t* d_image,
                      long long* d_out, int n_cus, hipStream_t s, bool voltages)
{
    if (n_freq <= 0 || n_units <= 0 || !d_packed || !d_image || !d_out || !stokes_supported(n_ant, 2, n_cols, n_sel, n_int) ||
        ((uintptr_t)d_packed & 3) || ((uintptr_t)d_image & 15))
        return hipErrorInvalidValue;
    StokesArgs a;
    a.in = (const uint8_t*)d_packed;
    a.w = (const v4i*)d_image;
    a.out = d_out;
    a.n_ant = n_ant;
    a.n_freq = n_freq;
    a.n_units = n_units;
    a.S = n_cols;
    a.K = n_sel;
    a.n_int = n_int;
    a.T = n_cols / n_int;
    const long long cap = (long long)(n_cus > 0 ? n_cus : 256) * 8;   // at most 8 workgroups per CU (8 waves per SIMD)
    a.wps = kStokesWindows;
    a.spans = (a.T + a.wps - 1) / a.wps;
    a.items = (long long)n_freq * n_units * a.spans;
    const bool cooperative = n_int > 1 && a.items < cap;   // fewer waves than 8 per CU: a span per workgroup, and shorter spans
    a.mode = voltages ? kVoltages : n_int == 1 ? kDirect : cooperative ? kCooperative : kPerWave;
    if (cooperative) {
        int gcd = 8;
        while (n_int % gcd) gcd >>= 1;
        a.wps = 8 / gcd;   // wps * n_int = lcm(n_int, 8): whole windows and whole tiles
        a.spans = (a.T + a.wps - 1) / a.wps;
        a.items = (long long)n_freq * n_units * a.spans;
        const long long groups = a.items < cap ? a.items : cap;
        a.per = (a.items + groups - 1) / groups;
    } else {
        // one span per wave at least; each workgroup a contiguous range of whole rounds of waves
        const long long want = (a.items + kWaves - 1) / kWaves;
        const long long groups = want < cap ? want : cap;
        a.per = ((a.items + groups - 1) / groups + kWaves - 1) / kWaves * kWaves;
    }
    const unsigned grid = (unsigned)((a.items + a.per - 1) / a.per);
    (void)hipGetLastError();
    return n_ant % 16 == 0 && ((uintptr_t)d_packed & 15) == 0 ? launch_v<true>(a, grid, s) : launch_v<false>(a, grid, s);
}
}  // namespace

}  // namespace dsabf
