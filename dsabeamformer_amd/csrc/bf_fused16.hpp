// bf_fused16.hpp -- the fused expand + complex int8 GEMM + detect kernel (fused16_kernel) as a template, so that its
// instantiations can be spread over several translation units that compile in parallel (bf_fused16_*.hip: one per antenna
// class).  Internal to libdsabf.so; design notes in DESIGN.md section 3 and at the top of bf_kernels.hip.
#pragma once
#include "bf_kernels.h"

#include <hip/hip_runtime.h>

#include "bf_fold_staging.h"

#include <atomic>
#include <type_traits>

#ifndef DSABF_CLOCKPROBE
#define DSABF_CLOCKPROBE 0 // the ONE compile-time switch left in this kernel: a diagnostic build that tools/clock_probe.sh makes beside
#endif                     // the product (-DDSABF_CLOCKPROBE=1: every workgroup overwrites out[blockIdx.x] with its in-kernel shader clock
                           // in GHz, s_memtime / s_memrealtime around the chunk loop; results invalid).  The experiment arms of rounds
                           // 1-5 (5 / 6 MFMAs per conjugate-pair tile, the 4-fragment general image, vector chunk addressing,
                           // sign-extended nibbles in the deep classes, the timing ablations, -DDSABF_WAVES / _NS / _OCC16 builds) were
                           // measured, lost, and are gone: profiles/r0[1-5]_variants_log.txt, docs/LOG_r06.md.

namespace dsabf {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// Detect variants (bf_config.detect_mode): how one sample's power enters the running sum.
constexpr int kDetCanonical = 0;   // xx = x*x; yy = y*y; p = xx + yy; acc += p        (6 VALU ops per complex sample)
constexpr int kDetFast = 1;        // acc = fma(d, d, acc) on the unscaled integers        (4)
constexpr int kDetContracted = 2;  // yy = y*y; p = fma(x, x, yy); acc += p  (nvcc -fmad)  (5)

// Antenna classes (template parameter AIN).  A positive value is a compile-time antenna count: since round 6 only 100 (BASELINE
// config 5, whose 100-byte rows are dword-staged: 3 - 7 % faster than the run-time class that covers them); the compile-time
// classes of 64 / 128 / 192 / 256 antennas measured inside the box noise of the run-time ones and were folded into them
// (profiles/r06_class_fold_ab.txt, r06_ab_fold_c3.txt).  The negative classes take the count from FusedArgs::n_ant at run time:
constexpr int kAntK1P16 = -1;  // <= 64 antennas, n_ant % 16 == 0: one k-step, 16-byte staging pieces
constexpr int kAntK1P4 = -2;   // <= 64 antennas, n_ant % 4 == 0:  one k-step, 4-byte staging pieces
constexpr int kAntK2P16 = -3;  // 65..128 antennas, n_ant % 16 == 0: two k-steps
constexpr int kAntK2P4 = -4;   // 65..128 antennas, n_ant % 4 == 0
constexpr int kAntK4P16 = -5;  // 193..256 antennas, n_ant % 16 == 0: four k-steps (the "deep" classes, round 4)
constexpr int kAntK3P16 = -6;  // 129..192 antennas, n_ant % 16 == 0: three k-steps
constexpr int kAntK4P4 = -7;   // 193..256 antennas, n_ant % 4 == 0: four k-steps, 4-byte staging pieces (round 5)
constexpr int kAntK3P4 = -8;   // 129..192 antennas, n_ant % 4 == 0

// Weight fragments per tile in the two images (weight_relayout16_kernel / weight_relayout16p_kernel, bf_kernels.hip):
constexpr int kGeneralComps = 3;   // Wr, -Wi, Wi: the real row multiplies (Vr | Vi) by (Wr | -Wi), the imaginary row by (Wi | Wr) -- Wr serves both
constexpr int kPairComps = 2;      // Wr, Wi: the conjugate-pair kernel forms +-P2, +-P4 on the VALU
constexpr int kFoldComps = 2;      // (Wr | -Wi), (Wi | Wr) over the 32 mirror pairs: the antenna-fold kernel (weight_relayout16f_kernel)

constexpr unsigned kMagicBits = 0x4B400000u;        // float 12582912 = 1.5 * 2^23
constexpr float kMagic = 12582912.0f;
constexpr float kAlpha = (float)(1.0 / 127.0);      // h_inv_max_value.x, src/beamformer.cu:191
constexpr float kAlpha16 = kAlpha * 0.0625f;        // exact (power-of-two scaling)
constexpr float kNegMagicAlpha16 = -(kMagic * kAlpha16);
constexpr float kNegMagicAlpha = -(kMagic * kAlpha);   // the deep classes stage TRUE nibbles (|16 n| would leave the seed's range)
constexpr float kAlpha8 = kAlpha * 0.125f;          // the antenna-fold kernel stages 8 x (sum | difference of two nibbles)
constexpr float kNegMagicAlpha8 = -(kMagic * kAlpha8);
static_assert((double)kMagic * (double)kAlpha == (double)(kMagic * kAlpha), "K * alpha must be exactly representable");
static_assert((double)kMagic * (double)kAlpha8 == (double)(kMagic * kAlpha8),
              "K * alpha/8 must be exactly representable for the single-fma conversion");
static_assert((double)kMagic * (double)kAlpha16 == (double)(kMagic * kAlpha16),
              "K * alpha/16 must be exactly representable for the single-fma conversion");

struct FusedArgs {
    const uint8_t* __restrict__ in;  // packed voltages [unit][f][t][a]
    const v4i* __restrict__ wimg;    // weight fragment image
    float* __restrict__ out;         // detected [unit*n_out + o][f][b]   (WRITE_C: c[f][t][b]{re,im})
    int n_freq, n_beams, n_bgroups;
    int n_ctiles;                    // 16-beam column tiles = ceil(n_beams / 16) (the last one may be partly filled)
    int n_ptiles;                    // conjugate-pair tiles of 16 base beams = n_beams / 32 (paired kernel only)
    int n_ant;                       // antennas per time sample (the run-time antenna classes read it; AIN > 0 ignores it)
    int T;                           // time samples per gemm-unit
    int t_shift;                     // log2(T) if T is a power of two, else -1
    unsigned S;                      // total time samples per frequency in this launch (n_units * T)
    int chunks_total;                // 128-sample chunks per frequency in this launch
    int n_tsplit;                    // workgroups along time
    int interleave;                  // MFMA column tiles per wave if beams are dealt to them round-robin (beam_of_tile), else 0
    // run-time accumulation window (template NIPO = 0): n_ipo, samples per stream = rt_kout * rt_L, windows per stream, chunks per stream group
    int rt_L, rt_Ls, rt_kout, rt_cpg;
};

// Which beam MFMA column c of MFMA column tile `tile` computes.  A wave owns 16 * NS consecutive beams (paired: 8 * NS base
// beams and their mirror images) in `per` MFMA column tiles (per = NS, paired NS / 2).  Interleaved (per > 0; n_beams a multiple
// of 16 * NS): beam = first + per * c + t, so a lane's results of one output are `per` consecutive floats (paired: per + per)
// -> 16-byte (8-byte for 2) stores, whole 128-byte lines per store instruction, instead of scattered 64-byte rows.
// per = 0: tile t = beams first + 16 t + c.
__host__ __device__ inline int beam_of_tile(int per, int tile, int c)
{
    if (!per) return tile * 16 + c;
    return (tile / per) * (16 * per) + per * c + tile % per;
}

// blockIdx -> (frequency f, beam group bg, time split ts).  Workgroups are dealt round-robin over the 8 XCDs, each
// with its own L2, so blocks b and b+8 share an L2: the low 3 bits of the block index select f % 8 (a frequency
// always lands on the same XCD), and the beam groups / time splits of one frequency are the NEXT-fastest index, so
// every workgroup that needs a frequency's 64-KiB weight panel (and, across beam groups, the same voltages) is
// resident at the same time on the same XCD: the panel is fetched once instead of once per time split
// (FETCH_SIZE 373 MB -> measured in profiles/).  Placement is only a speed matter; any mapping is correct.
__device__ __forceinline__ void decode_block(const FusedArgs& a, int& f, int& bg, int& ts)
{
    int bid = blockIdx.x;
    if ((a.n_freq & 7) == 0) {
        const int lo = bid & 7;
        bid >>= 3;
        bg = bid % a.n_bgroups;
        bid /= a.n_bgroups;
        ts = bid % a.n_tsplit;
        f = (bid / a.n_tsplit) * 8 + lo;
    } else {
        f = bid % a.n_freq;
        bid /= a.n_freq;
        bg = bid % a.n_bgroups;
        ts = bid / a.n_bgroups;
    }
}

// =========================================================================================================
// fused16_kernel -- expand + complex int8 GEMM + detect in one kernel, built on v_mfma_i32_16x16x64_i8.
//
// Why this shape: on random int8 operands the chip holds a higher clock on the 16x16x64 instruction than on
// 32x32x32 (tools/ubench_shape.hip: 129-142 ns vs 149-157 ns per 262,144 MACs per SIMD) and the composite tile
// (MFMA + LDS fragment reads + canonical detect) is 7 % faster (tools/ubench_tile16.hip); a 32x32x32 implementation
// of the same design was measured 4 % (64 antennas) to 5 % (100 antennas) slower on the whole kernel and removed
// (git history, profiles/r01_variants_log.txt).  The 4-register accumulator tile lets one wave cover 64 beams, which
// halves the LDS fragment traffic per MFMA, and the detect of one tile interleaves with the MFMAs of the next in the
// wave's own in-order stream.
//
// Mapping, per group of 64 antennas (K' = 128 = 64 re | 64 im = two MFMAs of K = 64 chained through srcC):
//   A operand: 16 time rows; lane l supplies row l&15, bytes 16*(l>>4).. of the re (s = 0) or im (s = 1) half (LDS piece
//              4*s + (l>>4)).
//   D tile   : lane (column c = l&15, group g = l>>4) holds rows 4g..4g+3 in 4 registers.  Row 4g+r of a tile is
//              position 4*q + r of STREAM g, so every lane accumulates one output at a time, in time order, and a
//              128-row chunk holds 4 streams x 32 positions (n_ipo >= 32) or 2 x 4 streams x 16 positions.
//   A wave   : 4 column tiles = 64 beams; workgroup = 4 waves = 256 beams; chunk = 8 row tiles of 16.
//              (two-k-step classes, where the beams allow: 8 column tiles = 128 beams per wave for the conjugate-pair
//              kernel -- template parameter NS --, else 8 waves = 512 beams per workgroup -- WAVES; bf_kernels.hip)
template <int NIPO>
__device__ __forceinline__ int lds_row16(int t8, int rho)  // row of the chunk image read by A-row rho of tile t8
{
    if constexpr (NIPO >= 32)
        return (rho >> 2) * 32 + 4 * t8 + (rho & 3);
    else
        return (t8 >> 2) * 64 + (rho >> 2) * 16 + 4 * (t8 & 3) + (rho & 3);
}

template <int NIPO>
__device__ __forceinline__ int swz16(int chunk, int row)  // 8 chunks of 16 B per 128-B row; conflict-free both ways
{
    constexpr int LR = NIPO >= 32 ? 32 : 16;  // rows per stream in a chunk
    return chunk ^ ((((row >> 1) & 1) | (((row / LR) & 3) << 1)) ^ ((row & 1) << 2));
}

constexpr int kWaves16 = 4;                  // waves per workgroup of fused16_kernel
constexpr int kThreads16 = 64 * kWaves16;
constexpr int kWavesWide16 = 8;              // ... of the two-k-step classes where the beam count allows (fused_wg_waves)
constexpr int kColTiles16 = 4;               // 16-beam column tiles (output slots) per wave
constexpr int kColTilesWide16 = 8;           // ... of the two-k-step conjugate-pair kernels where the beams allow (fused_col_tiles)

// PAIRED: the steering weights of beam B-1-b are the complex conjugates of those of beam b for every (frequency,
// antenna) -- true for any beam set that is symmetric about the boresight, e.g. the reference's linear fan and 16x16
// grid (checked exactly by pair_check_kernel when the weights are set).  Then with the four REAL K=64 products
//   P1 = sum Wr*Vr, P2 = sum Wi*Vi, P3 = sum Wr*Vi, P4 = sum Wi*Vr        (one 16x16x64 MFMA each)
// C(b) = (P1 - P2) + j(P3 + P4) and C(B-1-b) = (P1 + P2) + j(P3 - P4): two beams for the MFMA work of one, exact in
// int32 (the +-P2 / +-P4 are 4 integer VALU ops per sample pair; P1 and P3 carry the float seed, P2 and P4 start at 0).
//
// AIN = antenna class (above).  More than 64 antennas are two k-steps of 64: the LDS chunk image
// becomes two 128-row planes (antennas 0-63 | 64-127), every product is a chain of two MFMAs, and the detect -- whose
// cost does not depend on the antenna count -- is amortised over twice the MACs.  100 antennas run as 128 with zero
// weights behind antenna 99; their packed rows (100 B) are only dword-aligned, so they are staged in 4-byte pieces.
template <int AIN>
constexpr int ant_ksteps()
{
    if (AIN > 0) return (AIN + 63) / 64;
    return (AIN == kAntK4P16 || AIN == kAntK4P4) ? 4 : (AIN == kAntK3P16 || AIN == kAntK3P4) ? 3 : (AIN == kAntK2P16 || AIN == kAntK2P4) ? 2 : 1;
}
template <int AIN>
constexpr bool ant_two_ksteps() { return ant_ksteps<AIN>() == 2; }
// Three and four k-steps (129 ... 256 antennas; round 4): the same weight-stationary kernel, always on 8-wave workgroups (their
// LDS image -- 2 buffers x 3 | 4 planes of 16 KiB -- leaves one workgroup per CU).  A wave owns TWO output slots (general kernel:
// 24 weight registers per k-step; four slots = two pair tiles for the conjugate-pair kernel), its voltages are staged as true
// nibble values (sign-extended once per workgroup: the 16 x nibble operands of the shallower classes would carry |16 n| past the
// 2^22 the float seed covers), and the detect -- whose cost does not depend on the antenna count -- is amortised over 3 - 4 x
// the MACs of the 64-antenna kernel.
template <int AIN>
constexpr bool ant_deep() { return ant_ksteps<AIN>() > 2; }

// Waves per SIMD the register allocation is held to (= resident workgroups per CU).  Two k-steps: 2 (their 64 KiB of LDS
// allow no more).  One k-step: 3 -- except where 4 fit without a spill: since round 3's 3-fragment weight image the general
// kernel of the 16-byte-staged classes needs 124 VGPRs for n_ipo 8 / 16 / 32 (the conjugate-pair kernel always did), and the
// fourth resident workgroup is worth 2 % (canonical) to 3 % (contracted) on C3 (profiles/r03_ab_c3_general_occ4.txt).  The
// other window lengths and the dword-staged class would spill at 128 and stay at 3.
template <int AIN, int NIPO, bool WRITE_C, int NS = kColTiles16>
constexpr int fused_min_waves()
{
    if (NS == 8 || ant_ksteps<AIN>() >= 2) return 2;
    if (AIN == kAntK1P16 && (NIPO == 8 || NIPO == 16 || NIPO == 32) && !WRITE_C) return 4;
    return 3;   // 168 VGPRs
}

//
// WAVES = waves per workgroup (4, or 8 where fused_wg_waves() in bf_kernels.hip says so): a workgroup stages one frequency's
// voltages for 64 * WAVES beams.
// NS = 16-beam output slots per wave (4, or 8 where fused_col_tiles() says so): a wave's LDS fragment reads feed NS (paired: NS / 2)
// MFMA column tiles.
//
// FOLD (fused16_fold_kernel below; 64 antennas): the array is point-symmetric about its phase centre, W[f][63-a][b] = conj(W[f][a][b])
// (any regular line or grid; checked exactly by fold_check_kernel when the weights are set).  With S = V[a] + V[63-a] and
// D = V[a] - V[63-a] over the 32 mirror pairs, re(b) = sum Wr*Sr - Wi*Di and im(b) = sum Wi*Dr + Wr*Si: ONE K = 64 MFMA each, on the
// operands (Sr | Di) x (Wr | -Wi) and (Dr | Si) x (Wi | Wr) -- the MFMA count of the conjugate-pair kernel without its integer
// +-P2 / +-P4, for any beam set.  The sums and differences are formed while the chunk is staged (write_chunk), in units of 8.
// The kernel's text is bf_fused16_body.inc, included into both kernels below: as a function template shared by the two it compiled
// fused16_kernel's existing instantiations to another instruction schedule, and their code is pinned (tests/test_isa_guard_cpu.py).
template <int AIN, int NIPO, bool WRITE_C, int MODE = kDetCanonical, bool PAIRED = false, int WAVES = kWaves16, int NS = kColTiles16>
__global__ __launch_bounds__(64 * WAVES, (fused_min_waves<AIN, NIPO, WRITE_C, NS>())) void fused16_kernel(FusedArgs a)
{
    constexpr bool FOLD = false, STREAM = false;
#include "bf_fused16_body.inc"
}

// The antenna-fold kernel (FOLD above): 64 mirror-symmetric antennas, n_ipo 16 / 32 / 64, general (non-paired) tiles on the launch
// shape of the 64-antenna class -- same grid, block and LDS bytes as the conjugate-pair kernel of the configuration.
template <int NIPO>
struct FoldShape {   // the body's other compile-time parameters (members of a dependent type: the branches it discards stay unchecked)
    static constexpr int AIN = kAntK1P16, WAVES = kWaves16, NS = kColTiles16;
    static constexpr bool WRITE_C = false, PAIRED = false;
};
template <int NIPO, int MODE>
__global__ __launch_bounds__(kThreads16, (fused_min_waves<kAntK1P16, NIPO, false>())) void fused16_fold_kernel(FusedArgs a)
{
    constexpr int AIN = FoldShape<NIPO>::AIN, WAVES = FoldShape<NIPO>::WAVES, NS = FoldShape<NIPO>::NS;
    constexpr bool WRITE_C = FoldShape<NIPO>::WRITE_C, PAIRED = FoldShape<NIPO>::PAIRED, FOLD = true, STREAM = false;
#include "bf_fused16_body.inc"
}

// The antenna-fold kernel for gemm-units of whole chunk spans (T % 128 == 0; n_ipo 64: T % 256 == 0 -- every production geometry):
// the same sums, detect and stores; the chunk addressing is scalar state that advances by a constant, both prefetch loads are
// unconditional and back to back, and the chunk loop waits for global memory once, where the staging first reads the prefetched
// registers (STREAM in bf_fused16_body.inc; tests/test_isa_fold_stream_cpu.py).  Other gemm-units keep fused16_fold_kernel and its
// per-row addressing.  A kernel of its own name in a translation unit of its own (bf_fused16_k1p16_fold_stream.hip): the nine
// fused16_fold_kernel instantiations and their code stay what they were.
template <int NIPO>
constexpr unsigned fold_stream_span() { return NIPO == 64 ? 256u : 128u; }
template <int NIPO, int MODE>
__global__ __launch_bounds__(kThreads16, (fused_min_waves<kAntK1P16, NIPO, false>())) void fused16_fold_stream_kernel(FusedArgs a)
{
    constexpr int AIN = FoldShape<NIPO>::AIN, WAVES = FoldShape<NIPO>::WAVES, NS = FoldShape<NIPO>::NS;
    constexpr bool WRITE_C = FoldShape<NIPO>::WRITE_C, PAIRED = FoldShape<NIPO>::PAIRED, FOLD = true, STREAM = true;
#include "bf_fused16_body.inc"
}

template <int AIN, int NIPO, bool WRITE_C, int MODE, bool PAIRED, int WAVES, int NS>
hipError_t launch_fused16_t(const FusedArgs& args, const LaunchShape& ls, hipStream_t s)
{
    auto kern = fused16_kernel<AIN, NIPO, WRITE_C, MODE, PAIRED, WAVES, NS>;
    if (ls.block != 64 * WAVES || (args.interleave && args.interleave != (PAIRED ? NS / 2 : NS))) return hipErrorInvalidValue;
    if (ls.lds_bytes > 48 * 1024) {   // once per kernel and device, not per launch (the two-k-step image is always 64 KiB)
        static std::atomic<unsigned> done_mask{0};
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned bit = 1u << (dev & 31);
        if (dev >= 32 || !(done_mask.load(std::memory_order_acquire) & bit)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               ls.lds_bytes);
            if (e != hipSuccess) return e;
            done_mask.fetch_or(bit, std::memory_order_release);
        }
    }
    (void)hipGetLastError();   // clear what earlier, unrelated calls left behind: return this launch's own status
    hipLaunchKernelGGL(kern, dim3(ls.grid), dim3(ls.block), ls.lds_bytes, s, args);
    return hipGetLastError();
}

template <int NIPO, int MODE>
hipError_t launch_fused16_fold_t(const FusedArgs& args, const LaunchShape& ls, hipStream_t s)
{
    if (ls.block != kThreads16 || args.n_ant != 64 || (args.interleave && args.interleave != kColTiles16) || ls.lds_bytes > 48 * 1024)
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL((fused16_fold_kernel<NIPO, MODE>), dim3(ls.grid), dim3(ls.block), ls.lds_bytes, s, args);
    return hipGetLastError();
}

// (the streamed kernel never tests a sample against the launch's end: whole spans only, and chunks that hold nothing else)
template <int NIPO, int MODE>
hipError_t launch_fused16_fold_stream_t(const FusedArgs& args, const LaunchShape& ls, hipStream_t s)
{
    if (ls.block != kThreads16 || args.n_ant != 64 || (args.interleave && args.interleave != kColTiles16) || ls.lds_bytes > 48 * 1024)
        return hipErrorInvalidValue;
    if (args.T <= 0 || (unsigned)args.T % fold_stream_span<NIPO>() != 0 || args.chunks_total <= 0 ||
        (unsigned long long)args.chunks_total * kRowsPerChunk != args.S)
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL((fused16_fold_stream_kernel<NIPO, MODE>), dim3(ls.grid), dim3(ls.block), ls.lds_bytes, s, args);
    return hipGetLastError();
}

// One entry of the variant table: the kernel symbol (for hipFuncGetAttributes) and its launcher.
using fused_launch_fn = hipError_t (*)(const FusedArgs&, const LaunchShape&, hipStream_t);
struct FusedVariant {
    const void* fn = nullptr;
    fused_launch_fn launch = nullptr;
    // the instantiation's template arguments, in the kernel's own order: what the census (bf_variant_key, tests/test_census_cpu.py,
    // profiles/r06_instantiations.txt) compares with the kernel symbols of the shipped library
    int ain = 0, nipo = 0, write_c = 0, mode = 0, paired = 0, waves = 0, ns = 0;
    int fold = 0;   // 1: fused16_fold_kernel<nipo, mode>; 2: fused16_fold_stream_kernel<nipo, mode> (the same family under the same key)
};

template <int AIN, int NIPO, bool WRITE_C, int MODE, bool PAIRED, int WAVES, int NS = kColTiles16>
FusedVariant make_variant()
{
    return FusedVariant{reinterpret_cast<const void*>(fused16_kernel<AIN, NIPO, WRITE_C, MODE, PAIRED, WAVES, NS>),
                        launch_fused16_t<AIN, NIPO, WRITE_C, MODE, PAIRED, WAVES, NS>, AIN, NIPO, WRITE_C, MODE, PAIRED, WAVES, NS};
}

template <int AIN, int NIPO, int WAVES>
FusedVariant fused16_variant_nipo(bool write_c, int mode, bool paired)
{
    if (write_c) {   // stage parity: general kernel, canonical scale, 4 waves
        if constexpr (WAVES == kWaves16) return make_variant<AIN, NIPO, true, kDetCanonical, false, WAVES>();
        return FusedVariant{};
    }
    if constexpr (NIPO >= 16 || NIPO == 0) {   // (a run-time window: the caller asks for the fast detect only from 16 samples on)
        if (mode == kDetFast)
            return paired ? make_variant<AIN, NIPO, false, kDetFast, true, WAVES>() : make_variant<AIN, NIPO, false, kDetFast, false, WAVES>();
    }
    if (mode == kDetContracted)
        return paired ? make_variant<AIN, NIPO, false, kDetContracted, true, WAVES>()
                      : make_variant<AIN, NIPO, false, kDetContracted, false, WAVES>();
    return paired ? make_variant<AIN, NIPO, false, kDetCanonical, true, WAVES>() : make_variant<AIN, NIPO, false, kDetCanonical, false, WAVES>();
}

// Every instantiation of one antenna class (n_ipo 2 ... 64, general / conjugate-pair, three detect modes, stage parity).
// mode: kDet*; the fast detect falls back to canonical below n_ipo = 16 (include/dsabf.h).
template <int AIN>
FusedVariant fused16_variant(int n_ipo, bool write_c, int mode, bool paired)
{
    switch (n_ipo) {
        case 2: return fused16_variant_nipo<AIN, 2, kWaves16>(write_c, mode, paired);
        case 4: return fused16_variant_nipo<AIN, 4, kWaves16>(write_c, mode, paired);
        case 8: return fused16_variant_nipo<AIN, 8, kWaves16>(write_c, mode, paired);
        case 16: return fused16_variant_nipo<AIN, 16, kWaves16>(write_c, mode, paired);
        case 32: return fused16_variant_nipo<AIN, 32, kWaves16>(write_c, mode, paired);
        case 64: return fused16_variant_nipo<AIN, 64, kWaves16>(write_c, mode, paired);
        default: return fused16_variant_nipo<AIN, 0, kWaves16>(write_c, mode, paired);   // run-time window (the caller passes n_ipo = 0)
    }
}

// The conjugate-pair kernel with 8 output slots per wave (two-k-step classes, n_ipo >= 16; fused_col_tiles() in bf_kernels.hip).
// ... where its 236-256 registers hold without a spill: not the run-time dword-staged class (13 staging pieces per thread:
// 60-412 bytes of scratch per lane) and not 100 antennas at n_ipo 64 (140); those keep 4 slots on 8-wave workgroups.
template <int AIN, int NIPO>
constexpr bool ns8_fits() { return AIN == kAntK2P16 || (AIN == 100 && NIPO < 64); }

template <int AIN, int NIPO>
FusedVariant fused16_variant_ns8_nipo(int mode)
{
    if constexpr (!ns8_fits<AIN, NIPO>()) return FusedVariant{};
    else {
    if (mode == kDetFast) return make_variant<AIN, NIPO, false, kDetFast, true, kWaves16, kColTilesWide16>();
    if (mode == kDetContracted) return make_variant<AIN, NIPO, false, kDetContracted, true, kWaves16, kColTilesWide16>();
    return make_variant<AIN, NIPO, false, kDetCanonical, true, kWaves16, kColTilesWide16>();
    }
}

// The wide launches of the two-k-step classes (n_ipo >= 16), each kind in translation units of its own because each wants a
// different instruction scheduling strategy (dsabeamformer_amd/build.py): 8-wave workgroups (fused_wg_waves() in
// bf_kernels.hip), general kernel ...
template <int AIN, int NIPO, bool PAIRED>
FusedVariant fused16_variant_w8_nipo(int mode)
{
    if (mode == kDetFast) return make_variant<AIN, NIPO, false, kDetFast, PAIRED, kWavesWide16>();
    if (mode == kDetContracted) return make_variant<AIN, NIPO, false, kDetContracted, PAIRED, kWavesWide16>();
    return make_variant<AIN, NIPO, false, kDetCanonical, PAIRED, kWavesWide16>();
}

// (PAIRED = false: bf_fused16_*_w8.hip; true, the conjugate-pair kernel on 8-wave workgroups: bf_fused16_*_w8p.hip)
template <int AIN, bool PAIRED>
FusedVariant fused16_variant_w8(int n_ipo, int mode)
{
    static_assert(ant_two_ksteps<AIN>(), "the wide launches exist for the two-k-step classes only");
    switch (n_ipo) {
        case 16: return fused16_variant_w8_nipo<AIN, 16, PAIRED>(mode);
        case 32: return fused16_variant_w8_nipo<AIN, 32, PAIRED>(mode);
        case 64: return fused16_variant_w8_nipo<AIN, 64, PAIRED>(mode);
        default: return FusedVariant{};
    }
}

// ... and the conjugate-pair kernel on 4-wave workgroups whose waves own 8 output slots (fused_col_tiles()).
template <int AIN>
FusedVariant fused16_variant_s8(int n_ipo, int mode)
{
    static_assert(ant_two_ksteps<AIN>(), "the wide launches exist for the two-k-step classes only");
    switch (n_ipo) {
        case 16: return fused16_variant_ns8_nipo<AIN, 16>(mode);
        case 32: return fused16_variant_ns8_nipo<AIN, 32>(mode);
        case 64: return fused16_variant_ns8_nipo<AIN, 64>(mode);
        default: return FusedVariant{};
    }
}

// The deep classes (three / four k-steps): 8-wave workgroups; general kernel with 2 output slots per wave, conjugate-pair kernel
// with 4 (two pair tiles); n_ipo 16 / 32 / 64.
template <int AIN, int NIPO>
FusedVariant fused16_variant_deep_nipo(int mode, bool paired, int ns)
{
    if (paired && ns == 2) {   // one pair tile per wave: 8 waves x 32 beams = 256 beams per workgroup
        if (mode == kDetFast) return make_variant<AIN, NIPO, false, kDetFast, true, kWavesWide16, 2>();
        if (mode == kDetContracted) return make_variant<AIN, NIPO, false, kDetContracted, true, kWavesWide16, 2>();
        return make_variant<AIN, NIPO, false, kDetCanonical, true, kWavesWide16, 2>();
    }
    if (paired) {
        if (mode == kDetFast) return make_variant<AIN, NIPO, false, kDetFast, true, kWavesWide16, 4>();
        if (mode == kDetContracted) return make_variant<AIN, NIPO, false, kDetContracted, true, kWavesWide16, 4>();
        return make_variant<AIN, NIPO, false, kDetCanonical, true, kWavesWide16, 4>();
    }
    if (mode == kDetFast) return make_variant<AIN, NIPO, false, kDetFast, false, kWavesWide16, 2>();
    if (mode == kDetContracted) return make_variant<AIN, NIPO, false, kDetContracted, false, kWavesWide16, 2>();
    return make_variant<AIN, NIPO, false, kDetCanonical, false, kWavesWide16, 2>();
}
template <int AIN>
FusedVariant fused16_variant_deep(int n_ipo, int mode, bool paired, int ns)
{
    static_assert(ant_deep<AIN>(), "three or four k-steps");
    switch (n_ipo) {
        case 16: return fused16_variant_deep_nipo<AIN, 16>(mode, paired, ns);
        case 32: return fused16_variant_deep_nipo<AIN, 32>(mode, paired, ns);
        case 64:   // (the dword-staged classes would spill at this window -- 12 / 16 staging pieces per thread -- and lose to fusedg_kernel:
                   //  profiles/r05_deep_p4_perf.txt; deep_class() leaves them there)
            if constexpr (AIN == kAntK3P4 || AIN == kAntK4P4) return FusedVariant{};
            else return fused16_variant_deep_nipo<AIN, 64>(mode, paired, ns);
        default: return FusedVariant{};
    }
}
// ns: output slots per wave (general 2; conjugate-pair 4 where the beams come in groups of 512, else 2)
FusedVariant fused16_variant_k4p16(int n_ipo, int mode, bool paired, int ns);
FusedVariant fused16_variant_k3p16(int n_ipo, int mode, bool paired, int ns);
FusedVariant fused16_variant_k4p4(int n_ipo, int mode, bool paired, int ns);
FusedVariant fused16_variant_k3p4(int n_ipo, int mode, bool paired, int ns);

template <int NIPO, int MODE>
FusedVariant make_fold_variant()
{
    return FusedVariant{reinterpret_cast<const void*>(fused16_fold_kernel<NIPO, MODE>), launch_fused16_fold_t<NIPO, MODE>, kAntK1P16, NIPO, 0, MODE,
                        0, kWaves16, kColTiles16, 1};
}
// The antenna-fold kernels: n_ipo 16 / 32 / 64 x the three detect readings (bf_fused16_k1p16_fold.hip); anything else: none.
FusedVariant fused16_variant_k1p16_fold(int n_ipo, int mode);

template <int NIPO, int MODE>
FusedVariant make_fold_stream_variant()
{
    return FusedVariant{reinterpret_cast<const void*>(fused16_fold_stream_kernel<NIPO, MODE>), launch_fused16_fold_stream_t<NIPO, MODE>, kAntK1P16,
                        NIPO, 0, MODE, 0, kWaves16, kColTiles16, 2};
}
// ... and their streamed twins for gemm-units of whole chunk spans (bf_fused16_k1p16_fold_stream.hip).
FusedVariant fused16_variant_k1p16_fold_stream(int n_ipo, int mode);

// One definition per antenna class, each in its own translation unit (bf_fused16_*.hip).
FusedVariant fused16_variant_a100(int n_ipo, bool write_c, int mode, bool paired);
FusedVariant fused16_variant_k1p16(int n_ipo, bool write_c, int mode, bool paired);
FusedVariant fused16_variant_k1p4(int n_ipo, bool write_c, int mode, bool paired);
FusedVariant fused16_variant_k2p16(int n_ipo, bool write_c, int mode, bool paired);
FusedVariant fused16_variant_k2p4(int n_ipo, bool write_c, int mode, bool paired);
// ... and three per two-k-step class for its wide launches (bf_fused16_*_w8.hip, bf_fused16_*_w8p.hip, bf_fused16_*_s8.hip)
FusedVariant fused16_variant_a100_w8(int n_ipo, int mode);
FusedVariant fused16_variant_k2p16_w8(int n_ipo, int mode);
FusedVariant fused16_variant_k2p4_w8(int n_ipo, int mode);
FusedVariant fused16_variant_a100_w8p(int n_ipo, int mode);
FusedVariant fused16_variant_k2p16_w8p(int n_ipo, int mode);
FusedVariant fused16_variant_k2p4_w8p(int n_ipo, int mode);
FusedVariant fused16_variant_a100_s8(int n_ipo, int mode);
FusedVariant fused16_variant_k2p16_s8(int n_ipo, int mode);
FusedVariant fused16_variant_k2p4_s8(int n_ipo, int mode);

}  // namespace dsabf
