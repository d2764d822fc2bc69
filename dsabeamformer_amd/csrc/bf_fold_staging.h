// bf_fold_staging.h -- the antenna-fold staging of one dword pair, as the streamed fold kernel issues it (fused16_fold_stream_kernel,
// STREAM in bf_fused16_body.inc; docs/LOG_r09.md section 2).  Plain C++ on 32-bit integers: the kernel includes it through
// bf_fused16.hpp, tests/test_fold_staging_cpu.py compiles it on the host and runs it over every byte pair in every byte position.
//
// a = packed bytes of antennas 4 d ... 4 d + 3 of a row (re: bits 4-7, im: bits 0-3, two's-complement nibbles n in [-8, 7]),
// b = the packed bytes of their four mirror antennas, still in ascending antenna order (the function reverses them).  Per byte of
// the results: sr = 8 (n_re(a) + n_re(b)),  dr = 8 (n_re(a) - n_re(b)),  si, di: the same of the im nibbles -- two's-complement int8.
//
// The offset nibble N = n + 8 in [0, 15] is the nibble's bits with the top one flipped, so "mask the field, flip its top bit, set a
// guard bit above it" is (x & mask) ^ constant: ONE three-input bit operation (v_bitop3_b32) per field, with no w ^ 0x88 in front.
//   p  = 128 + 8 Nre(a)   from a >> 1: serves the sum AND the difference
//   rb = 8 Nre(b)         from reversed b >> 1
//   p + rb = 128 + 8 (Nre(a) + Nre(b)) in [128, 368]: the byte is sr, bit 8 lands in bit 0 of the next byte (whose bits 0-2 are 0 in
//            both operands, so it goes no further) and the mask 0xF8 takes it off; bit 8 of the top byte leaves the dword
//   p - rb = 128 + 8 (Nre(a) - Nre(b)) in [8, 248]: no borrow; ^ 0x80 gives dr
//   jp = 16 + Nim(a), jb = Nim(b): the im nibbles where they are, no shift.  (jp + jb) << 3 = 128 + 8 (Nim(a) + Nim(b)) per byte in one
//            v_add_lshl_u32, bit 8 masked off as above; jp - jb in [1, 31], << 3 in [8, 248], ^ 0x80 gives di
// 16 operations where the statement in write_chunk (bf_fused16_body.inc, kept by the non-stream fold kernel) takes 21.  Every constant
// is an operand, not a literal: the kernel holds them in vector registers formed once per workgroup.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DSABF_STAGE_FN __host__ __device__ __forceinline__
#else
#define DSABF_STAGE_FN inline
#endif

namespace dsabf {

struct FoldStageMasks {
    uint32_t m78 = 0x78787878u;   // 8 N: bits 3-6 of a byte
    uint32_t kC0 = 0xC0C0C0C0u;   // ... top bit of the field flipped (0x40), guard bit 0x80 set
    uint32_t k40 = 0x40404040u;   // ... top bit of the field flipped
    uint32_t f0f = 0x0F0F0F0Fu;   // N of the im nibble, in place
    uint32_t k18 = 0x18181818u;   // ... top bit flipped (0x08), guard bit 0x10 set
    uint32_t k08 = 0x08080808u;
    uint32_t h80 = 0x80808080u;
    uint32_t f8 = 0xF8F8F8F8u;    // a staged byte is a multiple of 8
    uint32_t rev = 0x00010203u;   // v_perm_b32 selector: the bytes of the second operand in reverse order
};

DSABF_STAGE_FN void fold_stage_pair(const uint32_t a, const uint32_t b, const FoldStageMasks& k, uint32_t& sr, uint32_t& si, uint32_t& dr,
                                    uint32_t& di)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t br = __builtin_amdgcn_perm(0u, b, k.rev);
#else
    const uint32_t br = __builtin_bswap32(b);
#endif
    const uint32_t p = ((a >> 1) & k.m78) ^ k.kC0;
    const uint32_t rb = ((br >> 1) & k.m78) ^ k.k40;
    const uint32_t jp = (a & k.f0f) ^ k.k18;
    const uint32_t jb = (br & k.f0f) ^ k.k08;
    sr = (p + rb) & k.f8;
    dr = (p - rb) ^ k.h80;
    si = ((jp + jb) << 3) & k.f8;
    di = ((jp - jb) << 3) ^ k.h80;
}

}  // namespace dsabf
