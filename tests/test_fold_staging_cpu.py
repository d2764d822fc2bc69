"""Host restatement check of the streamed fold kernel's staging (fold_stage_pair, csrc/bf_fold_staging.h; docs/LOG_r09.md section 2).
The header is plain C++ on 32-bit integers, so a small stand-alone program compiles it with the host compiler and runs it over all
2^16 (byte of a, byte of b) pairs that meet in every byte position of the dword -- a's byte p meets b's byte 3 - p, the mirror order --
with the other three bytes of both dwords held at the extreme nibbles, at zero and at pseudo-random values: a carry or a borrow that
crosses a byte shows in a neighbour.  The expected dwords are the unfolded statement of write_chunk's fold branch (the one the
non-stream fold kernel keeps), spelled here per byte on Python integers: offset nibbles N = n + 8 of t = w ^ 0x88, h = 8 N,
(h_a + h_b) - 128 and (h_a + 128 - h_b) - 128 modulo 256 -- and, as a second spelling, 8 (n_a + n_b) and 8 (n_a - n_b) of the signed
nibbles themselves."""
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT

PROGRAM = r"""
#include "bf_fold_staging.h"
#include <cstdio>
#include <vector>
// argv[1]: output file.  stdin-free: the cases are generated here, in the order the test regenerates them.
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    static const uint32_t fills[][2] = {{0x00000000u, 0x00000000u}, {0x88888888u, 0x88888888u}, {0x77777777u, 0x77777777u}, {0x88888888u, 0x77777777u},
                                        {0x77777777u, 0x88888888u}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0x8F70F807u, 0x078F7F80u}, {0x1C96E35Au, 0xB42D69C7u}};
    const dsabf::FoldStageMasks k;
    std::vector<uint32_t> out;
    out.reserve(4u * 8u * 65536u * 4u);
    for (int p = 0; p < 4; p++)
        for (const auto& f : fills)
            for (uint32_t x = 0; x < 256; x++)
                for (uint32_t y = 0; y < 256; y++) {
                    const uint32_t a = (f[0] & ~(0xFFu << (8 * p))) | (x << (8 * p));
                    const uint32_t b = (f[1] & ~(0xFFu << (8 * (3 - p)))) | (y << (8 * (3 - p)));
                    uint32_t sr, si, dr, di;
                    dsabf::fold_stage_pair(a, b, k, sr, si, dr, di);
                    out.push_back(sr), out.push_back(si), out.push_back(dr), out.push_back(di);
                }
    FILE* fp = std::fopen(argv[1], "wb");
    if (!fp) return 3;
    const bool ok = std::fwrite(out.data(), sizeof(uint32_t), out.size(), fp) == out.size();
    return (std::fclose(fp) == 0 && ok) ? 0 : 4;
}
"""
FILLS = [(0x00000000, 0x00000000), (0x88888888, 0x88888888), (0x77777777, 0x77777777), (0x88888888, 0x77777777),
         (0x77777777, 0x88888888), (0xFFFFFFFF, 0xFFFFFFFF), (0x8F70F807, 0x078F7F80), (0x1C96E35A, 0xB42D69C7)]


def cases():
    """(a, b) dwords in the program's order, as uint32 arrays."""
    x, y = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    x, y = x.ravel(), y.ravel()
    a_all, b_all = [], []
    for p in range(4):
        for fa, fb in FILLS:
            a_all.append((np.uint32(fa) & ~np.uint32(0xFF << (8 * p))) | (x << np.uint32(8 * p)))
            b_all.append((np.uint32(fb) & ~np.uint32(0xFF << (8 * (3 - p)))) | (y << np.uint32(8 * (3 - p))))
    return np.concatenate(a_all), np.concatenate(b_all)


def unfolded(a, b):
    """The parent statement per byte, on int64 arrays of bytes [case][4]: the mirror dword's bytes reversed, t = w ^ 0x88, h = 8 N."""
    ab = ((a[:, None] >> (8 * np.arange(4, dtype=np.uint32))) & 0xFF).astype(np.int64)
    bb = ((b[:, None] >> (8 * np.arange(4, dtype=np.uint32))) & 0xFF).astype(np.int64)[:, ::-1]
    ta, tb = ab ^ 0x88, bb ^ 0x88
    hra, hia, hrb, hib = 8 * (ta >> 4), 8 * (ta & 15), 8 * (tb >> 4), 8 * (tb & 15)
    for h in (hra, hia, hrb, hib):
        assert h.min() >= 0 and h.max() <= 120
    sr, si = (hra + hrb - 128) % 256, (hia + hib - 128) % 256
    dr, di = ((hra + 128 - hrb) - 128) % 256, ((hia + 128 - hib) - 128) % 256
    # the same from the signed nibbles: 8 (n_a +- n_b) as two's-complement bytes
    sn = lambda v: ((v & 15) ^ 8) - 8
    assert np.array_equal(sr, (8 * (sn(ab >> 4) + sn(bb >> 4))) % 256) and np.array_equal(dr, (8 * (sn(ab >> 4) - sn(bb >> 4))) % 256)
    assert np.array_equal(si, (8 * (sn(ab) + sn(bb))) % 256) and np.array_equal(di, (8 * (sn(ab) - sn(bb))) % 256)
    pack = lambda v: (v * (256 ** np.arange(4, dtype=np.int64))).sum(axis=1).astype(np.uint32)
    return pack(sr), pack(si), pack(dr), pack(di)


def test_the_folded_staging_equals_the_unfolded_statement_for_every_byte_pair_in_every_position(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe, out = tmp_path / "fold_staging_all_pairs.cpp", tmp_path / "fold_staging_all_pairs", tmp_path / "staged.u32"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "dsabeamformer_amd", "csrc"), str(src), "-o", str(exe)])
    subprocess.check_call([str(exe), str(out)])
    got = np.fromfile(out, dtype=np.uint32).reshape(-1, 4)
    a, b = cases()
    assert got.shape[0] == a.size == 4 * len(FILLS) * 65536
    for name, col, want in zip(("sr", "si", "dr", "di"), got.T, unfolded(a, b)):
        bad = np.flatnonzero(col != want)
        assert bad.size == 0, "%s: %d of %d dwords differ, first a=%08x b=%08x got %08x want %08x" % (
            name, bad.size, col.size, a[bad[0]], b[bad[0]], col[bad[0]], want[bad[0]])
