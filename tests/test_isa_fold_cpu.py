"""CPU-box guard on the antenna-fold kernel (fused16_fold_kernel, csrc/bf_fused16.hpp; n_ipo 32, canonical reading: the instantiation
the default 64-antenna configuration runs): the properties its speed rests on, read from the shipped gfx950 code object like
tests/test_isa_guard_cpu.py does -- and the symmetry that selects it, stated in numpy on the weights the oracle makes."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402

FOLD = "_ZN5dsabf19fused16_fold_kernelILi32ELi0EEEvNS_9FusedArgsE"
PAIR = "_ZN5dsabf14fused16_kernelILin1ELi32ELb0ELi0ELb1ELi4ELi4EEEvNS_9FusedArgsE"


@pytest.fixture(scope="module")
def objects():
    from dsabeamformer_amd import build

    build.build()
    wd = tempfile.mkdtemp(prefix="isafold")
    cos = {}
    for unit in ("bf_fused16_k1p16_fold", "bf_fused16_k1p16"):
        co = isa_report.code_object(os.path.join(ROOT, "dsabeamformer_amd", "build", unit + ".hip.o"), wd)
        cos[unit] = (co, isa_report.kernels(co))
    return cos


def chunk_loop(co, name):
    """Mnemonics of the kernel's chunk loop: the innermost loop (backward branch and its target) that holds every MFMA."""
    txt = subprocess.check_output([os.path.join(isa_report.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + name, co],
                                  text=True)
    start, insts = None, []                       # (offset inside the kernel, mnemonic, branch target offset or None)
    for line in txt.splitlines():
        m = re.match(r"^([0-9a-f]+) <%s>:" % re.escape(name), line)
        if m:
            start = int(m.group(1), 16)
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\b.*//\s*([0-9A-Fa-f]+):", line)
        if m and start is not None:
            t = re.search(r"<%s\+0x([0-9a-f]+)>" % re.escape(name), line)
            insts.append((int(m.group(2), 16) - start, m.group(1), int(t.group(1), 16) if t and "branch" in m.group(1) else None))
    mfma = [off for off, op, _ in insts if op.startswith("v_mfma")]
    loops = [(tgt, off) for off, op, tgt in insts if tgt is not None and tgt <= mfma[0] and off >= mfma[-1]]
    assert loops, "no loop around the MFMAs of %s" % name
    lo, hi = min(loops, key=lambda l: l[1] - l[0])
    return [op for off, op, _ in insts if lo <= off <= hi]


def valu(ops):
    return sum(1 for o in ops if o.startswith("v_") and not o.startswith("v_mfma"))


def test_fold_kernel_keeps_four_waves_per_simd_and_one_mfma_per_output_row(objects):
    co, ks = objects["bf_fused16_k1p16_fold"]
    assert sorted(ks) == sorted("_ZN5dsabf19fused16_fold_kernelILi%dELi%dEEEvNS_9FusedArgsE" % (n, m) for n in (16, 32, 64) for m in (0, 1, 2))
    k = ks[FOLD]
    assert k["vgpr_count"] + k["agpr_count"] <= 128, k               # 4 waves per SIMD, as the pair kernel it replaces
    assert k["private_segment_fixed_size"] == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("vgpr_spill_count", 0) == 0
    ops = isa_report.disassembly(co, FOLD)
    assert isa_report.count(ops, "scratch_") == 0
    loop = chunk_loop(co, FOLD)
    # 8 row tiles x 4 column tiles x (re row, im row): one K = 64 MFMA each, all of them in the chunk loop
    assert isa_report.count(loop, "v_mfma_i32_16x16x64_i8") == 64 and isa_report.count(ops, "v_mfma") == 64
    assert isa_report.count(ops, "v_pk_[a-z]+_f32") == 0
    assert isa_report.count(ops, r"v_fma_f32|v_fmac_f32") == 0, "a contracted multiply-add in the canonical detect"


def test_fold_loop_issues_fewer_vector_instructions_than_the_pair_loop(objects):
    """What the kernel is for: the pair kernel's 256 integer +- per (wave, chunk) are gone, the staging of sums and differences
    adds about 60 -- at least 150 fewer vector instructions in the chunk loop, same build, same detect."""
    fold = chunk_loop(*[objects["bf_fused16_k1p16_fold"][0], FOLD])
    pair = chunk_loop(*[objects["bf_fused16_k1p16"][0], PAIR])
    assert isa_report.count(pair, "v_mfma") == 64
    for f32 in ("v_fmamk_f32", "v_mul_f32", "v_add_f32"):            # the canonical detect is the same 768 operations in both
        assert isa_report.count(fold, f32) == isa_report.count(pair, f32), f32
    print("chunk loop VALU: pair %d, fold %d" % (valu(pair), valu(fold)))
    assert valu(fold) <= valu(pair) - 150, (valu(fold), valu(pair))


def mirror_symmetric(w):
    """numpy statement of fold_check_kernel: W[f][A-1-a][b] == conj(W[f][a][b]) for every f, a, b."""
    return np.array_equal(w[:, ::-1, :, 0], w[..., 0]) and np.array_equal(w[:, ::-1, :, 1].astype(np.int16), -w[..., 1].astype(np.int16))


def test_regular_arrays_have_the_antenna_symmetry(orc):
    sys.path.insert(0, ROOT)
    import bench

    g = orc.Geom(n_avg=16, n_out_per_gemm=16)
    assert g.n_ant == 64 and g.n_beams == 256
    w = orc.make_weights(g, orc.default_positions(64), orc.default_directions(256), 0)
    assert w.shape == (g.n_freq, 64, 256, 2) and mirror_symmetric(w)
    pos, dirs = bench.grid_100()                                      # a 10 x 10 grid (BASELINE config 5)
    g5 = orc.Geom(n_beams=512, n_ant=100, n_freq=16, n_avg=16, n_out_per_gemm=8)
    w5 = orc.make_weights(g5, pos, dirs, 0)
    assert mirror_symmetric(w5)
    w5[3, 10, 7, 1] += 1                                              # ... and the statement notices one component off by one
    assert not mirror_symmetric(w5)
