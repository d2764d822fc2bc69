"""CPU-box guard on the streamed antenna-fold kernels (fused16_fold_stream_kernel, csrc/bf_fused16.hpp: the fold kernel of gemm-units
of whole chunk spans, the bench line's among them): what their chunk loop must not contain, read from the shipped gfx950 code object
with tools/isa_report.py as tests/test_isa_fold_cpu.py does.  docs/PERF_MODEL.md section 4: every memory operation of the steady
state unconditional -- a load under a branch, or behind a zero-initialised destination, makes the compiler wait with vmcnt(0) beside
it; docs/LOG_r08.md section 1 has what that cost the fold kernel."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402

NIPOS, MODES = (16, 32, 64), (0, 1, 2)                       # modes: canonical, fast, contracted
STREAM = "_ZN5dsabf26fused16_fold_stream_kernelILi%dELi%dEEEvNS_9FusedArgsE"
FOLD = "_ZN5dsabf19fused16_fold_kernelILi%dELi%dEEEvNS_9FusedArgsE"
KERNELS = [(n, m) for n in NIPOS for m in MODES]


@pytest.fixture(scope="module")
def objects():
    from dsabeamformer_amd import build

    build.build()
    wd = tempfile.mkdtemp(prefix="isafoldstream")
    cos = {}
    for unit in ("bf_fused16_k1p16_fold_stream", "bf_fused16_k1p16_fold"):
        co = isa_report.code_object(os.path.join(ROOT, "dsabeamformer_amd", "build", unit + ".hip.o"), wd)
        cos[unit] = (co, isa_report.kernels(co))
    return cos


def chunk_loop(co, name):
    """[(offset, mnemonic, operand text, branch target or None)] of the kernel's chunk loop: the innermost loop (backward branch and
    its target) that holds every MFMA."""
    txt = subprocess.check_output([os.path.join(isa_report.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + name, co],
                                  text=True)
    start, insts = None, []
    for line in txt.splitlines():
        m = re.match(r"^([0-9a-f]+) <%s>:" % re.escape(name), line)
        if m:
            start = int(m.group(1), 16)
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\b(.*)//\s*([0-9A-Fa-f]+):", line)
        if m and start is not None:
            t = re.search(r"<%s\+0x([0-9a-f]+)>" % re.escape(name), line)
            insts.append((int(m.group(3), 16) - start, m.group(1), m.group(2).strip(), int(t.group(1), 16) if t and "branch" in m.group(1) else None))
    mfma = [off for off, op, _, _ in insts if op.startswith("v_mfma")]
    loops = [(tgt, off) for off, op, _, tgt in insts if tgt is not None and tgt <= mfma[0] and off >= mfma[-1]]
    assert loops, "no loop around the MFMAs of %s" % name
    lo, hi = min(loops, key=lambda l: l[1] - l[0])
    return [i for i in insts if lo <= i[0] <= hi]


def ops_of(loop):
    return [op for _, op, _, _ in loop]


def valu(ops):
    return sum(1 for o in ops if o.startswith("v_") and not o.startswith("v_mfma"))


def test_the_unit_holds_the_nine_streamed_kernels_and_nothing_else(objects):
    _, ks = objects["bf_fused16_k1p16_fold_stream"]
    assert sorted(ks) == sorted(STREAM % k for k in KERNELS)


@pytest.mark.parametrize("nipo,mode", KERNELS, ids=["nipo%d-mode%d" % k for k in KERNELS])
def test_chunk_loop_waits_for_global_memory_once_and_addresses_on_the_scalar_unit(objects, nipo, mode):
    co, ks = objects["bf_fused16_k1p16_fold_stream"]
    name = STREAM % (nipo, mode)
    k = ks[name]
    assert k["vgpr_count"] + k["agpr_count"] <= 128, k               # four waves per SIMD
    assert k["private_segment_fixed_size"] == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
    loop = chunk_loop(co, name)
    ops = ops_of(loop)
    assert isa_report.count(ops, "v_mfma_i32_16x16x64_i8") == 64 and isa_report.count(isa_report.disassembly(co, name), "v_mfma") == 64
    # the prefetch: two 16-byte loads, back to back as far as waiting goes
    loads = [i for i, (_, op, _, _) in enumerate(loop) if re.match(r"(global|buffer)_load_dwordx4$", op)]
    assert len(loads) == 2, [loop[i] for i in loads]
    assert isa_report.count(ops, r"(global|buffer|flat)_load") == 2, "a load of another width in the chunk loop"
    waits = [i for i, (_, op, text, _) in enumerate(loop) if op == "s_waitcnt" and "vmcnt" in text]
    assert len(waits) == 1, [loop[i] for i in waits]                 # the one in front of the staging's first read of the prefetch
    assert not loads[0] < waits[0] < loads[1], "a wait for global memory between the two prefetch loads"
    for op in ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32"):
        assert isa_report.count(ops, op) == 0, op + " in the chunk loop: vector addressing"
    # no inner loop: the only backward branch of the loop is the one that closes it
    lo, hi = loop[0][0], loop[-1][0]
    back = [(off, tgt) for off, _, _, tgt in loop if tgt is not None and lo <= tgt <= off]
    assert back == [(hi, lo)], back
    print("%s: chunk loop VALU %d, VGPRs %d" % (name, valu(ops), k["vgpr_count"]))
    assert valu(ops) <= 880, valu(ops)                               # the fold kernel's fast path executes 906 per wave and chunk


@pytest.mark.parametrize("nipo", NIPOS)
def test_canonical_detect_is_the_fold_kernels(objects, nipo):
    """The same 768 fp32 operations per chunk as fused16_fold_kernel's canonical detect: nothing contracted, nothing dropped."""
    stream = ops_of(chunk_loop(objects["bf_fused16_k1p16_fold_stream"][0], STREAM % (nipo, 0)))
    fold = ops_of(chunk_loop(objects["bf_fused16_k1p16_fold"][0], FOLD % (nipo, 0)))
    for f32 in ("v_fmamk_f32", "v_mul_f32", "v_add_f32"):
        assert isa_report.count(stream, f32) == isa_report.count(fold, f32), f32
    if nipo == 32:
        assert [isa_report.count(stream, f32) for f32 in ("v_fmamk_f32", "v_mul_f32", "v_add_f32")] == [256, 256, 252]
