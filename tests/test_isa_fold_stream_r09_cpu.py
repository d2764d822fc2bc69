"""CPU-box guard on what round 9 took out of the streamed antenna-fold kernels' chunk loop (docs/LOG_r09.md): the staging of a dword
pair in 16 vector operations instead of 21 (csrc/bf_fold_staging.h), no register copies beside the prefetch, LDS addresses that
step between the buffers in registers, one 64-bit vector add per parked store, the next row tile's fragments requested one tile early
with one stated wait per tile.  Read from the shipped gfx950 code object the way
tests/test_isa_fold_stream_cpu.py reads it (its chunk_loop: the innermost loop around the MFMAs, cold branches included).

PARENT_VALU are the nine loops' vector-instruction counts in the build of the parent commit, read there with the same function and
tabled in docs/LOG_r09.md section 1; the round claims 22 fewer in every instantiation: 20 in the staging (4 dword pairs x 5), the 2
copies.  The bound is parent - 22, not a number read from this tree."""
import os
import sys
import tempfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402
from test_isa_fold_stream_cpu import KERNELS, STREAM, chunk_loop, ops_of, valu  # noqa: E402

PARENT_VALU = {(16, 0): 859, (16, 1): 619, (16, 2): 731, (32, 0): 860, (32, 1): 612, (32, 2): 732, (64, 0): 872, (64, 1): 620, (64, 2): 744}
CLAIMED = 22
# ... and their s_waitcnt instructions that name lgkmcnt, same build, same table: the fragment prefetch of section 3 must not add any
PARENT_LGKM_WAITS = {(16, 0): 16, (16, 1): 16, (16, 2): 9, (32, 0): 16, (32, 1): 16, (32, 2): 10, (64, 0): 16, (64, 1): 16, (64, 2): 10}


@pytest.fixture(scope="module")
def stream_unit():
    from dsabeamformer_amd import build

    build.build()
    co = isa_report.code_object(os.path.join(ROOT, "dsabeamformer_amd", "build", "bf_fused16_k1p16_fold_stream.hip.o"), tempfile.mkdtemp(prefix="isar09"))
    return co, isa_report.kernels(co)


@pytest.mark.parametrize("nipo,mode", KERNELS, ids=["nipo%d-mode%d" % k for k in KERNELS])
def test_chunk_loop_lost_the_claimed_vector_instructions_and_kept_its_registers(stream_unit, nipo, mode):
    co, ks = stream_unit
    name = STREAM % (nipo, mode)
    k = ks[name]
    assert k["vgpr_count"] + k["agpr_count"] <= 128, k               # four waves per SIMD
    assert k["private_segment_fixed_size"] == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
    loop = chunk_loop(co, name)
    ops = ops_of(loop)
    print("%s: chunk loop VALU %d (parent %d), VGPRs %d" % (name, valu(ops), PARENT_VALU[(nipo, mode)], k["vgpr_count"]))
    assert valu(ops) <= PARENT_VALU[(nipo, mode)] - CLAIMED, (valu(ops), PARENT_VALU[(nipo, mode)])
    # where they went: fold_stage_pair is 16 operations, 3 of them plain adds / subtracts, so the loop's shifts, bit operations and
    # byte permutes are 4 x 13 at the most (the parent's statement: 4 x 17 beside 4 x 4 adds / subtracts), and no register is copied
    bit_ops = sum(isa_report.count(ops, op) for op in ("v_xor_b32", "v_and_b32", "v_or_b32", "v_and_or_b32", "v_bitop3_b32", "v_lshrrev_b32",
                                                       "v_lshlrev_b32", "v_add_lshl_u32", "v_perm_b32"))
    assert bit_ops <= 4 * 13, bit_ops
    assert isa_report.count(ops, "v_mov_b32") == 0
    # the staging stores and the fragment reads are still LDS instructions (typed pointers, not flat ones), and the parked store global
    assert isa_report.count(ops, "ds_write_b128") == 4 and isa_report.count(ops, "ds_read_b128") == 16
    assert isa_report.count(ops, "flat_") == 0 and isa_report.count(ops, "global_store") >= 1
    # the fragments of a row tile are requested one tile early and waited for once, where the tile opens
    lgkm = sum(1 for _, op, text, _ in loop if op == "s_waitcnt" and "lgkmcnt" in text)
    assert lgkm <= PARENT_LGKM_WAITS[(nipo, mode)], (lgkm, PARENT_LGKM_WAITS[(nipo, mode)])
