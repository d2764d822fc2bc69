"""What the tests of the periodicity search share (tests/test_ffa_cpu.py, tests/test_gpu_ffa.py, tests/test_gpu_ffa_shapes.py): the
parity cases and the edge cases, their inputs, and the driver that pushes one series through an api.PeriodicitySearch in pieces and checks every collected segment against
tests/support/ffa_oracle.py."""
from __future__ import annotations

import numpy as np
import pytest

import ffa_oracle

SIZES = [1, 7, 33, 64]

# name: n_beams, n_dm, n_seg, p_lo, p_hi, tdec, n_oct, K, input samples, push sizes (cycled), max_in_flight.
#   beams: 4 (one lane), 60 (less than a beam-lane group of 64), 64, 68 (one group and a lane of the next workgroup), 256
#   wide: p 13 .. 31 at 1000 samples crosses M = 64 -> 32 (octave 0), 32 -> 16 (octave 1), 16 -> 8 (octave 2); 1000 is no multiple of any M p
#   two_rows: p_hi - 1 = 48 = L / 2; p 25 .. 48 have M = 2, the first merge level is the last (20 .. 24 have M = 4: with two rows
#             alone there is one add per cell and no association to get wrong)
#   input lengths leave a decimation group AND a segment open at the end; 7 and 33 cut groups of 3 and 4 in two, and every
#   segment but a case's first starts in mid-push
PARITY_CASES = {
    "one_lane": (4, 1, 64, 8, 13, 1, 1, 1, 64 * 3 + 11, SIZES, 2),
    "octaves": (60, 3, 96, 8, 13, 3, 3, 3, 96 * 3 * 2 + 50, SIZES, 2),
    "wide": (64, 1, 1000, 13, 32, 4, 3, 3, 1000 * 4 + 203, [64, 33, 7, 1], 1),
    "two_rows": (68, 3, 96, 20, 49, 1, 1, 3, 96 * 2 + 5, SIZES, 3),
    "many_beams": (256, 1, 64, 8, 13, 4, 1, 3, 64 * 4 * 2 + 9, [33, 64, 1, 7], 2),
    # one push of 200 completes segments 0, 1, 2 (64 samples each); then 7 + 64 complete the fourth
    "three_at_once": (4, 3, 64, 8, 13, 1, 1, 3, 271, [200, 7, 64], 3),
}


BIG_SIZES = [4096, 33, 1000, 7]      # for n_seg >= 2048: a segment in a few dozen launches, not hundreds
DEC_SIZES = [64, 1, 600, 7]          # against groups of 200 / 256: 64 + 1 leave a group open, 600 closes it, completes others, opens one

# The edges of the contract the kernels branch on (tests/test_gpu_ffa_shapes.py), the same layout.  NOT in PARITY_CASES:
# test_every_parity_input_tells_a_left_fold_from_the_contract walks that table, and fold_left at M = 2048 builds a 268 MB index table.
#   k*:     ffa_search_kernel<K>, K = 1 .. 6, each at the smallest p_lo it allows (2^(K-1) = p_lo / 2 from K = 3 on); K = 4, 5, 6 write
#           2, 3, 4 ping-pong boxcar passes; k6_p64 has p = 64 (pw_log by the branch), 65, 66 (a second bin for lanes 0 and 0, 1)
#   p*:     both sides of p = 64; 2 .. 8 bins per lane with a ragged last stride; p = 511, the largest
#   lds_*:  M p = 6144 = 64 * 96: 2 * 6144 * 4 = 49152 bytes of dynamic LDS, exactly the 48 KiB a kernel gets unasked; and
#           M p = 6160 = 16 * 385: 49280 bytes, the opt-in by the smallest margin.  lds_just_over is the ONLY case above 48 KiB with K = 2,
#           so it is the first launch of ffa_search_kernel<2> that needs the opt-in in whatever order the cases run -- keep it that way
#   timed_geometry: docs/PERIODICITY.md section 8's n_seg, K, octaves, tdec and its first periods, on 4 columns (64 KiB)
#   max_seg: 128 KiB, M = 2048 rows at p = 8 (the largest shift a record carries), six octaves; max_seg_p511: 130816 bytes, and five
#           octaves because a sixth would hold fewer than two rows of 510
#   tdec*:  groups far longer than most pushes: several consecutive pushes leave one group open (carry in -> carry out), and a push of
#           600 closes it, completes one or two more and opens the next; the cycle is 672 rows, so the cuts fall at every place of a group
EDGE_CASES = {
    "k1_p8": (4, 2, 64, 8, 11, 1, 1, 1, 64 * 2 + 5, SIZES, 2),
    "k2_p8": (4, 2, 64, 8, 11, 1, 1, 2, 64 * 2 + 5, SIZES, 2),
    "k3_p8": (4, 2, 64, 8, 11, 1, 1, 3, 64 * 2 + 5, SIZES, 2),
    "k4_p16": (4, 2, 128, 16, 19, 1, 1, 4, 128 * 2 + 5, SIZES, 2),
    "k5_p32": (4, 2, 256, 32, 35, 1, 1, 5, 256 * 2 + 5, SIZES, 2),
    "k6_p64": (4, 2, 512, 64, 67, 1, 1, 6, 512 * 2 + 5, SIZES, 2),
    "p63_66": (8, 1, 2048, 63, 67, 1, 2, 5, 2048 + 9, BIG_SIZES, 2),
    "p127_130": (8, 1, 2048, 127, 131, 1, 2, 6, 2048 + 9, BIG_SIZES, 2),
    "p255_258": (8, 1, 2048, 255, 259, 1, 2, 6, 2048 + 9, BIG_SIZES, 2),
    "p508_511": (8, 1, 2048, 508, 512, 1, 2, 6, 2048 + 9, BIG_SIZES, 2),
    "lds_48k_exact": (4, 1, 6144, 96, 97, 1, 1, 2, 6144 + 3, BIG_SIZES, 2),
    "lds_just_over": (4, 1, 6160, 385, 386, 1, 1, 2, 6160 + 3, BIG_SIZES, 2),
    "timed_geometry": (4, 1, 8192, 64, 68, 4, 3, 5, 8192 * 4 + 17, BIG_SIZES, 2),
    "max_seg": (4, 1, 16384, 8, 10, 1, 6, 3, 16384 + 40, BIG_SIZES, 2),
    "max_seg_p511": (4, 1, 16384, 510, 512, 1, 5, 6, 16384 + 40, BIG_SIZES, 2),
    "tdec256": (8, 2, 32, 8, 10, 256, 1, 2, 32 * 256 * 2 + 300, DEC_SIZES, 2),
    "tdec200": (8, 2, 64, 8, 11, 200, 2, 3, 64 * 200 * 2 + 77, DEC_SIZES, 2),
}
# The selection threshold of a case: 3.0 as in the parity test.  With M <= 4 rows (n_seg 32) no S/N of tdec256 reaches it, so that
# case lets every column through and the candidate path is still compared.
EDGE_THRESHOLDS = {"tdec256": -1e300}


def case_of(name):
    """The tuple of `name`, from whichever table holds it."""
    return PARITY_CASES[name] if name in PARITY_CASES else EDGE_CASES[name]


def case_cfg(name):
    """cfg of run_stage: (tdec, n_seg, n_oct, p_lo, p_hi, K)."""
    _, _, n_seg, p_lo, p_hi, tdec, n_oct, K, *_ = case_of(name)
    return (tdec, n_seg, n_oct, p_lo, p_hi, K)


def case_threshold(name):
    return EDGE_THRESHOLDS.get(name, 3.0)


def case_input(name):
    n_beams, n_dm, *_rest = case_of(name)
    n_in = case_of(name)[8]
    return ffa_oracle.parity_input(sum(map(ord, name)), n_dm, n_in, n_beams)


def case_lds_bytes(name, rows_of=ffa_oracle.rows_of):
    """Dynamic LDS of the case's octave 0 as the launcher sizes it: both copies of the largest fold, rounded up to 16 bytes."""
    _, _, n_seg, p_lo, p_hi, *_ = case_of(name)
    return 2 * ((max(rows_of(n_seg, p) * p for p in range(p_lo, p_hi)) + 3) & ~3) * 4


def case_max_rows(name):
    _, _, n_seg, p_lo, p_hi, *_ = case_of(name)
    return max(ffa_oracle.rows_of(n_seg, p) for p in range(p_lo, p_hi))


def same_candidates(a, b):
    """Two candidate arrays from the library, field by field (the struct's padding bytes are nobody's)."""
    return len(a) == len(b) and all(a[f].tobytes() == b[f].tobytes() for f in ffa_oracle.CAND_FIELDS)


def check_segment(rec, cands, w, cfg, where=(), dm_first=0, threshold=8.0):
    """One collected segment against the oracle's dict w: records to the bit, statistics to a relative n_seg 2^-52; the candidates,
    bit for bit, against the oracle's selection over the DEVICE's records (its fp64 statistics may differ from numpy's in the last
    bits, and the S/N with them)."""
    tdec, n_seg, n_oct, p_lo, p_hi, K = cfg
    assert (rec["first_row"], rec["n_rows"]) == (w["first_row"], w["n_rows"]), where
    assert np.array_equal(rec["value"].view(np.uint32), w["value"].view(np.uint32)), where
    assert np.array_equal(rec["shift"], w["shift"]) and np.array_equal(rec["bin"], w["bin"]), where
    rtol = n_seg * 2.0 ** -52
    for f in ("sum", "sumsq"):
        err = np.abs(rec[f] - w[f]) / np.maximum(np.abs(w[f]), 1e-300)
        print("ffa %s %s: worst relative error %.3g (bound %.3g)" % (where, f, err.max(), rtol))
        assert np.allclose(rec[f], w[f], rtol=rtol, atol=0.0), (where, f)
    ffa_oracle.assert_candidates_equal(cands, ffa_oracle.select(rec["value"], rec["shift"], rec["bin"], rec["sum"], rec["sumsq"], tdec, n_seg, p_lo,
                                                                 rec["first_row"], dm_first, threshold))


def run_stage(torch, bf, x, cfg, sizes, max_in_flight, t_offset=0, log=None, eager=False, **kw):
    """Pushes x [n_dm][T][n_b] through a PeriodicitySearch in pieces `sizes` (cycled) on two alternating HIP streams without
    synchronisation, collects a segment only when the next push needs its result set (or, `eager`, as soon as it is pending), and
    checks every segment against the oracle.  cfg = (tdec, n_seg, n_oct, p_lo, p_hi, K).  Returns the number of segments."""
    from dsabeamformer_amd import api

    tdec, n_seg, n_oct, p_lo, p_hi, K = cfg
    n_dm, T, n_b = x.shape
    want = ffa_oracle.Search(x, tdec, n_seg, n_oct, p_lo, p_hi, K, t_offset=t_offset, **kw).segments()
    ffa = api.PeriodicitySearch(bf, n_dm, tdec, n_seg, n_oct, p_lo, p_hi, K, max(sizes), max_in_flight=max_in_flight, **kw)
    streams = [torch.cuda.Stream() for _ in range(2)]
    keep, at, k, done, pending = [], 0, 0, 0, 0

    def collect():
        nonlocal done, pending
        cands = ffa.collect()
        rec = ffa.last_records()
        check_segment(rec, cands, want[done], cfg, (done, cfg, n_dm, n_b), kw.get("dm_first", 0), kw.get("threshold", 8.0))
        # the stage's candidates: the library's own selection over the device's records
        mine = api.PeriodicitySearch.select((rec["value"], rec["shift"], rec["bin"]), (rec["sum"], rec["sumsq"]), tdec, n_seg, p_lo,
                                            rec["first_row"], kw.get("dm_first", 0), kw.get("threshold", 8.0))
        assert same_candidates(cands, mine)
        if log is not None:
            log.append((want[done], rec, cands))
        done += 1
        pending -= 1

    while at < T:
        n = min(sizes[k % len(sizes)], T - at)
        completes = (at + n) // (n_seg * tdec) - at // (n_seg * tdec)
        while pending and (eager or pending + completes > max_in_flight):
            collect()
        chunk = torch.from_numpy(np.ascontiguousarray(x[:, at:at + n])).cuda()    # [n_dm][n][n_b], as bf_dm_stream_push emits it
        keep.append(chunk)
        ffa.push(chunk, n, t_offset + at, streams[k % 2].cuda_stream)
        pending += completes
        assert ffa.pending == pending
        at += n
        k += 1
    while pending:
        collect()
    assert done == len(want) == T // (n_seg * tdec)
    with pytest.raises(Exception, match="no segment is pending"):
        ffa.collect()
    ffa.close()
    return done
