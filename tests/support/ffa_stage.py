"""What the tests of the periodicity search share (tests/test_ffa_cpu.py, tests/test_gpu_ffa.py): the parity cases, their inputs, and
the driver that pushes one series through an api.PeriodicitySearch in pieces and checks every collected segment against
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


def case_input(name):
    n_beams, n_dm, *_rest = PARITY_CASES[name]
    n_in = PARITY_CASES[name][8]
    return ffa_oracle.parity_input(sum(map(ord, name)), n_dm, n_in, n_beams)


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
