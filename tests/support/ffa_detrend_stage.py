"""What the tests of the periodicity search's detrend share (tests/test_ffa_detrend_cpu.py, tests/test_gpu_ffa_detrend.py): the
cases, their inputs, the red-noise case, and the driver that pushes one series through an api.PeriodicitySearch with
bf_ffa_set_detrend and checks every collected segment against tests/support/ffa_detrend_oracle.py."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ffa_detrend_oracle as det
import ffa_oracle
from ffa_stage import BIG_SIZES, SIZES, check_segment, same_candidates

# name: n_beams, n_dm, n_seg, p_lo, p_hi, tdec, n_oct, K, input samples, push sizes (cycled), max_in_flight, blk, win.
#   blk1_win3:   nb = n_seg, a is always 0: trend[u] = fl(r[u] + fl(0 d))
#   blk1_win129: nb = 64 < win: every window is truncated on both sides of some c and on one side of every c; the counts n run
#                65 .. 64 .. 65 over odd and even values, so the lower median of an even count is taken 32 times a segment
#   one_block:   blk = n_seg, nb = 1: r[0] everywhere (k < 0 for the first half, c0 >= nb - 1 = 0 for the second)
#   two_blocks:  blk 256 at n_seg 512, nb = 2: 128 clamped samples, 256 interpolated with every a = 1/512 .. 511/512, 128 clamped.  win 1,
#                so that r = m: any wider window makes r[0] == r[1], the lower median of the same two means, and the span flat
#   win1:        r = m, the median selects each mean itself
#   interior:    n_seg 4096, blk 8, win 129: nb 512, 384 full windows of 129
#   wide:        ffa_stage's `wide` (n_seg 1000, 3 octaves, tdec 4, p 13 .. 31, pushes 64 / 33 / 7 / 1: segments end in mid-push), blk 8, win 9
#   max_*:       n_seg 16384, p 8 .. 9, one octave.  blk 1 win 129: 131072 bytes of LDS (keys and medians of 16384 blocks), the largest
#                there is, and the largest rank count; blk 2: 65536 bytes; blk 16 win 65: 8192, blocks summed with 16-byte loads
#   beams*:      the column indexing of the grid, 3 trials x 4 / 60 / 68 / 256 beams at n_seg 96, blk 4, win 5
CASES = {
    "blk1_win3": (4, 2, 64, 8, 11, 1, 1, 2, 64 * 2 + 5, SIZES, 2, 1, 3),
    "blk1_win129": (4, 2, 64, 8, 11, 1, 1, 2, 64 * 2 + 5, SIZES, 2, 1, 129),
    "one_block": (4, 2, 64, 8, 11, 1, 1, 2, 64 * 2 + 5, SIZES, 2, 64, 3),
    "two_blocks": (8, 1, 512, 8, 11, 1, 1, 2, 512 * 2 + 5, SIZES, 2, 256, 1),
    "win1": (4, 2, 64, 8, 11, 1, 1, 2, 64 * 2 + 5, SIZES, 2, 4, 1),
    "interior": (4, 1, 4096, 64, 66, 1, 1, 3, 4096 + 9, BIG_SIZES, 2, 8, 129),
    "wide": (8, 1, 1000, 13, 32, 4, 3, 3, 1000 * 4 + 203, [64, 33, 7, 1], 1, 8, 9),
    "max_blk1": (4, 1, 16384, 8, 10, 1, 1, 3, 16384 + 40, BIG_SIZES, 2, 1, 129),
    "max_blk2": (4, 1, 16384, 8, 10, 1, 1, 3, 16384 + 40, BIG_SIZES, 2, 2, 129),
    "max_blk16": (4, 1, 16384, 8, 10, 1, 1, 3, 16384 + 40, BIG_SIZES, 2, 16, 65),
    "beams4": (4, 3, 96, 8, 13, 1, 1, 2, 96 * 2 + 5, SIZES, 2, 4, 5),
    "beams60": (60, 3, 96, 8, 13, 1, 1, 2, 96 * 2 + 5, SIZES, 2, 4, 5),
    "beams68": (68, 3, 96, 8, 13, 1, 1, 2, 96 * 2 + 5, SIZES, 2, 4, 5),
    "beams256": (256, 3, 96, 8, 13, 1, 1, 2, 96 + 5, SIZES, 2, 4, 5),
}
# Which rule of the contract a case's input can tell from its mutant (ffa_detrend_oracle.mutant_changes; asserted in
# tests/test_ffa_detrend_cpu.py, which also asserts that the cases NOT listed change nothing -- they are no test of that rule):
#   upper:    needs a window of even count, i.e. a truncated one: not win 1 (win1, two_blocks), and not one_block (nb = 1)
#   constant: needs an interpolated span with a != 0 or two different medians side by side: not blk 1 ... but there r[u // 1] = r[u]
#             IS the contract's fl(r[u] + 0 d) unless that sum changes -0 to +0, so blk 1 is left out; and not nb = 1
#   fused:    needs a != 0: blk >= 2 and nb >= 2
COVERS = {
    "upper": sorted(set(CASES) - {"win1", "two_blocks", "one_block"}),
    "constant": sorted(set(CASES) - {"blk1_win3", "blk1_win129", "max_blk1", "one_block"}),
    "fused": sorted(set(CASES) - {"blk1_win3", "blk1_win129", "max_blk1", "one_block"}),
}


def case_cfg(name):
    """(tdec, n_seg, n_oct, p_lo, p_hi, K), (blk, win)."""
    _, _, n_seg, p_lo, p_hi, tdec, n_oct, K, _, _, _, blk, win = CASES[name]
    return (tdec, n_seg, n_oct, p_lo, p_hi, K), (blk, win)


@functools.lru_cache(maxsize=None)
def case_input(name):
    n_beams, n_dm, *_ = CASES[name]
    x = ffa_oracle.parity_input(sum(map(ord, name)) + 1000, n_dm, CASES[name][8], n_beams)
    x.setflags(write=False)
    return x


# ---- the red-noise case (docs/PERIODICITY.md section 1a) -------------------------------------------------------------------------
RED_CFG, RED_DETREND = (1, 1024, 1, 16, 24, 3), (8, 9)
RED_PERIOD, RED_BEAM, RED_HEIGHT = 19.37, 2, 4.0


@functools.lru_cache(maxsize=None)
def red_noise_input(height=RED_HEIGHT):
    """One trial x 1024 samples x 4 beams: N(0,1) noise, 40 sin(2 pi t / 700) and half a random walk in every beam; in beam RED_BEAM
    alone a train of one-sample pulses of `height` at period RED_PERIOD."""
    rng = np.random.default_rng(2024)
    n = RED_CFG[1]
    t = np.arange(n)
    x = rng.standard_normal((1, n, 4)) + 40.0 * np.sin(2.0 * np.pi * t / 700.0)[None, :, None] + 0.5 * np.cumsum(rng.standard_normal((1, n, 4)), axis=1)
    x[0, np.round(np.arange(3.0, n - 1, RED_PERIOD)).astype(int), RED_BEAM] += height
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def best_per_beam(cands):
    """{beam: (snr, period_rows)} of a candidate list (ffa_oracle.select tuples or a CAND_DTYPE array)."""
    out = {}
    for c in cands:
        beam, snr, period = (int(c["beam"]), float(c["snr"]), float(c["period_rows"])) if isinstance(c, np.void) else (c[4], c[10], c[2])
        if beam not in out or snr > out[beam][0]:
            out[beam] = (snr, period)
    return out


def run_stage(torch, bf, x, cfg, detrend, sizes, max_in_flight, t_offset=0, log=None, want=None, set_detrend="ctor", **kw):
    """ffa_stage.run_stage with the detrend: pushes x [n_dm][T][n_b] through a PeriodicitySearch in pieces `sizes` (cycled) on two
    alternating HIP streams without synchronisation, collects a segment only when the next push needs its result set, and checks every
    segment against the detrend oracle (`want`: its segments, if the caller has them already): records to the bit, statistics to
    n_seg 2^-52, candidates to the bit against the oracle's selection over the device's records.  detrend = (blk, win) or None;
    set_detrend: "ctor" (api's argument), "call" (set_detrend after the constructor) or "never".  Returns the number of segments."""
    from dsabeamformer_amd import api

    tdec, n_seg, n_oct, p_lo, p_hi, K = cfg
    n_dm, T, n_b = x.shape
    blk, win = detrend if detrend else (0, 0)
    if want is None:
        want = det.Search(x, tdec, n_seg, n_oct, p_lo, p_hi, K, blk, win, t_offset=t_offset, **kw).segments()
    if set_detrend == "ctor":
        ffa = api.PeriodicitySearch(bf, n_dm, tdec, n_seg, n_oct, p_lo, p_hi, K, max(sizes), max_in_flight=max_in_flight, detrend=detrend, **kw)
    else:
        ffa = api.PeriodicitySearch(bf, n_dm, tdec, n_seg, n_oct, p_lo, p_hi, K, max(sizes), max_in_flight=max_in_flight, **kw)
        if set_detrend == "call":
            ffa.set_detrend(blk, win)
    assert ffa.detrend == (detrend if blk else None)
    streams = [torch.cuda.Stream() for _ in range(2)]
    keep, at, k, done, pending = [], 0, 0, 0, 0

    def collect():
        nonlocal done, pending
        cands = ffa.collect()
        rec = ffa.last_records()
        check_segment(rec, cands, want[done], cfg, (done, cfg, detrend, n_dm, n_b), kw.get("dm_first", 0), kw.get("threshold", 8.0))
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
        while pending and pending + completes > max_in_flight:
            collect()
        chunk = torch.from_numpy(np.array(x[:, at:at + n])).cuda()    # (a copy) [n_dm][n][n_b], as bf_dm_stream_push emits it
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
