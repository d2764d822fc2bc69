"""GPU tests (-m gpu) of the periodicity search on the shapes its kernels branch on (docs/PERIODICITY.md sections 1 and 4): every
compiled ffa_search_kernel<K>, K = 1 .. 6 (one to four ping-pong boxcar passes); periods on both sides of 64 and up to 511 (the
pw_log branch, and lanes that walk bins j, j + 64, ...); segments whose dynamic LDS is exactly 48 KiB, just above it (the launcher's
opt-in), 64 KiB at the geometry docs/PERIODICITY.md section 8 times, and the contract's largest (n_seg 16384: 128 KiB, M = 2048
rows, six octaves); decimation groups of 200 and 256 samples that several consecutive pushes leave open; and a column that holds
no finite sample.  The cases are tests/support/ffa_stage.py's EDGE_CASES; driver and checks are that file's run_stage and
check_segment, as in tests/test_gpu_ffa.py: records bit-equal to tests/support/ffa_oracle.py, statistics to n_seg 2^-52,
candidates bit for bit over the device's records.  tests/test_ffa_cpu.py asserts for the inputs that a left-to-right fold and a
reversed decimation give other bits, and that the LDS cases sit where their names say."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import ffa_oracle  # noqa: E402
from ffa_stage import EDGE_CASES, case_cfg, case_input, case_threshold, run_stage  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _bf(bfmod, n_beams):
    return bfmod.Beamformer(bfmod.debug_config(n_beams=n_beams, n_freq=8))


@pytest.mark.sweep_cap(len(EDGE_CASES))
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_every_width_period_and_segment_edge_to_the_bit(torch, bfmod, case):
    """One EDGE_CASES entry through the stage in its own pushes, alternating over two streams without synchronisation: every
    segment's records equal the oracle's bit for bit, and every case yields candidates (dm_first and a first_t beyond 2^40 label
    them)."""
    n_beams, n_dm, _, _, _, _, _, _, _, sizes, mif = EDGE_CASES[case]
    bf = _bf(bfmod, n_beams)
    log = []
    n = run_stage(torch, bf, case_input(case), case_cfg(case), sizes, mif, t_offset=2 ** 40 + 5, dm_first=17, threshold=case_threshold(case), log=log)
    assert n >= 1 and sum(len(c) for _, _, c in log) > 0
    for _, _, c in log:
        assert np.all(c["first_row"] >= 2 ** 40) and np.all((c["dm"] >= 17) & (c["dm"] < 17 + n_dm))
    bf.close()


def test_a_wholly_non_finite_column_stays_in_range_and_alone(torch, bfmod):
    """8 beams x 2 trials, n_seg 64, p 8 .. 10, K 3, two segments.  Column (trial 0, beam 3) is NaN throughout and (trial 1, beam 6)
    is -inf throughout, so every fold cell of theirs is NaN / -inf.  docs/PERIODICITY.md section 1: the value of such a column's
    records is unspecified, shift < M and bin < p hold all the same, and the column yields no candidate.  The other 14 columns are
    what the oracle gives for them alone, bit for bit -- a neighbour's NaN reaches no other column (the decimation reads four beams
    per lane, the maxima cross lanes) -- and their candidates are the oracle's selection over the device's records."""
    from dsabeamformer_amd import api

    n_beams, n_dm, n_seg, thr = 8, 2, 64, 3.0
    cfg = (1, n_seg, 1, 8, 11, 3)
    x = ffa_oracle.parity_input(1234, n_dm, 2 * n_seg + 5, n_beams)
    bad = [(0, 3), (1, 6)]
    x[0, :, 3] = np.nan
    x[1, :, 6] = -np.inf
    good = np.array([d * n_beams + b for d in range(n_dm) for b in range(n_beams) if (d, b) not in bad])
    alone = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(1, x.shape[1], n_dm * n_beams)[:, :, good])      # [1][T][14]
    want = ffa_oracle.Search(alone, *cfg, threshold=thr).segments()
    assert len(want) == 2 and all(len(w["cands"]) > 0 for w in want)
    # no S/N of the 14 columns within a relative 1e-7 of the threshold: the device's statistics, an ulp or so off the oracle's exact
    # ones, cannot put a column on the other side of it
    snr = np.array([c[10] for w in ffa_oracle.Search(alone, *cfg, threshold=-np.inf).segments() for c in w["cands"]])
    assert snr.size == 2 * len(good) and np.all(np.abs(snr - thr) > 1e-7 * thr)
    rows =np.array([ffa_oracle.rows_of(n_seg, p) for p in range(8, 11)])

    bf = _bf(bfmod, n_beams)
    ffa = api.PeriodicitySearch(bf, n_dm, *cfg, 64, max_in_flight=2, threshold=thr)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep, at = [], 0
    for k, n in enumerate((33, 7, 64, 1, 28)):
        chunk = torch.from_numpy(np.ascontiguousarray(x[:, at:at + n])).cuda()
        keep.append(chunk)
        ffa.push(chunk, n, at, streams[k % 2].cuda_stream)
        at += n
    assert at == x.shape[1] and ffa.pending == 2
    rtol = n_seg * 2.0 ** -52
    for s in range(2):
        cands = ffa.collect()
        rec = ffa.last_records()
        assert (rec["first_row"], rec["n_rows"]) == (s * n_seg, n_seg)
        # in range everywhere, the two columns included
        assert np.all(rec["shift"] < rows[None, :, None, None, None]) and np.all(rec["bin"] < np.arange(8, 11)[None, :, None, None, None])
        flat = {f: rec[f].reshape(rec[f].shape[:3] + (1, n_dm * n_beams))[..., good] for f in ("value", "shift", "bin")}
        assert np.array_equal(flat["value"].view(np.uint32), want[s]["value"].view(np.uint32)), s
        assert np.array_equal(flat["shift"], want[s]["shift"]) and np.array_equal(flat["bin"], want[s]["bin"]), s
        for f in ("sum", "sumsq"):
            assert np.allclose(rec[f].reshape(1, -1)[:, good], want[s][f], rtol=rtol, atol=0.0), (s, f)
        ffa_oracle.assert_candidates_equal(cands, ffa_oracle.select(rec["value"], rec["shift"], rec["bin"], rec["sum"], rec["sumsq"], 1, n_seg, 8,
                                                                     rec["first_row"], 0, thr))
        got = {(int(c["dm"]), int(c["beam"])) for c in cands}
        assert got and not got & set(bad), got
        # ... and they are the columns the oracle finds among the 14 (its statistics are exact, the device's within an ulp or so:
        # the S/N itself is compared above, over the device's records)
        assert got == {divmod(int(good[c[4]]), n_beams) for c in want[s]["cands"]}
    ffa.close()
    bf.close()
