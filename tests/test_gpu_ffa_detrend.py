"""GPU tests (-m gpu) of the periodicity search's running-median detrend (include/dsabf.h: bf_ffa_set_detrend; docs/PERIODICITY.md
section 1a), through the C-ABI.  The reference is tests/support/ffa_detrend_oracle.py in front of tests/support/ffa_oracle.py.
Records are compared on .view(np.uint32) and their integer fields, statistics to a relative n_seg 2^-52, candidates bit for bit
against the oracle's selection over the device's records.  tests/test_ffa_detrend_cpu.py asserts for every input here which of
the oracle's mutants (upper median, constant trend, one rounding) it can tell from the contract."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dm_side  # noqa: E402
import ffa_detrend_oracle as det  # noqa: E402
import ffa_oracle  # noqa: E402
import sps_oracle  # noqa: E402
from ffa_detrend_stage import (CASES, RED_BEAM, RED_CFG, RED_DETREND, RED_PERIOD, best_per_beam, case_cfg, case_input, red_noise_input,  # noqa: E402
                               run_stage)
from ffa_stage import check_segment, same_candidates  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _bf(bfmod, n_beams, n_freq=8):
    return bfmod.Beamformer(bfmod.debug_config(n_beams=n_beams, n_freq=n_freq))


@pytest.mark.sweep_cap(len(CASES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_detrended_records_to_the_bit(torch, bfmod, case):
    """One ffa_detrend_stage.CASES entry through the stage in its own pushes, alternating over two streams without synchronisation:
    every segment's records equal the detrend oracle's bit for bit, and every case yields candidates."""
    n_beams, n_dm, _, _, _, _, _, _, _, sizes, mif, _, _ = CASES[case]
    cfg, detrend = case_cfg(case)
    bf = _bf(bfmod, n_beams)
    log = []
    n = run_stage(torch, bf, case_input(case), cfg, detrend, sizes, mif, t_offset=2 ** 40 + 5, dm_first=17, threshold=3.0, log=log)
    assert n >= 1 and sum(len(c) for _, _, c in log) > 0
    bf.close()


def test_ties_both_zeros_and_a_constant_series(torch, bfmod):
    """Samples drawn from {-1, -0.0, +0.0, 1} with blk 1 (the means ARE the samples): every window is full of equal keys and of both
    zeros, so the rank of an element rests on the index tie-break and -0 < +0 decides which zero is selected; with blk 2 the means
    are 0, +-0.5, +-1 and -0 again.  A constant series: y' is exactly zero, so sum = sumsq = 0, sigma = 0 and no candidate."""
    n_beams, n_dm, n_seg = 8, 2, 64
    cfg = (1, n_seg, 1, 8, 11, 2)
    rng = np.random.default_rng(5)
    x = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=(n_dm, 2 * n_seg + 3, n_beams))
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    bf = _bf(bfmod, n_beams)
    for detrend in ((1, 9), (1, 129), (2, 5)):
        # (a window of 33 .. 64 of these four values has the same lower and upper median: only the short windows tell them apart)
        assert any(w.any() for w, _ in det.mutant_changes(x, 1, n_seg, *detrend, "upper")) == (detrend[1] < 129)
        run_stage(torch, bf, x, cfg, detrend, [33, 64], 2, threshold=-1e300)
    const = np.full((n_dm, n_seg + 5, n_beams), 7.25, np.float32)
    for detrend in ((1, 3), (8, 5), (64, 1)):
        log = []
        run_stage(torch, bf, const, cfg, detrend, [33, 64], 1, threshold=-1e300, log=log)
        rec, cands = log[0][1], log[0][2]
        assert not rec["sum"].any() and not rec["sumsq"].any() and not rec["value"].any() and len(cands) == 0
        assert not rec["shift"].any() and not rec["bin"].any()
    bf.close()


def test_the_cut_into_pushes_does_not_matter(torch, bfmod):
    """One series under three cuttings -- the case's own, short pushes only, and one push for everything -- leaves identical records."""
    case = "beams60"
    n_beams, _, n_seg, _, _, tdec, *_ = CASES[case]
    cfg, detrend = case_cfg(case)
    x = case_input(case)
    want = det.Search(x, *cfg, *detrend, threshold=3.0).segments()
    bf = _bf(bfmod, n_beams)
    logs = []
    for sizes, mif in (([1, 7, 33, 64], 2), ([5, 1, 2], 1), ([n_seg * tdec * 2 + 1], 2)):
        log = []
        run_stage(torch, bf, x, cfg, detrend, sizes, mif, threshold=3.0, log=log, want=want)
        logs.append(log)
    for other in logs[1:]:
        assert len(other) == len(logs[0]) == 2
        for (_, a, ca), (_, b, cb) in zip(logs[0], other):
            for f in ("value", "shift", "bin"):
                assert a[f].tobytes() == b[f].tobytes(), f
            assert same_candidates(ca, cb)
    bf.close()


def test_detrend_off_is_the_stage_as_it_was(torch, bfmod):
    """bf_ffa_set_detrend(s, 0, 0), detrend=None and never calling it: all bit-equal to ffa_oracle.Search, the oracle that knows no
    detrend."""
    case = "beams4"
    n_beams, _, _, _, _, _, _, _, _, sizes, mif, _, _ = CASES[case]
    cfg, _ = case_cfg(case)
    x = case_input(case)
    want = ffa_oracle.Search(x, *cfg, threshold=3.0).segments()
    on = det.Search(x, *cfg, *case_cfg(case)[1], threshold=3.0).segments()
    assert not np.array_equal(want[0]["value"].view(np.uint32), on[0]["value"].view(np.uint32))
    bf = _bf(bfmod, n_beams)
    for how in ("ctor", "call", "never"):
        assert run_stage(torch, bf, x, cfg, None, sizes, mif, threshold=3.0, want=want, set_detrend=how) == 2
    bf.close()


def test_set_detrend_refusals_with_a_stage(torch, bfmod):
    """n_seg % blk != 0 is BF_ERR_INVALID and leaves the stage as it was; after the first push bf_ffa_set_detrend is BF_ERR_STATE
    and the stage runs on as it was configured (the oracle's records for (4, 5)); an orphaned stage answers BF_ERR_STATE."""
    from dsabeamformer_amd import api

    case = "beams4"
    n_beams, n_dm, n_seg, *_ = CASES[case]
    cfg, detrend = case_cfg(case)
    x = case_input(case)
    want = det.Search(x, *cfg, *detrend, threshold=3.0).segments()
    bf = _bf(bfmod, n_beams)
    with pytest.raises(bfmod.DsabfError, match="no multiple of blk") as e:
        api.PeriodicitySearch(bf, n_dm, *cfg, 64, detrend=(64, 3))           # n_seg 96
    assert e.value.code == BF_ERR_INVALID
    ffa = api.PeriodicitySearch(bf, n_dm, *cfg, 64, max_in_flight=2, threshold=3.0, detrend=(8, 3))
    for blk, win, msg in ((64, 3, "no multiple of blk"), (3, 3, "power of two"), (8, 4, "odd")):
        with pytest.raises(bfmod.DsabfError, match=msg) as e:
            ffa.set_detrend(blk, win)
        assert e.value.code == BF_ERR_INVALID and ffa.detrend == (8, 3)
    ffa.set_detrend(0, 0)
    assert ffa.detrend is None
    ffa.set_detrend(*detrend)
    st = torch.cuda.Stream()
    chunks = [torch.from_numpy(np.ascontiguousarray(x[:, a:a + 48])).cuda() for a in range(0, 192, 48)]
    ffa.push(chunks[0], 48, 0, st.cuda_stream)
    for blk, win in ((0, 0), (8, 3), detrend):
        with pytest.raises(bfmod.DsabfError, match="before the first") as e:
            ffa.set_detrend(blk, win)
        assert e.value.code == BF_ERR_STATE and ffa.detrend == detrend
    for i in range(1, 4):
        ffa.push(chunks[i], 48, 48 * i, st.cuda_stream)
    for s in range(2):
        cands = ffa.collect()
        check_segment(ffa.last_records(), cands, want[s], cfg, ("after the refusal", s), 0, 3.0)
    other = api.PeriodicitySearch(bf, n_dm, *cfg, 64)
    bf.close()                                                               # the handle first: the stage is orphaned
    with pytest.raises(bfmod.DsabfError) as e:
        other.set_detrend(4, 5)
    assert e.value.code == BF_ERR_STATE
    other.close()
    ffa.close()


def test_a_non_finite_column_stays_in_range_and_alone(torch, bfmod):
    """8 beams x 2 trials, n_seg 64, blk 4, win 5.  Column (trial 0, beam 3) is NaN throughout, (trial 1, beam 6) is -inf throughout
    and (trial 1, beam 1) has one +inf sample: their records and statistics are unspecified, shift < M and bin < p hold all the
    same.  The other 13 columns are what the oracle gives for them alone, bit for bit."""
    from dsabeamformer_amd import api

    n_beams, n_dm, n_seg, thr = 8, 2, 64, 3.0
    cfg, detrend = (1, n_seg, 1, 8, 11, 3), (4, 5)
    x = ffa_oracle.parity_input(4321, n_dm, 2 * n_seg + 5, n_beams)
    bad = [(0, 3), (1, 6), (1, 1)]
    x[0, :, 3] = np.nan
    x[1, :, 6] = -np.inf
    x[1, 40, 1] = x[1, 64 + 9, 1] = np.inf
    good = np.array([d * n_beams + b for d in range(n_dm) for b in range(n_beams) if (d, b) not in bad])
    alone = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(1, x.shape[1], n_dm * n_beams)[:, :, good])      # [1][T][13]
    want = det.Search(alone, *cfg, *detrend, threshold=thr).segments()
    assert len(want) == 2 and all(len(w["cands"]) > 0 for w in want)
    rows = np.array([ffa_oracle.rows_of(n_seg, p) for p in range(8, 11)])

    bf = _bf(bfmod, n_beams)
    ffa = api.PeriodicitySearch(bf, n_dm, *cfg, 64, max_in_flight=2, threshold=thr, detrend=detrend)
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
        ffa.collect()
        rec = ffa.last_records()
        assert (rec["first_row"], rec["n_rows"]) == (s * n_seg, n_seg)
        assert np.all(rec["shift"] < rows[None, :, None, None, None]) and np.all(rec["bin"] < np.arange(8, 11)[None, :, None, None, None])
        flat = {f: rec[f].reshape(rec[f].shape[:3] + (1, n_dm * n_beams))[..., good] for f in ("value", "shift", "bin")}
        assert np.array_equal(flat["value"].view(np.uint32), want[s]["value"].view(np.uint32)), s
        assert np.array_equal(flat["shift"], want[s]["shift"]) and np.array_equal(flat["bin"], want[s]["bin"]), s
        for f in ("sum", "sumsq"):
            assert np.allclose(rec[f].reshape(1, -1)[:, good], want[s][f], rtol=rtol, atol=0.0), (s, f)
    ffa.close()
    bf.close()


# ---- behind the DM stage -------------------------------------------------------------------------------------------------------
DM_SIZES = [32, 1, 7, 32, 3, 19, 2, 32, 31, 11]
DM_CFG, DM_DETREND = (2, 32, 1, 8, 13, 2), (4, 3)          # 64 output times per segment: two whole segments in the ladder's 165


def test_attached_to_a_dm_stage_together_with_a_search(torch, bfmod, orc):
    """bf_dm_stream_attach_periodicity with the detrend on, next to bf_dm_stream_attach_search, on the fine ladder of
    tests/test_gpu_ffa.py (210 x 48 x 256, 40 trials): the chunks and the search stage's records are the oracle's, unchanged, and
    the periodicity records are the detrend oracle's over the chunks."""
    from dsabeamformer_amd import api
    from test_gpu_round5 import _pulse_delays

    rng = np.random.default_rng(78)
    n_t, n_f, n_b, n_dm, max_rows = 210, 48, 256, 40, 32
    delays = _pulse_delays(n_dm, n_f, 45)
    D = int(delays.max())
    series = (rng.standard_normal((n_t, n_f, n_b)) * np.exp2(rng.integers(-10, 11, (n_t, n_f, n_b)))).astype(np.float32)
    want = orc.dedisperse_dm(series, delays, n_t - D)          # [n_dm][n_t - D][n_b]
    tdec, n_seg = DM_CFG[0], DM_CFG[1]
    segs = det.Search(want, *DM_CFG, *DM_DETREND, dm_first=3, threshold=3.0).segments()
    plain = ffa_oracle.Search(want, *DM_CFG, dm_first=3, threshold=3.0).segments()
    assert len(segs) == 2 and not np.array_equal(segs[0]["value"].view(np.uint32), plain[0]["value"].view(np.uint32))
    bf = _bf(bfmod, n_b, n_f)
    d_series = torch.from_numpy(series).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    row_bytes = n_f * n_b * 4
    dm = api.DmStream(bf, delays, n_f, max_rows)
    sps = api.SinglePulseSearch(bf, n_dm, 3, max_rows, threshold=1e9)
    ffa = api.PeriodicitySearch(bf, n_dm, *DM_CFG, max_rows, dm_first=3, max_in_flight=2, threshold=3.0, detrend=DM_DETREND)
    dm.attach_search(sps)
    dm.attach_periodicity(ffa)
    sorc = sps_oracle.Search(want, 3, threshold=1e9)
    host = torch.full((n_dm * max_rows * n_b,), float("nan"), dtype=torch.float32).pin_memory()
    parts, pushed, k, emitted = [], 0, 0, 0
    while pushed < n_t:
        n = min(DM_SIZES[k % len(DM_SIZES)], n_t - pushed)
        st = streams[k % 2]
        first_t, n_out = dm.push(d_series.data_ptr() + pushed * row_bytes, n, host, st.cuda_stream)
        pushed += n
        k += 1
        if not n_out:
            continue
        emitted += n_out
        assert first_t == emitted - n_out and ffa.pending == min(emitted // (n_seg * tdec), 2)
        st.synchronize()
        parts.append(host[:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b).copy())
        w = sorc.push(n_out)
        sps.collect()
        rec = sps.last_records()
        assert np.array_equal(rec["value"].view(np.uint32), w["value"].view(np.uint32)) and np.array_equal(rec["t_end"], w["t_end"])
    assert np.array_equal(np.concatenate(parts, axis=1).view(np.uint32), want.view(np.uint32))
    for s in range(2):
        cands = ffa.collect()
        check_segment(ffa.last_records(), cands, segs[s], DM_CFG, ("dm stage", s), 3, 3.0)
        assert len(cands) > 0
    ffa.close()
    sps.close()
    dm.close()
    bf.close()


def test_the_detrend_recovers_a_pulse_train_from_red_noise(torch, bfmod):
    """The red-noise case of tests/test_ffa_detrend_cpu.py on the device: with the detrend (8, 9) the injected train is the best
    candidate of its beam at S/N >= 8, within 1 / (M - 1) of its period, and the only candidate; with the detrend off the same
    input gives no candidate at threshold 8."""
    x = red_noise_input()
    bf = _bf(bfmod, 4)
    log = []
    run_stage(torch, bf, x, RED_CFG, RED_DETREND, [64, 33], 1, threshold=8.0, log=log)
    cands = log[0][2]
    snr, period = best_per_beam(cands)[RED_BEAM]
    M = ffa_oracle.rows_of(RED_CFG[1], int(period))
    print("red noise, detrended: S/N %.2f at period %.3f (injected %.3f, step %.4f)" % (snr, period, RED_PERIOD, 1.0 / (M - 1)))
    assert snr >= 8.0 and abs(period - RED_PERIOD) <= 1.0 / (M - 1) and set(cands["beam"].tolist()) == {RED_BEAM}
    log = []
    run_stage(torch, bf, x, RED_CFG, None, [64, 33], 1, threshold=8.0, log=log)
    assert len(log[0][2]) == 0
    bf.close()


def test_beam_cli_with_ffa_detrend_writes_what_the_oracle_finds_in_its_dm_file(tmp_path):
    """`beam -j 33 -M 250 -N 8 -W dm.bin --ffa 8:13 --ffa-seg 64 --ffa-dec 2 --ffa-oct 2 --ffa-widths 2 --ffa-snr 3 --ffa-detrend 8:5
    --ffa-out ffa.txt` in a child process: the header carries detrend=8:5, and the lines are the detrend oracle's candidates over
    the chunks written to dm.bin (integers, period and value exactly; the S/N to 1e-9, with no S/N of the run within 1e-7 of the
    threshold)."""
    from dsabeamformer_amd import build, host

    dm_file, ffa_file = tmp_path / "dm.bin", tmp_path / "ffa.txt"
    thr, cfg = 3.0, (2, 64, 2, 8, 13, 2)
    r = subprocess.run([build.BEAM, "-j", "33", "-M", "250", "-N", "8", "-W", str(dm_file), "--ffa", "8:13", "--ffa-seg", "64", "--ffa-dec", "2", "--ffa-oct", "2",
                        "--ffa-widths", "2", "--ffa-snr", str(thr), "--ffa-detrend", "8:5", "--ffa-out", str(ffa_file)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hdr, data, chunks = host.read_dm_file(str(dm_file))
    n_segs = data.shape[1] // 128
    assert data.shape[0] == 8 and n_segs >= 2
    # (the comparison itself: tests/support/dm_side.py, shared with the trial-split runs of tests/test_gpu_trial_split.py)
    head, want, n_every = dm_side.check_ffa(ffa_file, r.stdout, data, cfg, thr, detrend=(8, 5))
    assert 1 <= len(want) < n_every
    assert head["detrend"] == "8:5" and head["n_seg"] == "64" and head["tdec"] == "2"
    # out of range: refused by bf_ffa_set_detrend, with its message
    r = subprocess.run([build.BEAM, "-j", "33", "-M", "250", "-N", "8", "--ffa", "8:13", "--ffa-seg", "64", "--ffa-detrend", "128:5"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "no multiple of blk" in r.stdout + r.stderr
