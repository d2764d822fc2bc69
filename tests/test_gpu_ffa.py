"""GPU tests (-m gpu) of the periodicity search (include/dsabf.h: bf_ffa_*; docs/PERIODICITY.md), through the C-ABI.  The reference
is tests/support/ffa_oracle.py: decimation, octaves, the Fast Folding Algorithm's merges, boxcars and records over the WHOLE series.
Records are compared on .view(np.uint32) and their integer fields, statistics to a relative n_seg 2^-52, candidates bit for bit.
The parity inputs are N(0,1) 2^e, e in -20 .. 20; tests/test_ffa_cpu.py asserts for each of them that a left-to-right fold gives
other bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dm_side  # noqa: E402
import ffa_oracle  # noqa: E402
import sps_oracle  # noqa: E402
from ffa_stage import PARITY_CASES, case_cfg, case_input, check_segment, run_stage, same_candidates  # noqa: E402

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


_cfg = case_cfg          # (a name of either table of ffa_stage)


@pytest.mark.sweep_cap(len(PARITY_CASES))
@pytest.mark.parametrize("case", sorted(PARITY_CASES))
def test_records_to_the_bit_whatever_the_pushes(torch, bfmod, case):
    """Every segment's records equal the oracle's, bit for bit, with pushes of 1 / 7 / 33 / 64 times alternating over two streams
    without synchronisation: segments that end in mid-push, decimation groups cut by a push, one push that completes three
    segments; dm_first and a first_t beyond 2^40 label the candidates."""
    n_beams, n_dm, _, _, _, _, _, _, _, sizes, mif = PARITY_CASES[case]
    bf = _bf(bfmod, n_beams)
    log = []
    n = run_stage(torch, bf, case_input(case), _cfg(case), sizes, mif, t_offset=2 ** 40 + 5, dm_first=17, threshold=3.0, log=log)
    assert n >= 1 and sum(len(c) for _, _, c in log) > 0
    for _, _, c in log:
        assert np.all(c["first_row"] >= 2 ** 40) and np.all((c["dm"] >= 17) & (c["dm"] < 17 + n_dm))
    bf.close()


def test_the_cut_into_pushes_does_not_matter(torch, bfmod):
    """The same series under three cuttings -- the case's own, single samples only, and pushes as long as the series allows --
    leaves identical records (and the oracle's)."""
    case = "octaves"
    n_beams, _, n_seg, _, _, tdec, *_ = PARITY_CASES[case]
    x = case_input(case)
    bf = _bf(bfmod, n_beams)
    logs = []
    for sizes, mif in (([1, 7, 33, 64], 2), ([5, 1, 2], 1), ([n_seg * tdec * 2 + 1], 2)):
        log = []
        run_stage(torch, bf, x, _cfg(case), sizes, mif, threshold=3.0, log=log)
        logs.append(log)
    for other in logs[1:]:
        assert len(other) == len(logs[0]) == 2
        for (_, a, ca), (_, b, cb) in zip(logs[0], other):
            for f in ("value", "shift", "bin"):
                assert a[f].tobytes() == b[f].tobytes(), f
            assert same_candidates(ca, cb)
    bf.close()


def test_ties_resolve_to_the_first_row_and_bin(torch, bfmod):
    """Small integers, so every association is exact: this is about WHERE the maximum is reported.  A constant series: shift 0,
    bin 0 at every octave, period and width.  Two equal samples in one row (bins 0 and 3 at p = 8): every profile holds the maximum
    twice, and every row holds it: shift 0, bin 0.  One sample in row 1, bin 1 at p = 8: row 1 is rotated differently in every
    profile, so all M rows tie at different bins -- shift 0 with ITS bin, 1."""
    n_beams, n_dm, n_seg = 68, 2, 64
    cfg = (1, n_seg, 3, 8, 9, 3)            # octaves of 64, 32, 16 samples at p = 8: M = 8, 4, 2
    bf = _bf(bfmod, n_beams)
    const = np.full((n_dm, n_seg, n_beams), 7.0, np.float32)
    pair = np.zeros_like(const)
    pair[:, 0], pair[:, 3] = 5.0, 5.0
    one = np.zeros_like(const)
    one[:, 8 + 1] = 5.0
    for x, want_bin in ((const, 0), (pair, 0), (one, None)):
        log = []
        run_stage(torch, bf, x, cfg, [33, 64], 1, threshold=1e9, log=log)
        rec = log[0][1]
        assert np.all(rec["shift"] == 0)
        if want_bin is not None:
            assert np.all(rec["bin"] == want_bin)
    assert np.all(rec["bin"][0, 0, 0] == 1) and np.all(rec["value"][0, 0, 0] == 5.0)       # (octave 0, p = 8, width 1) of `one`
    bf.close()


def test_back_pressure_and_collect_order(torch, bfmod):
    """max_in_flight + 1 segments: the push that would complete a segment with every result set uncollected is refused with
    BF_ERR_STATE before it queues anything (pushing it again after a collect gives the oracle's records); a push that completes
    nothing is still taken; collect with nothing pending is BF_ERR_STATE; collect with too little room is BF_ERR_INVALID and consumes
    nothing."""
    from dsabeamformer_amd import api

    n_beams, n_dm, n_seg, cfg = 64, 2, 64, (1, 64, 1, 8, 13, 2)
    x = ffa_oracle.parity_input(5, n_dm, 3 * n_seg, n_beams)
    want = ffa_oracle.Search(x, *cfg, threshold=3.0).segments()
    bf = _bf(bfmod, n_beams)
    ffa = api.PeriodicitySearch(bf, n_dm, *cfg, 64, max_in_flight=2, threshold=3.0)
    st = torch.cuda.Stream()
    with pytest.raises(bfmod.DsabfError) as e:
        ffa.collect()
    assert e.value.code == BF_ERR_STATE and str(e.value) == "libdsabf error -4: bf_ffa_collect: no segment is pending"
    pieces = [(0, 64), (64, 60), (124, 4), (128, 10), (138, 54)]
    chunks = [torch.from_numpy(np.ascontiguousarray(x[:, a:a + n])).cuda() for a, n in pieces]
    for i in range(4):
        ffa.push(chunks[i], pieces[i][1], pieces[i][0], st.cuda_stream)         # segments 0 and 1, and ten samples of segment 2
    assert ffa.pending == 2
    with pytest.raises(bfmod.DsabfError) as e:
        ffa.push(chunks[4], 54, 138, st.cuda_stream)
    assert e.value.code == BF_ERR_STATE and ffa.pending == 2
    assert str(e.value) == ("libdsabf error -4: bf_ffa_push: 2 segments are uncollected and this push completes 1 more (max_in_flight 2): "
                            "bf_ffa_collect first")
    out = np.zeros(n_dm * n_beams - 1, api._ffa_candidate_dtype())
    n_out = C.c_size_t()
    assert ffa._lib.bf_ffa_collect(ffa._s, api._ptr(out), out.size, C.byref(n_out)) == BF_ERR_INVALID and ffa.pending == 2
    for s in range(3):
        if s == 1:
            ffa.push(chunks[4], 54, 138, st.cuda_stream)                        # room for one now
        cands = ffa.collect()
        check_segment(ffa.last_records(), cands, want[s], cfg, ("back pressure", s), 0, 3.0)
        assert len(cands) > 0
    assert ffa.pending == 0
    ffa.close()
    bf.close()


# ---- behind the DM stage -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladder(orc):
    """The fine ladder of tests/test_gpu_round5.py (210 x 48 x 256, 40 trials, 45 rows of delay): 165 output times."""
    from test_gpu_round5 import _pulse_delays

    rng = np.random.default_rng(78)
    n_t, n_f, n_b, n_dm, max_rows = 210, 48, 256, 40, 32
    delays = _pulse_delays(n_dm, n_f, 45)
    D = int(delays.max())
    series = (rng.standard_normal((n_t, n_f, n_b)) * np.exp2(rng.integers(-10, 11, (n_t, n_f, n_b)))).astype(np.float32)
    want = orc.dedisperse_dm(series, delays, n_t - D)          # [n_dm][n_t - D][n_b]
    return dict(n_t=n_t, n_f=n_f, n_b=n_b, n_dm=n_dm, max_rows=max_rows, delays=delays, D=D, series=series, want=want)


DM_SIZES = [32, 1, 7, 32, 3, 19, 2, 32, 31, 11]
DM_CFG = (2, 32, 1, 8, 13, 2)          # 64 output times per segment: two whole segments in the ladder's 165


def test_attached_to_a_dm_stage_together_with_a_search(torch, bfmod, ladder):
    """bf_dm_stream_attach_periodicity next to bf_dm_stream_attach_search: the chunks and the search stage's records are what they
    are without the periodicity stage (the oracle's), and the periodicity records equal the oracle's over the chunks -- ring and
    linear buffer, pushes alternating over two streams."""
    from dsabeamformer_amd import api

    fl = ladder
    n_dm, n_b, n_f, D, max_rows, want = fl["n_dm"], fl["n_b"], fl["n_f"], fl["D"], fl["max_rows"], fl["want"]
    tdec, n_seg = DM_CFG[0], DM_CFG[1]
    assert ffa_oracle.association_matters(want[:2, :, :8], *DM_CFG)
    segs = ffa_oracle.Search(want, *DM_CFG, dm_first=3, threshold=3.0).segments()
    assert len(segs) == 2
    bf = _bf(bfmod, n_b, n_f)
    d_series = torch.from_numpy(fl["series"]).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    row_bytes = n_f * n_b * 4
    for ring in (1, 0):
        bf.set_switch("dm_ring", ring)
        dm = api.DmStream(bf, fl["delays"], n_f, max_rows)
        sps = api.SinglePulseSearch(bf, n_dm, 3, max_rows, threshold=1e9)
        ffa = api.PeriodicitySearch(bf, n_dm, *DM_CFG, max_rows, dm_first=3, max_in_flight=2, threshold=3.0)
        dm.attach_search(sps)
        dm.attach_periodicity(ffa)
        sorc = sps_oracle.Search(want, 3, threshold=1e9)
        host = torch.full((n_dm * max_rows * n_b,), float("nan"), dtype=torch.float32).pin_memory()
        parts, pushed, k, emitted = [], 0, 0, 0
        while pushed < fl["n_t"]:
            n = min(DM_SIZES[k % len(DM_SIZES)], fl["n_t"] - pushed)
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
        assert np.array_equal(np.concatenate(parts, axis=1).view(np.uint32), want.view(np.uint32)), ring
        for s in range(2):
            cands = ffa.collect()
            check_segment(ffa.last_records(), cands, segs[s], DM_CFG, ("dm stage", ring, s), 3, 3.0)
            assert len(cands) > 0
        ffa.close()
        sps.close()
        dm.close()
    bf.set_switch("dm_ring", 1)
    bf.close()


def test_dm_stage_back_pressure_detaching_and_the_handle_going_first(torch, bfmod, ladder):
    from dsabeamformer_amd import api

    fl = ladder
    n_dm, n_b, n_f, D, max_rows = fl["n_dm"], fl["n_b"], fl["n_f"], fl["D"], fl["max_rows"]
    bf = _bf(bfmod, n_b, n_f)
    dm = api.DmStream(bf, fl["delays"], n_f, max_rows)
    other = api.PeriodicitySearch(bf, 2, *DM_CFG, max_rows)
    with pytest.raises(bfmod.DsabfError, match="trials") as e:
        dm.attach_periodicity(other)
    assert e.value.code == BF_ERR_INVALID
    short = api.PeriodicitySearch(bf, n_dm, *DM_CFG, max_rows - 1)
    with pytest.raises(bfmod.DsabfError, match="max_t_per_push"):
        dm.attach_periodicity(short)
    ffa = api.PeriodicitySearch(bf, n_dm, *DM_CFG, max_rows, max_in_flight=1, threshold=1e9)   # 64 output times per segment
    dm.attach_periodicity(ffa)
    st = torch.cuda.Stream()
    d_series = torch.from_numpy(fl["series"]).cuda()
    host = torch.zeros((n_dm * max_rows * n_b,), dtype=torch.float32).pin_memory()
    row = n_f * n_b * 4
    pushed, parts = 0, []

    def push(n):
        nonlocal pushed
        first, n_out = dm.push(d_series.data_ptr() + pushed * row, n, host, st.cuda_stream)
        st.synchronize()
        pushed += n
        if n_out:
            parts.append(host[:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b).copy())
        return n_out

    for n in (32, 32, 32, 64 + D - 96):                          # 64 + D rows: 64 output times, segment 0 is complete
        push(n)
    assert pushed - D == 64 and ffa.pending == 1
    push(32)
    push(31)
    assert ffa.pending == 1
    with pytest.raises(bfmod.DsabfError) as e:
        push(1)                                                  # would complete segment 1 with the only set uncollected
    assert e.value.code == BF_ERR_STATE and pushed - D == 127
    assert str(e.value) == ("libdsabf error -4: bf_ffa_push: 1 segments are uncollected and this push completes 1 more (max_in_flight 1): "
                            "bf_ffa_collect first")
    ffa.collect()
    assert ffa.last_records()["first_row"] == 0
    assert push(1) == 1 and ffa.pending == 1
    ffa.collect()
    assert ffa.last_records()["first_row"] == 64
    dm.attach_periodicity(None)                                  # detached in mid-stream: the DM stage goes on alone
    assert push(32) == 32 and push(5) == 5 and ffa.pending == 0
    assert np.array_equal(np.concatenate(parts, axis=1), fl["want"][:, :pushed - D])
    chunk = torch.zeros((n_dm, 4, n_b), dtype=torch.float32).cuda()
    ffa.push(chunk, 4, 0, st.cuda_stream)                        # ... and the stage still takes pushes of its own
    # destroying an attached stage detaches it
    tmp = api.PeriodicitySearch(bf, n_dm, *DM_CFG, max_rows)
    dm.attach_periodicity(tmp)
    tmp.close()
    dm.attach_periodicity(ffa)                                   # (a link to the destroyed stage would be followed here and at the push)
    # the handle destroyed first: the stages answer BF_ERR_STATE and can still be destroyed
    bf.close()
    for call in (lambda: ffa.push(chunk, 4, 4, st.cuda_stream), ffa.collect, lambda: dm.attach_periodicity(None)):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE
    for s in (ffa, other, short, dm):
        s.close()


def test_a_pulse_train_is_the_best_candidate(torch, bfmod):
    """Unit noise in 4 trials x 8 beams and a pulse train of period 83.3 input rows, two rows wide, in beam 5 of trial 2 alone.
    tdec 2, so the period is 41.65 decimated samples: base period 41, M = 16 rows at n_seg = 1000, trial step 1 / 15 sample.
    Orderings only: the best candidate of the segment is in that beam and trial, and its period_rows lies within one trial step
    (tdec / (M - 1) rows) of the truth."""
    n_dm, n_b, tdec, n_seg = 4, 8, 2, 1000
    period, d0, b0 = 83.3, 2, 5
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n_dm, n_seg * tdec, n_b)).astype(np.float32)
    t = np.round(np.arange(0, n_seg * tdec - 2, period) + 7).astype(int)
    x[d0, t, b0] += 6.0
    x[d0, t + 1, b0] += 6.0
    bf = _bf(bfmod, n_b)
    log = []
    run_stage(torch, bf, x, (tdec, n_seg, 2, 32, 64, 3), [64, 33], 1, threshold=5.0, dm_first=10, log=log)
    cands = log[0][2]
    assert len(cands) >= 1
    top = cands[int(np.argmax(cands["snr"]))]
    assert (int(top["dm"]), int(top["beam"])) == (10 + d0, b0)
    M = ffa_oracle.rows_of(n_seg >> int(top["octave"]), int(top["p"]))
    step = tdec * (1 << int(top["octave"])) / (M - 1)
    print("pulse train: period_rows %.3f (truth %.3f), snr %.1f, octave %d, p %d, shift %d, step %.3f" %
          (top["period_rows"], period, top["snr"], top["octave"], top["p"], top["shift"], step))
    assert abs(float(top["period_rows"]) - period) <= step
    bf.close()


def test_refusals_launch_nothing(torch, bfmod):
    from dsabeamformer_amd import api

    bf = _bf(bfmod, 8)
    good = dict(n_dm=2, tdec=2, n_seg=64, n_oct=1, p_lo=8, p_hi=13, n_widths=2, max_t_per_push=16)
    bad = [dict(tdec=0), dict(tdec=257), dict(n_seg=0), dict(n_seg=16385), dict(n_oct=0), dict(n_oct=7), dict(n_oct=2, n_seg=63, p_hi=9),
           dict(p_lo=7), dict(p_hi=513, n_seg=16384), dict(p_hi=8), dict(n_widths=0), dict(n_widths=7), dict(n_widths=4),   # 2^3 > p_lo / 2
           dict(p_hi=34),                                   # 64 / 33 = 1 row
           dict(n_oct=3, p_hi=10),                          # octave 2 has 16 samples: one row of 9
           dict(n_dm=0), dict(n_dm=65536), dict(dm_first=-1), dict(max_t_per_push=0), dict(max_in_flight=0), dict(threshold=float("nan"))]
    for over in bad:
        kw = dict(good, **over)
        with pytest.raises(bfmod.DsabfError) as e:
            api.PeriodicitySearch(bf, **kw)
        assert e.value.code == BF_ERR_INVALID, over
    lib = bf._lib
    out = C.c_void_p()
    assert lib.bf_ffa_create(None, 2, 0, 2, 64, 1, 8, 13, 2, 16, 2, 8.0, C.byref(out)) == BF_ERR_INVALID
    assert lib.bf_ffa_create(bf._h, 2, 0, 2, 64, 1, 8, 13, 2, 16, 2, 8.0, None) == BF_ERR_INVALID
    ffa = api.PeriodicitySearch(bf, **good)
    chunk = torch.zeros((2, 17, 8), dtype=torch.float32).cuda()
    for n_t in (0, -1, 17):
        with pytest.raises(bfmod.DsabfError, match="max_t_per_push") as e:
            ffa.push(chunk, n_t, 0)
        assert e.value.code == BF_ERR_INVALID
    with pytest.raises(bfmod.DsabfError, match="NULL") as e:
        ffa.push(None, 4, 0)
    assert e.value.code == BF_ERR_INVALID
    with pytest.raises(bfmod.DsabfError, match="aligned") as e:
        ffa.push(chunk.data_ptr() + 4, 4, 0)
    assert e.value.code == BF_ERR_INVALID
    n_out = C.c_size_t()
    assert lib.bf_ffa_collect(ffa._s, None, 16, C.byref(n_out)) == BF_ERR_INVALID
    assert lib.bf_ffa_push(None, C.c_void_p(chunk.data_ptr()), 4, 0, None) == BF_ERR_INVALID
    assert lib.bf_ffa_pending(None) == BF_ERR_INVALID and lib.bf_ffa_last_records(ffa._s, None, None, None, None) == BF_ERR_STATE
    assert ffa.pending == 0
    ffa.push(chunk, 16, 0)                                  # ... and the stage is as it was: a good push is taken
    torch.cuda.synchronize()
    ffa.close()
    bf.close()


def test_beam_cli_writes_the_candidates_the_oracle_finds_in_its_dm_file(tmp_path):
    """`beam -j 33 -M 250 -N 8 -W dm.bin --ffa 8:13 --ffa-seg 64 --ffa-dec 2 --ffa-oct 2 --ffa-widths 2 --ffa-snr 3 --ffa-out ffa.txt` in a
    child process: 25 burn-in reads + 8 analysed blocks.  The candidates are recomputed from dm.bin by the oracle -- segments of 128
    output times from time 0 -- and compared with the file: integers, period and value exactly; the S/N to 1e-9 (the oracle sums
    the statistics exactly, the device to an ulp or so), with no S/N of the run within 1e-7 of the threshold."""
    from dsabeamformer_amd import build, host

    dm_file, ffa_file = tmp_path / "dm.bin", tmp_path / "ffa.txt"
    thr, cfg = 3.0, (2, 64, 2, 8, 13, 2)
    r = subprocess.run([build.BEAM, "-j", "33", "-M", "250", "-N", "8", "-W", str(dm_file), "--ffa", "8:13", "--ffa-seg", "64", "--ffa-dec", "2", "--ffa-oct", "2",
                        "--ffa-widths", "2", "--ffa-snr", str(thr), "--ffa-out", str(ffa_file)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hdr, data, chunks = host.read_dm_file(str(dm_file))
    assert data.shape[0] == 8 and sum(n for _, n in chunks) == data.shape[1]
    # (the comparison itself: tests/support/dm_side.py, shared with the trial-split runs of tests/test_gpu_trial_split.py)
    head, want, n_every = dm_side.check_ffa(ffa_file, r.stdout, data, cfg, thr)
    n_segs = data.shape[1] // 128
    print("periodicity candidates recomputed from dm.bin: %d of %d series x %d segments" % (len(want), data.shape[0] * data.shape[2], n_segs))
    assert n_segs >= 2 and 1 <= len(want) < n_every
    assert head["p_lo"] == "8" and head["p_hi"] == "13" and head["n_seg"] == "64" and head["tdec"] == "2" and head["n_oct"] == "2" and head["n_widths"] == "2"
