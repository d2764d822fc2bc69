"""What the DM-side files of a `beam` run must hold, stage by stage, as functions of (files, dm_first, dm_count, delays): each check
reads the files a run wrote and holds them to the stage's own oracle.  A single-process run is the case dm_first = 0 with the whole
ladder; the rank of a trial-split run (`-R world -r rank -X`) passes its share, and the trials in its files are numbered over the whole
ladder.  The stages' end-to-end tests (tests/test_gpu_sps.py, _stamps, _ffa, _ffa_detrend, _psr, _cond, _inj) and
tests/test_gpu_trial_split.py call the same functions.  Importing this needs neither a GPU nor the library; the functions that parse
the library's files import dsabeamformer_amd.host when called."""
import os
import subprocess

import numpy as np

import cond_oracle
import evt_oracle as eo
import ffa_detrend_oracle
import ffa_oracle
import inj_oracle
import psr_oracle
import sps_oracle
import stamp_oracle as so

SUPPORT = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(SUPPORT, "libfakerccl.so")
STAMP_BINS, STAMP_CAP = 64, 16        # the driver's --stamps defaults: bins per stamp, stamps per deliver
BORDERLINE = 1e-7                     # no S/N of a run this close (relative) to a threshold: 100 x the tolerance the S/N is held to


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fake_rccl():
    """tests/support/libfakerccl.so, the loopback stand-in for RCCL (DSABF_RCCL_LIB), built if it is missing or older than its source."""
    from dsabeamformer_amd import build

    src = os.path.join(SUPPORT, "fake_rccl.cpp")
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(src):
        obj = os.path.join(SUPPORT, "fake_rccl.o")
        subprocess.check_call([build.HIPCC, "-O2", "-std=c++17", "-fPIC", "-c", src, "-o", obj])
        cxx = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
        subprocess.check_call([cxx if os.path.exists(cxx) else "g++", "-shared", "-fPIC", "-o", FAKE, obj, "-lpthread", "-lrt"])
    return FAKE


def beam_ladder(dm_max, n_cap, n_freq=256, tsamp_ms=0.131):
    """What `beam -M dm_max -N n_cap -T tsamp_ms` computes (csrc/beam_main.cpp): the notebook's ladder, evenly picked, and its delays at
    the band's channels, referred to channel 0.  Returns (dms [n_dm], freq float32 [n_freq], delays int32 [n_dm][n_freq])."""
    from dsabeamformer_amd import host

    dms = host.dm_trials(dm_max=dm_max)
    if len(dms) > n_cap:
        dms = np.array([dms[int(i * (len(dms) - 1) / (n_cap - 1 if n_cap > 1 else 1))] for i in range(n_cap)])
    freq = np.array([host.channel_frequency(0, c) for c in range(n_freq)], np.float32)
    return dms, freq, host.dm_delays(dms, freq, float(freq[0]), tsamp_ms)


def read_rows(det_file):
    """The rows of a -w file in time order: float32 [T][f][b]."""
    from dsabeamformer_amd import host

    _, det = host.read_detected_file(str(det_file))                 # [gemm][output][f][b]
    return np.ascontiguousarray(det.reshape(-1, det.shape[2], det.shape[3]))


def conditioned_rows(raw, rows_per_push, window, zero_dm=False, auto_threshold=0.0, mask=None):
    """cond_oracle over the rows push by push, as the run conditions them.  Returns (rows, the conditioner after the last push)."""
    c = cond_oracle.Conditioner(raw.shape[1], raw.shape[2], window, zero_dm, auto_threshold, mask)
    return np.concatenate([c.push(raw[at:at + rows_per_push]) for at in range(0, raw.shape[0], rows_per_push)]), c


def injected_rows(raw, rows_per_push, freq, tsamp_ms, bursts=(), trains=()):
    """inj_oracle over the rows with the tables `beam --inject T0:DM:BEAM:FLUENCE:SIGMA:W` and `--inject-train F0:DM:BEAM:AMP[:DUTY:BINS]`
    make (csrc/beam_main.cpp: wire_injector): bursts (t0, dm, beam, fluence, sigma, W), trains (f0, dm, beam, amp, duty, n_bins)."""
    from dsabeamformer_amd import api, host

    n_f, n_b = raw.shape[1], raw.shape[2]
    delay_of = lambda dm: host.dm_delays(np.array([float(dm)]), freq, float(freq[0]), tsamp_ms)[0]  # noqa: E731

    def one_beam(beam):
        resp = np.zeros(n_b, np.float32)
        resp[beam] = 1.0
        return resp

    b_tab = [(t0, delay_of(dm), api.Injector.burst_profile(n_f, W, (W - 1) / 2.0, sigma, fluence), one_beam(beam)) for t0, dm, beam, fluence, sigma, W in bursts]
    t_tab = []
    for f0, dm, beam, amp, duty, n_bins in trains:
        m = api.PulsarFolder.model_from_spin(f0, row_seconds=tsamp_ms * 1e-3)
        prof = np.zeros((n_f, n_bins), np.float32)
        prof[:, :max(1, round(duty * n_bins))] = amp
        t_tab.append(((m.phase0, m.dphase, m.ddphase, m.epoch_row), delay_of(dm), prof, one_beam(beam), 0, None))
    return inj_oracle.inject(raw, b_tab, t_tab, cuts=[rows_per_push] * (raw.shape[0] // rows_per_push))


def closing_lines(stdout):
    """What run_observation prints behind its closing report ("Synchronized" ends that), without the driver's own "Wrote ..." lines."""
    lines = stdout.splitlines()
    return [l for l in lines[lines.index("Synchronized") + 1:] if not l.startswith("Wrote ")]


def sorted_records(path, read, key):
    """(header, the records of a stamp or voltage-cut file as sorted (key fields, data bytes)): a retried cut lands a deliver later, and
    when a deliver comes depends on the clock -- two runs hold the same records in any order."""
    hdr, recs = read(path)
    return hdr, sorted((tuple(r[k] for k in key), r["data"].tobytes()) for r in recs)


# ---- the DM file ----------------------------------------------------------------------------------------------------------------------
def check_dm_file(dm_file, rows, delays, dm_first=0, dm_count=None):
    """The -W file of the share [dm_first, dm_first + dm_count) of the ladder `delays` ([n_dm][f], the whole ladder) is
    orc.dedisperse_dm of `rows` (what the DM stage dedispersed: [T][f][b]) over the share's delays, bit for bit, and its header says
    which share it is.  Returns (header, data [dm_count][T - D][b], chunks)."""
    import oracle as orc

    from dsabeamformer_amd import host

    dm_count = len(delays) - dm_first if dm_count is None else dm_count
    mine = np.ascontiguousarray(delays[dm_first:dm_first + dm_count])
    D = int(mine.max())
    hdr, data, chunks = host.read_dm_file(str(dm_file))
    assert (int(hdr["N_DM"]), int(hdr["DM_FIRST_TRIAL"]), int(hdr["MAX_DELAY"])) == (dm_count, dm_first, D), hdr
    assert int(hdr["N_FREQUENCIES"]) == rows.shape[1] and sum(n for _, n in chunks) == data.shape[1] == rows.shape[0] - D
    want = orc.dedisperse_dm(rows, mine, rows.shape[0] - D)
    assert data.shape == want.shape and np.array_equal(bits(data), bits(want)), (dm_first, dm_count)
    return hdr, data, chunks


# ---- the single-pulse search ----------------------------------------------------------------------------------------------------------
def read_candidates(cand_file):
    """A -C file as records of api._candidate_dtype()."""
    from dsabeamformer_amd import api

    lines = open(str(cand_file)).read().splitlines()
    assert lines[0].startswith("#")
    tab = [l.split() for l in lines[1:]]
    got = np.zeros(len(tab), api._candidate_dtype())
    for i, f in enumerate(("t_start", "dm", "beam", "width", "snr", "peak")):
        got[f] = [row[i] for row in tab]
    return got


def oracle_candidates(data, chunks, n_widths, threshold, dm_first=0):
    """sps_oracle over the chunks of a DM file (the driver's baseline window of 8 chunks and 64-sample minimum are the oracle's
    defaults), with the guard that no S/N of the run lies on the threshold."""
    every = sps_oracle.Search(data, n_widths, dm_first=dm_first, threshold=-np.inf)
    snr = np.array([c[5] for _, n in chunks for c in every.push(n)["cands"]])
    assert np.all(np.abs(snr - threshold) > BORDERLINE * threshold)
    search = sps_oracle.Search(data, n_widths, dm_first=dm_first, threshold=threshold)
    return [c for _, n in chunks for c in search.push(n)["cands"]]


def check_candidates(cand_file, stdout, data, chunks, n_widths, threshold, dm_first=0, printed=None):
    """The -C file is what sps_oracle finds in the chunks of the run's own DM file (S/N to 1e-9, the rest exactly), every trial numbered
    over the whole ladder, and the closing lines carry the count and the file's name as the run was given it (`printed`, where that is
    not cand_file).  Returns (the file's records, the oracle's candidates)."""
    want = oracle_candidates(data, chunks, n_widths, threshold, dm_first)
    assert ("Single-pulse search: boxcar widths 1 .. %d, %d candidates" % (1 << (n_widths - 1), len(want))) in stdout, stdout[-2000:]
    assert ("Wrote %d candidates to %s" % (len(want), printed or cand_file)) in stdout
    got = read_candidates(cand_file)
    assert len(got) == len(want)
    sps_oracle.assert_candidates_equal(got, want, rtol=1e-9)
    assert np.all((got["dm"] >= dm_first) & (got["dm"] < dm_first + data.shape[0]))
    return got, want


# ---- events and stamps ----------------------------------------------------------------------------------------------------------------
def by_best_key(events):
    return sorted(events, key=lambda e: (int(e["best"]["t_start"]), int(e["best"]["dm"]), int(e["best"]["beam"])))


def check_events(ev_file, cand_file, **opts):
    """The --events file is evt_oracle.events over the run's own -C file (snr to 1e-9, as the candidates' own test).  Returns (the
    candidates as the event builder takes them, the oracle's events)."""
    from dsabeamformer_amd import host

    tab = np.loadtxt(str(cand_file), ndmin=2)
    cands = eo.candidates([(int(v[0]), int(v[1]), int(v[2]), int(v[3]), v[4], v[5]) for v in tab])
    want = eo.events(cands, **opts)
    eo.assert_events_equal(by_best_key(host.read_event_file(str(ev_file))), want, snr_rtol=1e-9)
    return cands, want


def stamp_request(e):
    """(t0, dm, beam, tbin, width) of the stamp the driver asks for around the event e: 64 bins centred on its best member."""
    b = e["best"]
    tbin = max(1, int(b["width"]) // 2)
    return max(0, int(b["t_start"]) + int(b["width"]) // 2 - STAMP_BINS * tbin // 2), int(b["dm"]), int(b["beam"]), tbin, int(b["width"])


def picked_events(cands, chunks, n_events, **opts):
    """The selection rule of the stamps over the events of every deliver: api.EventBuilder replayed over the chunks of the DM file (a
    candidate is reported with the END of its boxcar), the unflagged events of each feed by S/N descending, 16 at most.  Returns (the
    events picked, the number dropped)."""
    from dsabeamformer_amd import api

    t_end = cands["t_start"].astype(np.int64) + cands["width"] - 1
    picked, dropped, total = [], 0, 0
    with api.EventBuilder(**opts) as eb:
        feeds = [eb.feed(cands[(t_end >= first_t) & (t_end < first_t + n_t)], first_t + n_t) for first_t, n_t in chunks] + [eb.flush()]
    for ev in feeds:
        total += len(ev)
        pick = [e for e in ev if not e["flags"]]
        pick = sorted(pick, key=lambda e: -float(e["best"]["snr"]))              # (stable: ties stay in event order)
        dropped += max(0, len(pick) - STAMP_CAP)
        picked += pick[:STAMP_CAP]
    assert total == n_events
    return picked, dropped


def check_stamps(st_file, stdout, cands, chunks, n_events, rows, delays, **opts):
    """The --stamps file holds the set the selection rule picks from the events of every deliver; the closing line reports it, with
    stamps_dropped, stamps_missed 0 and the count of windows that pass the last row of the run (arithmetic on the request, nothing the
    run reports); every stamp is bit-equal to stamp_oracle.stamp over `rows` (what the DM stage's ring held) at the delays of the WHOLE
    ladder, with the global trial the record carries.  Returns the stamps."""
    from dsabeamformer_amd import host

    picked, dropped = picked_events(cands, chunks, n_events, **opts)
    past = lambda e: stamp_request(e)[0] + so.span(delays, stamp_request(e)[1], STAMP_BINS, stamp_request(e)[3]) > rows.shape[0]  # noqa: E731
    beyond = [e for e in picked if past(e)]
    picked = [e for e in picked if not past(e)]
    assert ("Events: %d events, stamps %d, stamps_dropped %d, stamps_missed 0, beyond the end of the run %d" % (n_events, len(picked), dropped, len(beyond))) \
        in stdout, stdout[-1500:]
    hdr, stamps = host.read_stamp_file(str(st_file))
    assert len(stamps) == len(picked) and (hdr["NFREQ_OUT"], hdr["NBINS"], hdr["FBIN"]) == (str(rows.shape[1]), str(STAMP_BINS), "1")
    key = lambda t0, dm, beam, tbin, width: (int(t0), int(dm), int(beam), int(tbin), int(width))   # noqa: E731
    assert sorted(key(s["t0"], s["dm"], s["beam"], s["tbin"], s["width"]) for s in stamps) == sorted(key(*stamp_request(e)) for e in picked)
    for s in stamps:
        want = so.stamp(rows, delays, s["t0"], s["dm"], s["beam"], STAMP_BINS, s["tbin"], 1)
        assert np.array_equal(bits(s["data"]), bits(want)), key(*[s[k] for k in ("t0", "dm", "beam", "tbin", "width")])
    return stamps


# ---- the periodicity search -----------------------------------------------------------------------------------------------------------
def check_ffa(ffa_file, stdout, data, cfg, threshold, dm_first=0, detrend=None):
    """The --ffa-out file is what the ffa oracle -- the detrend oracle with detrend = (blk, win) -- finds in the run's own DM file:
    integers, period and value exactly; the S/N to 1e-9 (the oracle sums the statistics exactly, the device to an ulp or so), with no
    S/N of the run within 1e-7 of the threshold.  cfg = (tdec, n_seg, n_oct, p_lo, p_hi, n_widths).  Returns (header, the oracle's
    candidates, the number of segments)."""
    tdec, n_seg = cfg[0], cfg[1]
    n_segs = data.shape[1] // (tdec * n_seg)
    assert n_segs >= 2
    if detrend:
        search = ffa_detrend_oracle.Search(data, *cfg, detrend[0], detrend[1], dm_first=dm_first, threshold=-np.inf)
    else:
        search = ffa_oracle.Search(data, *cfg, dm_first=dm_first, threshold=-np.inf)
    every = [c for s in search.segments() for c in s["cands"]]
    snr = np.array([c[10] for c in every])
    assert np.all(np.abs(snr - threshold) > BORDERLINE * threshold)
    want = [c for c in every if c[10] >= threshold]
    assert ("%d segments of %d samples, %d candidates" % (n_segs, n_seg, len(want))) in stdout, stdout[-2000:]
    assert ("Wrote %d periodicity candidates" % len(want)) in stdout
    head, got = ffa_oracle.read_candidates(str(ffa_file))
    assert (head["tdec"], head["n_seg"], head["n_oct"], head["p_lo"], head["p_hi"], head["n_widths"]) == tuple(str(cfg[i]) for i in (0, 1, 2, 3, 4, 5))
    assert not detrend or head["detrend"] == "%d:%d" % tuple(detrend)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:10] == w[:10] and g[11] == w[11], (g, w)
        assert abs(g[10] - w[10]) <= 1e-9 * abs(w[10])
    return head, want, len(every)


# ---- the folder -----------------------------------------------------------------------------------------------------------------------
def check_folds(fold_file, rows, freq, tsamp_ms, spins, dms, n_bins, dump_rows):
    """The --fold-out file holds a dump per whole `dump_rows` rows, each the psr_oracle fold of those rows ([T][f][b]: what the DM
    stage's buffer held) at the models and delays the driver derives (bf_psr_model_from_spin at the row time, dsabf::dm_delays at the
    run's channels): hits exactly, profiles bit for bit.  spins: (f0, f1, phase0) per pulsar; dms: per pulsar.  Returns the records."""
    from dsabeamformer_amd import host

    n_f, n_b, n_psr = rows.shape[1], rows.shape[2], len(spins)
    header, recs = psr_oracle.read_file(str(fold_file))
    assert [int(header[k]) for k in ("NPSR", "NFREQ", "NBINS", "NBEAMS")] == [n_psr, n_f, n_bins, n_b]
    assert [(q["first_row"], q["n_rows"]) for q in recs] == [(k * dump_rows, dump_rows) for k in range(rows.shape[0] // dump_rows)]
    delays = host.dm_delays(np.array(dms, np.float64), freq, float(freq[0]), tsamp_ms)
    assert delays.shape == (n_psr, n_f)
    models = [psr_oracle.model_from_spin(f0, f1, ph, tsamp_ms * 1e-3) for f0, f1, ph in spins]
    for q in recs:
        assert int(q["hits"].sum()) == n_psr * n_f * dump_rows and q["hits"].shape == (n_psr, n_f, n_bins)
        want_prof, want_hits = psr_oracle.fold(rows[q["first_row"]:q["first_row"] + dump_rows], models, delays, n_bins, first_row=q["first_row"])
        assert np.array_equal(q["hits"], want_hits) and np.array_equal(bits(q["profile"]), bits(want_prof))
    return recs
