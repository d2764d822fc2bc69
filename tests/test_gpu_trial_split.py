"""GPU tests of the DM-side stages on a SHARDED run of `beam`, where a stage is addressed with a local trial index that must become a global
one or the reverse (csrc/bf_run_observation.cpp: plan.dm_first; csrc/beam_main.cpp: wire_*, per_trial_share).  Every run is `beam -j 29`
(25 burn-in reads + 4 analysed blocks of 256 rows: two fold dumps of 512 rows, the conditioner's window of 4 filled, and the stamp of
every injected burst inside the run) with the conditioner, injector, folder, periodicity search, single-pulse search, event builder and
stamp cut on, as child processes over tests/support/fake_rccl.cpp (the loopback stand-in for RCCL), at most four at a time.

One function per leg, nothing parametrised: the root leg (`-R 2`, everything on the gather root, beside the same command as one process), the even
split (`-R 2 -X -N 8`: 4 + 4), the ragged split (`-N 7`: 4 + 3, with --ffa-detrend), four ranks (`-R 4 -X -N 6`: 2, 2, 1, 1) and the
surplus rank (`-N 1`: rank 1 has no trials).  Every file of every rank is held to its stage's own oracle by the functions of
tests/support/dm_side.py -- the ones the stages' single-process end-to-end tests call with dm_first = 0.

The rows a rank dedisperses are recomputed from rank 0's -w file (the raw gathered band): inj_oracle, then cond_oracle, push by push.
The bursts are aimed at trials of the ranks with dm_first > 0 -- one of them at the first trial of rank 1's share, so that its
candidates lie on both sides of a share boundary -- and the assertions on the oracles' own counts (`found`) decide that every such rank
has a candidate, an unflagged event, a stamp and a periodicity candidate to get wrong."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dm_side as ds  # noqa: E402
import evt_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu

N_AN, ROWS, TSAMP, DM_MAX = 4, 256, 0.131, 250.0      # analysed blocks, rows of a block, the driver's default sample time, -M
THR, N_WIDTHS, IB = 4.0, 6, 255                        # -S, -B, -i
EVT = dict(max_width=1 << (N_WIDTHS - 1), ib_beam=IB)
FFA, FFA_THR, DETREND = (2, 64, 2, 8, 13, 2), 3.0, (8, 5)     # (tdec, n_seg, n_oct, p_lo, p_hi, n_widths), --ffa-snr, --ffa-detrend
SPINS, FOLD_DMS, FOLD_BINS, FOLD_ROWS = [(31.7, -0.4, 0.3), (1200.0, 0.0, 0.0)], [25.0, 0.0], 16, 512
COND_WINDOW = 4
FLUENCE, BURST_W, TRAIN = 2.0e5, 8, (400.0, 5, 3.0e4, 0.05, 64)    # per channel, rows; the train: f0, beam, amplitude, duty, bins
PER_TRIAL = ("dm.bin", "cands.txt", "ev.txt", "st.bin", "ffa.txt", "folds.bin", "truth.txt")
DM_SIDE_TITLES = ("DM stage:", "Conditioner:", "Injector:", "Pulsar folder:", "Periodicity search:", "Single-pulse search:", "Events:")
TIMEOUT = 240


def stage_args(n_cap, dms, bursts, train_trial, detrend):
    """The DM-side options of tests/test_gpu_all_stages.py without the voltage cuts (a sharded run refuses them), the pulses aimed at
    trials of THIS ladder.  bursts: (t0, trial, beam)."""
    args = ["-j", str(25 + N_AN), "-i", str(IB), "-w", "det.bin", "-M", str(int(DM_MAX)), "-N", str(n_cap), "-S", str(int(THR)), "-B", str(N_WIDTHS),
            "-n", str(COND_WINDOW), "-W", "dm.bin", "-C", "cands.txt", "--events", "ev.txt", "--stamps", "st.bin",
            "--fold", "31.7:-0.4:0.3", "--fold-dm", "25", "--fold", "1200", "--fold-bins", str(FOLD_BINS), "--fold-rows", str(FOLD_ROWS), "--fold-out", "folds.bin",
            "--ffa", "8:13", "--ffa-seg", "64", "--ffa-dec", "2", "--ffa-oct", "2", "--ffa-widths", "2", "--ffa-snr", "3.0", "--ffa-out", "ffa.txt"]
    if detrend:
        args += ["--ffa-detrend", "%d:%d" % detrend]
    for t0, trial, beam in bursts:
        args += ["--inject", "%d:%.17g:%d:%.17g:1:%d" % (t0, float(dms[trial]), beam, FLUENCE, BURST_W)]
    args += ["--inject-train", "%.17g:%.17g:%d:%.17g" % (TRAIN[0], float(dms[train_trial]), TRAIN[1], TRAIN[2]), "--inject-out", "truth.txt"]
    return args


def run_ranks(cwd, args, world, split):
    """The ranks of one sharded run, side by side; every return code asserted before anything is read.  A rank that does not end
    within its time limit ends the test: all of them are killed, and nothing more is started."""
    from dsabeamformer_amd import build

    env = dict(os.environ, DSABF_RCCL_LIB=ds.fake_rccl())
    cmd = lambda rk: [build.BEAM] + args + ["-R", str(world), "-r", str(rk), "-I", "id"] + (["-X"] if split else [])  # noqa: E731
    procs = [subprocess.Popen(cmd(rk), env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rk in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=TIMEOUT)[0])
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        pytest.fail("a rank of `%s` did not end within %d s: %s" % (" ".join(cmd(0)), TIMEOUT, "\n".join(outs)[-3000:]))
    assert [p.returncode for p in procs] == [0] * world, "\n".join(o[-3000:] for o in outs)
    return outs


def dm_side_lines(stdout):
    return [l for l in ds.closing_lines(stdout) if l.startswith(DM_SIDE_TITLES)]


def stage_rows(cwd, dms, freq, bursts, train_trial):
    """What every rank that holds the band dedisperses: rank 0's raw -w rows with the pulses added, then conditioned, push by push."""
    raw = ds.read_rows(os.path.join(cwd, "det.bin"))
    assert raw.shape == (N_AN * ROWS, 256, 256)
    rows = ds.injected_rows(raw, ROWS, freq, TSAMP, [(t0, float(dms[k]), beam, FLUENCE, 1.0, BURST_W) for t0, k, beam in bursts],
                            [(TRAIN[0], float(dms[train_trial]), TRAIN[1], TRAIN[2], TRAIN[3], TRAIN[4])])
    assert not np.array_equal(ds.bits(rows), ds.bits(raw))
    return ds.conditioned_rows(rows, ROWS, COND_WINDOW)[0]


def check_rank(cwd, rk, out, first, count, n_cap, rows, freq, delays, detrend, split=True):
    """Every per-trial file of rank rk against its oracle; split=False: the gather root of a run without -X, whose files carry no
    rank.  Returns what the oracles found there, and the files' bytes that every rank with trials must share."""
    sfx = ".%d" % rk if split else ""
    name = lambda n: os.path.join(cwd, n + sfx)  # noqa: E731
    assert (("Shard %d dedisperses trials %d .. %d" % (rk, first, first + count - 1)) in out) == split
    assert ("DM stage: trials %d .. %d of %d" % (first, first + count - 1, n_cap)) in out
    hdr, data, chunks = ds.check_dm_file(name("dm.bin"), rows, delays, first, count)
    assert ("Wrote %d dedispersed samples x %d trials to dm.bin%s" % (data.shape[1], count, sfx)) in out
    got, _ = ds.check_candidates(name("cands.txt"), out, data, chunks, N_WIDTHS, THR, first, printed="cands.txt" + sfx)
    cands, events = ds.check_events(name("ev.txt"), name("cands.txt"), **EVT)
    assert all(first <= e["dm_lo"] <= e["dm_hi"] < first + count for e in events)          # a cluster ends where the share ends
    stamps = ds.check_stamps(name("st.bin"), out, cands, chunks, len(events), rows, delays, **EVT)
    assert all(first <= s["dm"] < first + count for s in stamps)                            # (the GLOBAL trial in every record)
    _, ffa_want, _ = ds.check_ffa(name("ffa.txt"), out, data, FFA, FFA_THR, first, detrend)
    ds.check_folds(name("folds.bin"), rows, freq, TSAMP, SPINS, FOLD_DMS, FOLD_BINS, FOLD_ROWS)
    found = dict(candidates=len(got), unflagged=sum(1 for e in events if not e["flags"]), stamps=len(stamps), periodicity=len(ffa_want))
    print("rank %d%s, trials %d .. %d: %s" % (rk, "" if split else " (the gather root)", first, first + count - 1, found))
    return found, cands, open(name("folds.bin"), "rb").read(), open(name("truth.txt")).read()


def split_leg(cwd, world, n_cap, bursts, train_trial, detrend=None):
    """One `-X` run and all its checks.  bursts: (t0, trial, beam), the first of them at the first trial of rank 1's share."""
    from dsabeamformer_amd import host

    cwd = str(cwd)
    dms, freq, delays = ds.beam_ladder(DM_MAX, n_cap, 256, TSAMP)
    assert len(dms) == n_cap
    shares = [host.dm_trial_share(n_cap, world, rk) for rk in range(world)]
    assert sum(c for _, c in shares) == n_cap and shares[0][0] == 0
    outs = run_ranks(cwd, stage_args(n_cap, dms, bursts, train_trial, detrend), world, split=True)
    assert not any(os.path.exists(os.path.join(cwd, n)) for n in PER_TRIAL)                  # none without a rank
    rows = stage_rows(cwd, dms, freq, bursts, train_trial)
    cands, folds, truths = {}, set(), set()
    for rk, (first, count) in enumerate(shares):
        if count == 0:
            continue
        found, cands[rk], fold, truth = check_rank(cwd, rk, outs[rk], first, count, n_cap, rows, freq, delays, detrend)
        # the condition on the input: the oracles found something of every kind on this rank (asked of rank 0 as well)
        assert min(found.values()) >= 1, (rk, found)
        folds.add(fold)
        truths.add(truth)
    assert len(folds) == 1 and len(truths) == 1            # the folder and the injector work in front of the trials: the same on every rank
    truth = [l.split() for l in truths.pop().splitlines() if not l.startswith("#")]
    assert [int(l[4]) for l in truth] == [k for _, k, _ in bursts] + [train_trial]           # the trial of every pulse over the whole ladder
    if world > 1 and shares[1][1]:
        # the first burst's candidates lie on both sides of rank 1's first trial: ONE cluster over the whole ladder, cut by the split
        edge = shares[1][0]
        both = eo.events(np.concatenate([cands[0], cands[1]]), **EVT)
        assert any(e["dm_lo"] < edge <= e["dm_hi"] and int(e["best"]["beam"]) == bursts[0][2] for e in both)
    return outs, shares


DATA_FREE_TITLES = ("DM stage:", "Conditioner:", "Injector:", "Pulsar folder:")     # closing lines that do not depend on the powers


def test_the_root_leg_runs_every_stage_on_the_gathered_band(tmp_path):
    """`-R 2` without -X: both shards beamform, rank 0 gathers the band and runs every DM-side stage on it; rank 1, given the same
    options, writes nothing.  Rank 0's files carry no rank and are held to the oracles over ITS -w file with dm_first = 0 and the
    whole ladder -- the checks of the stages' one-process tests.  Beside it the same command as one process: the ladder and the
    chunking are the same, so truth.txt is the same bytes, the DM-side closing lines come in the same order, and those that do not
    depend on the powers are equal.

    (The other files of the two runs are NOT the same bytes, and cannot be with the junk source: a shard's source serves the junk
    bytes of the SHARD's geometry, 128 channels, so the band the root gathers -- the same 128 channels' voltages twice, under
    each half's own weights -- is another band than the 256 channels one process reads; tests/test_gpu_round5.py computes its
    series per shard for that reason.  Each run's files are the oracle's over its own band instead.)"""
    from dsabeamformer_amd import build

    bursts, train_trial = [(300, 4, 3), (460, 6, 9)], 5
    dms, freq, delays = ds.beam_ladder(DM_MAX, 8, 256, TSAMP)
    args = stage_args(8, dms, bursts, train_trial, None)
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    r = subprocess.run([build.BEAM] + args, capture_output=True, text=True, timeout=TIMEOUT, cwd=one)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    outs = run_ranks(str(two), args, 2, split=False)
    assert set(os.listdir(two)) - {"id"} == set(os.listdir(one)) == set(PER_TRIAL) | {"det.bin"}     # no file of rank 1's, none with a rank
    rows = stage_rows(str(two), dms, freq, bursts, train_trial)
    found, _, _, _ = check_rank(str(two), 0, outs[0], 0, 8, 8, rows, freq, delays, None, split=False)
    assert min(found.values()) >= 1, found
    assert filecmp.cmp(one / "truth.txt", two / "truth.txt", shallow=False) and not filecmp.cmp(one / "det.bin", two / "det.bin", shallow=False)
    lines, root = dm_side_lines(r.stdout), dm_side_lines(outs[0])
    assert [l.split(":")[0] + ":" for l in lines] == [l.split(":")[0] + ":" for l in root] == list(DM_SIDE_TITLES), (lines, root)
    assert [l for l in root if l.startswith(DATA_FREE_TITLES)] == [l for l in lines if l.startswith(DATA_FREE_TITLES)]
    assert "Synchronized" in outs[1] and dm_side_lines(outs[1]) == [] and "Wrote" not in outs[1]


def test_the_even_split(tmp_path):
    """`-R 2 -X -N 8`: trials 0 .. 3 and 4 .. 7.  Bursts at trial 4 (the boundary) and trial 6, the train at trial 5."""
    _, shares = split_leg(tmp_path, 2, 8, [(300, 4, 3), (460, 6, 9)], 5)
    assert shares == [(0, 4), (4, 4)]


def test_the_ragged_split_with_the_detrend(tmp_path):
    """`-R 2 -X -N 7 --ffa-detrend 8:5`: trials 0 .. 3 and 4 .. 6.  Bursts at trial 4 (the boundary) and trial 6, the train at trial 5."""
    _, shares = split_leg(tmp_path, 2, 7, [(300, 4, 3), (460, 6, 9)], 5, DETREND)
    assert shares == [(0, 4), (4, 3)]


def test_four_ranks(tmp_path):
    """`-R 4 -X -N 6`: four processes of 64 channels each, trials 0 .. 1, 2 .. 3, 4 and 5.  Bursts at trial 2 (the boundary), 4 and 5,
    the train at trial 5."""
    _, shares = split_leg(tmp_path, 4, 6, [(300, 2, 3), (460, 4, 9), (380, 5, 13)], 5)
    assert shares == [(0, 2), (2, 2), (4, 1), (5, 1)]


def test_the_surplus_rank_only_beamforms(tmp_path):
    """`-R 2 -X -N 1`: rank 0 has the one trial and is checked as every rank; rank 1 has none -- it says so, beamforms, sends its
    channels, exits 0, and neither creates a per-trial file nor prints a DM-side closing line."""
    outs, shares = split_leg(tmp_path, 2, 1, [(300, 0, 3)], 0)
    assert shares == [(0, 1), (1, 0)]
    assert not any(os.path.exists(tmp_path / ("%s.1" % n)) for n in PER_TRIAL)
    assert "Shard 1 dedisperses no trials: the ladder has 1, fewer than the 2 shards" in outs[1] and "dedisperses trials" not in outs[1]
    assert "Synchronized" in outs[1] and dm_side_lines(outs[1]) == [] and "Wrote" not in outs[1]
