"""GPU tests (-m gpu) of the single-pulse search stage on the shapes its kernels branch on (docs/SINGLE_PULSE.md §3): every compiled
sps_tile_kernel<K>, beam counts around one beam-lane group of 64, a maximum on every row of the tile layout, several pushes in
flight and the host-side baseline window.  Driver and checks: tests/support/sps_stage.py (records bit-equal to
tests/support/sps_oracle.py, statistics to n_t 2^-52, candidates equal in their integers, snr to 1e-9).

Every test is ONE function that loops over its cases, as tests/test_gpu_census.py does: the sweep cap of conftest.py thins
parametrised cases, and none of these may be left out."""
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import sps_oracle  # noqa: E402
from sps_stage import run_stage  # noqa: E402
from test_sps_cpu import SHAPE_SIZES as SIZES, SHAPE_T as T, pushes_of, series_for  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_T = max(SIZES)
ROTATIONS = (0, 3)          # as it stands (three 1-row pushes first), and starting on 126: the stream start inside a long push


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _rotated(rot):
    return SIZES[rot:] + SIZES[:rot]


def _no_snr_near(x, n_widths, sizes, threshold, **kw):
    """The oracle alone, every (trial, beam, push) record let through: no S/N of the run within a relative 1e-7 of the threshold
    (100 x the tolerance the S/N is compared to), so the device and the oracle cannot fall on different sides of it."""
    orc = sps_oracle.Search(x, n_widths, threshold=-np.inf, **kw)
    snr = np.array([c[5] for _, n in pushes_of(sizes, x.shape[1]) for c in orc.push(n)["cands"]])
    assert snr.size and np.all(np.abs(snr - threshold) > 1e-7 * threshold), np.abs(snr - threshold).min() / threshold


def test_every_compiled_width_on_the_edge_beam_counts(torch, bfmod):
    """Launches all eight sps_tile_kernel<K>, K = 1 .. 8, at each of the beam counts 4, 60 (less than one beam-lane group of 64:
    most lanes of every wave are outside the beams and still take part in the LDS exchange, the shuffles and the barriers), 64
    (exactly one group) and 68 (one group and one lane of a second workgroup): 32 cases, each with the push-size cycle as it
    stands and rotated by three.  The cycle holds 1-row pushes, one exact tile (128), a tile and one row, a tile less one row, two
    exact tiles, three tiles (257), and short pushes behind long ones (the new tail comes partly from the old one).  dm_first 17
    and a first_t beyond 2^40 label the candidates; every run yields candidates, and (the oracle alone) no S/N sits on the
    threshold."""
    thr, kw = 3.0, dict(dm_first=17, t_offset=2 ** 40 + 5)
    n_cases, t0 = 0, time.perf_counter()
    for n_beams in (4, 60, 64, 68):
        bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_beams, n_freq=8))
        for n_widths in range(1, 9):
            x = series_for(3, T, n_beams, 1000 * n_widths + n_beams)
            for rot in ROTATIONS:
                _no_snr_near(x, n_widths, _rotated(rot), thr, **kw)
                log = []
                n = run_stage(torch, bf, x, n_widths, _rotated(rot), MAX_T, threshold=thr, log=log, **kw)
                assert n > 0, (n_beams, n_widths, rot)
                got = np.concatenate([c for _, _, c in log])
                assert np.all(got["t_start"] >= 2 ** 40) and np.all((got["dm"] >= 17) & (got["dm"] < 20))
            n_cases += 1
        bf.close()
    assert n_cases == 32
    print("sps_tile_kernel<1..8> x 4 beam counts: %d cases x %d rotations, %.1f s" % (n_cases, len(ROTATIONS), time.perf_counter() - t0))


def test_a_maximum_at_every_time_position(torch, bfmod):
    """Zeros, and one spike per (trial, beam) at t = 2 (68 d + b) + b % 2: 340 distinct times 0 .. 679 -- every row tl + 16 i of
    the first tiles, both sides of every tile boundary and of every push seam, rows taken from the carried tail.  The spikes are
    small integers, so every association is exact: this is about WHERE the maximum is reported.  Against the oracle, and directly:
    the push that holds the spike reports it at t - lo for width 1, and for every wider boxcar that exists at t (the first window
    to reach the spike ends on the spike; the later windows tie and lose)."""
    n_dm, n_beams = 5, 68
    x = np.zeros((n_dm, T, n_beams), np.float32)
    d, b = np.meshgrid(np.arange(n_dm), np.arange(n_beams), indexing="ij")
    t_spike = 2 * (68 * d + b) + b % 2
    x[d, t_spike, b] = 1000 + t_spike % 7
    assert len(np.unique(t_spike)) == 340 and t_spike.min() == 0 and t_spike.max() == 679
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_beams, n_freq=8))
    n_cases, t0 = 0, time.perf_counter()
    for n_widths in (5, 8):
        for rot in ROTATIONS:
            log = []
            run_stage(torch, bf, x, n_widths, _rotated(rot), MAX_T, threshold=1e9, log=log)
            n_checked = 0
            for w, rec, _ in log:
                lo, n_t = w["first_t"], w["n_t"]
                here = (t_spike >= lo) & (t_spike < lo + n_t)
                where = (n_widths, rot, lo, n_t)
                assert np.array_equal(rec["t_end"][0][here], (t_spike - lo)[here]), where
                assert np.array_equal(rec["value"][0][here], (1000 + t_spike % 7)[here].astype(np.float32)), where
                for k in range(1, n_widths):
                    exists = here & (t_spike >= 2 ** k - 1)
                    assert np.array_equal(rec["t_end"][k][exists], (t_spike - lo)[exists]), where + (k,)
                n_checked += int(here.sum())
            assert n_checked == 340
            n_cases += 1
    bf.close()
    print("a maximum on each of 340 times: %d runs, %.1f s" % (n_cases, time.perf_counter() - t0))


# 400 times; at 8 widths the carried tail is 127 rows: 40, 1, 7, 64, 2 and 29 are shorter than it
C_SIZES = [40, 1, 129, 7, 64, 2, 128, 29]
# the window total n (sum of n_t over the last 3 pushes) after every push of the cycle
C_WINDOW_3 = [40, 41, 170, 137, 200, 73, 194, 159]


def test_several_pushes_in_flight_and_the_baseline_window(torch, bfmod):
    """68 beams, 2 trials, 8 widths, 400 times in 8 pushes.  (1) Three pushes behind the collector on three HIP streams with
    max_in_flight = 4: the result sets rotate, both tail buffers are reused, the stage's event chain orders the queues.  (2) Baseline
    windows of 1, 2 and 3 pushes.  (3) min_samples = 170 with a window of 3 pushes: the window total is 40, 41, then EXACTLY 170
    at push 2 -- the gate opens there (n < min_samples is what skips), closes again at 137, opens at 200, ...: no candidates where
    the total is below 170, some at every push where it is not.  The oracle alone: no S/N within 1e-7 of the threshold."""
    n_dm, n_beams, n_widths, thr = 2, 68, 8, 3.0
    x = series_for(n_dm, 400, n_beams, 77)
    assert sum(C_SIZES) == x.shape[1]
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_beams, n_freq=8))
    t0 = time.perf_counter()
    _no_snr_near(x, n_widths, C_SIZES, thr)
    assert run_stage(torch, bf, x, n_widths, C_SIZES, max(C_SIZES), lag=3, n_streams=3, threshold=thr) > 0
    for baseline in (1, 2, 3):
        _no_snr_near(x, n_widths, C_SIZES, thr, baseline_pushes=baseline)
        log = []
        assert run_stage(torch, bf, x, n_widths, C_SIZES, max(C_SIZES), threshold=thr, baseline_pushes=baseline, log=log) > 0
        assert [w["n"] for w, _, _ in log] == [sum(C_SIZES[max(0, j + 1 - baseline):j + 1]) for j in range(len(C_SIZES))]
    log = []
    run_stage(torch, bf, x, n_widths, C_SIZES, max(C_SIZES), lag=2, n_streams=3, threshold=thr, baseline_pushes=3, min_samples=170, log=log)
    assert [w["n"] for w, _, _ in log] == C_WINDOW_3 and C_WINDOW_3[2] == 170
    for j, (w, _, cands) in enumerate(log):
        assert (len(cands) > 0) == (C_WINDOW_3[j] >= 170), (j, len(cands))
    assert [len(c) for _, _, c in log[:2]] == [0, 0] and len(log[2][2]) > 0            # the crossing: push 2
    bf.close()
    print("in flight / baseline window / min_samples: 5 runs, %.1f s" % (time.perf_counter() - t0))
