"""The end-to-end scenario of docs/CONDITIONING.md section 5: a band with a bandpass, three interference channels, two DM-0 bursts
and one dispersed pulse; its settings and its assertions, shared by tests/test_cond_cpu.py (the oracles alone) and
tests/test_gpu_cond.py (the device).  numpy only."""
from __future__ import annotations

import numpy as np

import sps_oracle

F, B, PUSH_ROWS, N_PUSHES, N_DM = 32, 8, 48, 6, 6
T = PUSH_ROWS * N_PUSHES
BAD_CHANNELS = (5, 17, 18)
BURST_ROWS = (70, 71, 160)
PULSE_BEAM, PULSE_TRIAL, PULSE_ROWS = 3, 4, (100, 101)
# The amplitudes (noise: mean 100, deviation 25 per unit gain), chosen so that the assertions below hold with room.  The pulse's S/N
# saturates near sqrt(samples of the window / 2) ~ 9 whatever its height -- its own two samples dominate the deviation it is
# measured against -- so what decides "the raw run's best candidate is not the pulse" is the ratio of burst to pulse: the burst
# (all 32 channels) beats the pulse (sum of the gains ~ 80) in the raw stream from about 2.5 x its height on.  300 and 50 give, on the
# oracles: conditioned, the pulse 8.4 against 3.9 for the best other candidate; raw, a burst 7.3 against the pulse 6.5.
BURST_AMPLITUDE, PULSE_AMPLITUDE = 300.0, 50.0
BASELINE_PUSHES, AUTO_THRESHOLD, N_WIDTHS, MIN_SAMPLES = 3, 5.0, 3, 16


def delays():
    """Trials d = 1 .. 6: no trial is DM 0 itself.  There the zero-DM'd channels sum to their own rounding residue, and the S/N of that
    residue (8 at the burst rows, where the summands are largest) says nothing about the stage."""
    nu = np.linspace(1.53, 1.28, F)
    x = (nu ** -2 - nu[0] ** -2) / (nu[-1] ** -2 - nu[0] ** -2)
    return np.rint(3.0 * np.arange(1, N_DM + 1)[:, None] * x[None, :]).astype(np.int32)


def make():
    """The raw series [T][F][B] float32 and the delays [N_DM][F]."""
    rng = np.random.default_rng(7)
    gain = 1.0 + 3.0 * rng.random(F)
    x = 100.0 * rng.gamma(16.0, 1.0 / 16.0, (T, F, B)) * gain[None, :, None]
    for f in BAD_CHANNELS:
        x[:, f, :] += rng.gamma(0.5, 400.0, T)[:, None]
    for t in BURST_ROWS:
        x[t] += BURST_AMPLITUDE
    d = delays()
    for f in range(F):
        for t in PULSE_ROWS:
            x[t + d[PULSE_TRIAL, f], f, PULSE_BEAM] += PULSE_AMPLITUDE * gain[f]
    return x.astype(np.float32), d


def dedisperse(series, d):
    """out[dm][t][b] = sum over f, ascending, fp32, of series[t + delay[dm][f]][f][b] for the complete times."""
    n_out = series.shape[0] - int(d.max())
    out = np.zeros((d.shape[0], n_out, series.shape[2]), np.float32)
    for k in range(d.shape[0]):
        for f in range(series.shape[1]):
            out[k] = out[k] + series[d[k, f]:d[k, f] + n_out, f, :]
    return out


def chunk_sizes(d):
    """Output times of every push of PUSH_ROWS rows."""
    D, out = int(d.max()), []
    for k in range(N_PUSHES):
        out.append(max(0, (k + 1) * PUSH_ROWS - D) - max(0, k * PUSH_ROWS - D))
    return out


def search(dedispersed, d):
    """Every candidate of the search over the chunks, threshold -inf: list of (t_start, dm, beam, width, peak, snr)."""
    orc = sps_oracle.Search(dedispersed, N_WIDTHS, baseline_pushes=8, min_samples=MIN_SAMPLES, threshold=-np.inf)
    return [c for n in chunk_sizes(d) if n for c in orc.push(n)["cands"]]


def is_pulse(c, d):
    """The candidate's boxcar, in the pulse's beam, overlaps where trial c.dm puts the pulse's power."""
    if c[2] != PULSE_BEAM:
        return False
    shift = d[PULSE_TRIAL].astype(int) - d[c[1]].astype(int)       # the pulse in channel f lands on rows PULSE_ROWS + shift[f]
    lo, hi = PULSE_ROWS[0] + shift.min(), PULSE_ROWS[-1] + shift.max()
    return c[0] <= hi and c[0] + c[3] - 1 >= lo


def check(cands, d, mask=None):
    """The assertions of the scenario on the candidates of a conditioned run (and on the mask of its last push)."""
    if mask is not None:
        assert set(np.flatnonzero(mask)) == set(BAD_CHANNELS), np.flatnonzero(mask)
    snr = np.array([c[5] for c in cands])
    best = cands[int(snr.argmax())]
    assert np.count_nonzero(snr == snr.max()) == 1
    assert (best[0], best[1], best[2], best[3]) == (PULSE_ROWS[0], PULSE_TRIAL, PULSE_BEAM, 2), best
    others = np.array([c[5] for c in cands if not is_pulse(c, d)])
    print("pulse S/N %.3f, best other candidate %.3f" % (best[5], others.max()))
    assert best[5] >= 1.5 * others.max()
    # nothing that decides an assertion sits within 1e-6 of what it is compared with
    assert abs(best[5] - 1.5 * others.max()) > 1e-6 * best[5]
    second = np.sort(snr)[-2]
    assert best[5] - second > 1e-6 * best[5]
    return best
