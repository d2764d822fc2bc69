"""Stamp oracle (docs/EVENTS.md section 2): the contract of bf_dm_stream_cut restated over a series held whole.

    out[r][g][tau] = sum over f = g fbin .. g fbin + fbin - 1, ascending, of
                     ( sum over i = 0 .. tbin - 1, ascending, of x[t0 + tau tbin + i + delay[dm][f]][f][beam] )

Every sum is fp32, sequential, starting from its first element, one rounding per add: the adds below are np.float32 arrays added
one term at a time (vectorised along tau only, which no sum runs over)."""
import numpy as np

SENTINEL = np.uint32(0x7FC0DEAD)      # a NaN with a payload: nothing the cut computes has these bits


def span(delays, dm, n_tau, tbin):
    """Rows request (t0, dm, .) needs: [t0, t0 + span)."""
    return n_tau * tbin + int(np.max(delays[dm]))


def status(delays, reqs, n_tau, tbin, oldest_row, next_row):
    """0 cut, 1 a row is older than oldest_row, 2 a row is not pushed yet (1 wins)."""
    return np.array([1 if t0 < oldest_row else 2 if t0 + span(delays, dm, n_tau, tbin) > next_row else 0 for t0, dm, _ in reqs], np.int32)


def stamp(series, delays, t0, dm, beam, n_tau, tbin, fbin):
    """series float32 [t][f][b] (row 0 = the first row ever pushed) -> float32 [n_f / fbin][n_tau]."""
    n_f = series.shape[1]
    assert series.dtype == np.float32 and n_f % fbin == 0
    out = np.empty((n_f // fbin, n_tau), np.float32)
    rows = t0 + np.arange(n_tau) * tbin
    for g in range(n_f // fbin):
        acc = None
        for f in range(g * fbin, (g + 1) * fbin):
            s = None
            for i in range(tbin):
                x = series[rows + i + int(delays[dm, f]), f, beam]
                s = x if s is None else (s + x).astype(np.float32)
            acc = s if acc is None else (acc + s).astype(np.float32)
        out[g] = acc
    return out


def cut(series, delays, reqs, n_tau, tbin, fbin, oldest_row, next_row):
    """What bf_dm_stream_cut leaves in a SENTINEL-filled output, as uint32 bits [n_req][n_f / fbin][n_tau], and the statuses."""
    st = status(delays, reqs, n_tau, tbin, oldest_row, next_row)
    out = np.full((len(reqs), series.shape[1] // fbin, n_tau), SENTINEL, np.uint32)
    for r, (t0, dm, beam) in enumerate(reqs):
        if st[r] == 0:
            out[r] = stamp(series, delays, t0, dm, beam, n_tau, tbin, fbin).view(np.uint32)
    return out, st
