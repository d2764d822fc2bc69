"""numpy restatement of the single-pulse search stage (docs/SINGLE_PULSE.md): the boxcar tree over a WHOLE series, the per-push
peak records and statistics cut from it, and the candidate selection.  No GPU, no libdsabf."""
from __future__ import annotations

import numpy as np

CAND_FIELDS = ("t_start", "dm", "beam", "width", "peak", "snr")


def tree_sums(x, n_widths):
    """S_k for k < n_widths over a series x [n_dm][T][n_beams] float32: S_0 = x, S_k[t] = S_{k-1}[t] + S_{k-1}[t - 2^(k-1)], fp32,
    one rounding per add.  S_k[:, t] is meaningful for t >= 2^k - 1 only (earlier entries are left as they were)."""
    s = np.ascontiguousarray(x, np.float32)
    out = [s]
    for k in range(1, n_widths):
        d = 1 << (k - 1)
        nxt = s.copy()
        if s.shape[1] > d:
            nxt[:, d:] = s[:, d:] + s[:, :-d]          # float32 + float32: one rounding
        out.append(nxt)
        s = nxt
    return out


def running_sums(x, n_widths):
    """The same windows summed left to right (oldest sample first), fp32: a different association, NOT the contract."""
    x = np.ascontiguousarray(x, np.float32)
    out = []
    for k in range(n_widths):
        w = 1 << k
        s = np.zeros_like(x)
        for j in range(w - 1, -1, -1):                 # x[t - w + 1] first
            if x.shape[1] > j:
                s[:, j:] = s[:, j:] + x[:, :x.shape[1] - j]
        out.append(s)
    return out


def push_records(sums, lo, hi):
    """Peak records of the push covering series times [lo, hi): value, t_end [K][n_dm][n_beams] (t_end relative to lo; -inf / -1
    where no time of the push has S_k), from whole-series sums (tree_sums)."""
    n_dm, _, n_beams = sums[0].shape
    value = np.full((len(sums), n_dm, n_beams), -np.inf, np.float32)
    t_end = np.full((len(sums), n_dm, n_beams), -1, np.int32)
    for k, s in enumerate(sums):
        first = max(lo, (1 << k) - 1)
        if first >= hi:
            continue
        seg = s[:, first:hi]
        arg = np.argmax(seg, axis=1)                   # first occurrence of the maximum
        value[k] = np.take_along_axis(seg, arg[:, None, :], axis=1)[:, 0, :]
        t_end[k] = arg + (first - lo)
    return value, t_end


def push_stats(x, lo, hi):
    seg = np.asarray(x[:, lo:hi], np.float64)
    return seg.sum(axis=1), (seg * seg).sum(axis=1)


def select(value, t_end, tot_sum, tot_sumsq, n, first_t=0, dm_first=0, min_samples=64, threshold=8.0):
    """The candidate selection, fp64: list of (t_start, dm, beam, width, peak, snr) in (d, b) order."""
    n_widths, n_dm, n_beams = value.shape
    if n == 0 or n < min_samples:
        return []
    mu = np.asarray(tot_sum, np.float64) / float(n)
    var = np.asarray(tot_sumsq, np.float64) / float(n) - mu * mu
    sigma = np.sqrt(np.maximum(var, 0.0))
    out = []
    for d in range(n_dm):
        for b in range(n_beams):
            if sigma[d, b] == 0.0:
                continue
            best_k, best = -1, 0.0
            for k in range(n_widths):
                if t_end[k, d, b] < 0:
                    continue
                w = float(1 << k)
                snr = (float(value[k, d, b]) - w * mu[d, b]) / (sigma[d, b] * np.sqrt(w))
                if best_k < 0 or snr > best:
                    best_k, best = k, snr
            if best_k < 0 or not best >= threshold:
                continue
            w = 1 << best_k
            out.append((int(first_t) + int(t_end[best_k, d, b]) - (w - 1), dm_first + d, b, w, float(value[best_k, d, b]), float(best)))
    return out


class Search:
    """The stage over a whole series x [n_dm][T][n_beams] (time 0 = the first sample the stage is given): push(n_t) returns the
    records of the next n_t times and the candidates bf_sps_collect must give for them."""

    def __init__(self, x, n_widths, dm_first=0, baseline_pushes=8, min_samples=64, threshold=8.0, t_offset=0):
        self.x = np.ascontiguousarray(x, np.float32)
        self.sums = tree_sums(self.x, n_widths)
        self.pos, self.window = 0, []
        self.dm_first, self.baseline, self.min_samples, self.threshold, self.t_offset = dm_first, baseline_pushes, min_samples, threshold, t_offset

    def push(self, n_t):
        lo, hi = self.pos, self.pos + n_t
        assert hi <= self.x.shape[1]
        value, t_end = push_records(self.sums, lo, hi)
        s, q = push_stats(self.x, lo, hi)
        self.window = (self.window + [(n_t, s, q)])[-self.baseline:]
        n = sum(w[0] for w in self.window)
        tot_s, tot_q = np.zeros_like(s), np.zeros_like(q)
        for _, ws, wq in self.window:                  # oldest first
            tot_s, tot_q = tot_s + ws, tot_q + wq
        cands = select(value, t_end, tot_s, tot_q, n, self.t_offset + lo, self.dm_first, self.min_samples, self.threshold)
        self.pos = hi
        return {"value": value, "t_end": t_end, "sum": s, "sumsq": q, "first_t": self.t_offset + lo, "n_t": n_t, "cands": cands,
                "totals": (tot_s, tot_q), "n": n}


def assert_candidates_equal(got, want, rtol):
    """got: numpy structured array from the library; want: list of tuples from select()."""
    assert len(got) == len(want), (len(got), len(want))
    if not len(want):
        return
    w = list(zip(*want))
    for i, f in enumerate(CAND_FIELDS[:4]):
        assert np.array_equal(np.asarray(got[f], np.int64), np.asarray(w[i], np.int64)), f
    assert np.array_equal(got["peak"], np.asarray(w[4], np.float32))
    assert np.allclose(got["snr"], np.asarray(w[5]), rtol=rtol, atol=0.0)
