"""numpy restatement of the pulse injector's contract (docs/INJECTION.md section 1; include/dsabf.h: bf_inj_*): bursts and trains
added to rows [row][freq][beam] with one fp32 multiply and one fp32 add per covering pulse -- bursts first, then trains, each in
ascending id --, cells outside every window left untouched, the lifetime of a pulse in host arithmetic, and the three host helpers
operation for operation.  numpy's float32 multiply and add round once each and are never fused.  Nothing here reads the library."""
import math

import numpy as np

import psr_oracle

MAX_TRAINS = 4
U64_MAX = (1 << 64) - 1
INVALID, STATE = -1, -4


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


class Injector:
    """The stage: add_burst / add_train / apply as the library's, on host arrays.  apply rewrites ``rows`` ([n][f][b] float32) in place.
    ``reverse=True`` applies the pulses of each kind in DESCENDING id -- what the tests use to show that their inputs make the
    order matter."""

    def __init__(self, n_freq, n_beams, max_rows, max_pulses=64, max_width=256, reverse=False):
        assert n_beams % 4 == 0 and 1 <= max_pulses <= 4096 and 1 <= max_width <= 4096
        self.n_freq, self.n_beams, self.max_rows, self.max_pulses, self.max_width = n_freq, n_beams, max_rows, max_pulses, max_width
        self.next_row, self.next_id, self.live, self.reverse = 0, 0, [], reverse

    def _tables(self, width, delay, profile, response):
        d = np.asarray(delay, np.int32)
        p = np.asarray(profile, np.float32)
        r = np.asarray(response, np.float32)
        assert d.shape == (self.n_freq,) and p.shape == (self.n_freq, width) and r.shape == (self.n_beams,)
        if np.any(d < 0):
            raise Refused(INVALID)
        return d.astype(np.int64), p.copy(), r.copy()

    def _store(self, pulse):
        if len(self.live) >= self.max_pulses:
            raise Refused(STATE)
        pulse["id"] = self.next_id
        self.next_id += 1
        self.live.append(pulse)
        return pulse["id"]

    def add_burst(self, t0, delay, profile, response):
        W = int(np.shape(profile)[1])
        if t0 < 0 or not 1 <= W <= self.max_width:
            raise Refused(INVALID)
        d, p, r = self._tables(W, delay, profile, response)
        if t0 + int(d.min()) < self.next_row:
            raise Refused(STATE)
        return self._store(dict(train=False, t0=int(t0), W=W, delay=d, profile=p, response=r))

    def add_train(self, model, delay, profile, response, first_row=0, n_rows=None):
        n_bins = int(np.shape(profile)[1])
        if not 2 <= n_bins <= min(self.max_width, 4096) or (n_rows is not None and n_rows < 1):
            raise Refused(INVALID)
        d, p, r = self._tables(n_bins, delay, profile, response)
        if first_row < self.next_row:
            raise Refused(STATE)
        if sum(q["train"] for q in self.live) >= MAX_TRAINS:
            raise Refused(STATE)
        end = U64_MAX if n_rows is None else min(first_row + n_rows, U64_MAX)
        return self._store(dict(train=True, model=tuple(int(v) for v in model), n_bins=n_bins, first=int(first_row), end=end, delay=d,
                                profile=p, response=r))

    def _spent(self, q):
        if q["train"]:
            return q["end"] <= self.next_row
        return self.next_row > q["t0"] + int(q["delay"].max()) + q["W"] - 1

    def apply(self, rows):
        assert rows.dtype == np.float32 and rows.shape[1:] == (self.n_freq, self.n_beams)
        n = rows.shape[0]
        if not 1 <= n <= self.max_rows:
            raise Refused(INVALID)
        first = self.next_row
        r_abs = np.arange(first, first + n, dtype=np.int64)[:, None]            # [n][1]
        chan = np.arange(self.n_freq)[None, :]
        order = sorted(self.live, key=lambda q: (q["train"], -q["id"] if self.reverse else q["id"]))
        for q in order:
            if q["train"]:
                lo, hi = max(first, q["first"]), min(first + n, q["end"])
                if lo >= hi:
                    continue
                b = psr_oracle.bins(q["model"], q["delay"], lo, hi - lo, q["n_bins"])      # [hi - lo][f]
                v = q["profile"][np.broadcast_to(chan, b.shape), b]                        # float32 [hi - lo][f]
                sl = rows[lo - first:hi - first]
                sl[...] = sl + v[:, :, None] * q["response"][None, None, :]
            else:
                i = r_abs - q["t0"] - q["delay"][None, :]                                   # [n][f]
                inside = (i >= 0) & (i < q["W"])
                if not inside.any():
                    continue
                rr, ff = np.nonzero(inside)
                v = q["profile"][ff, i[rr, ff]]                                             # float32 [cells]
                rows[rr, ff, :] = rows[rr, ff, :] + v[:, None] * q["response"][None, :]
        self.next_row = first + n
        self.live = [q for q in self.live if not self._spent(q)]


def inject(x, bursts=(), trains=(), cuts=None, reverse=False, max_width=4096):
    """x float32 [T][f][b] -> a copy with the pulses added.  bursts: (t0, delay, profile, response); trains: (model, delay, profile,
    response, first_row, n_rows); every add before the first apply, bursts' ids first; cuts: the row counts of the applies (None: one)."""
    x = np.array(x, np.float32)
    T, n_f, n_b = x.shape
    cuts = [T] if cuts is None else list(cuts)
    inj = Injector(n_f, n_b, max(cuts), max_pulses=4096, max_width=max_width, reverse=reverse)
    for b in bursts:
        inj.add_burst(*b)
    for t in trains:
        inj.add_train(*t)
    at = 0
    for c in cuts:
        inj.apply(x[at:at + c])
        at += c
    assert at == T
    return x


def burst_profile(n_freq, W, centre, sigma, fluence, smear=None):
    """bf_inj_burst_profile, fp64, the library's operations in the library's order; None where it refuses."""
    fl = np.broadcast_to(np.asarray(fluence, np.float64), (n_freq,))
    sm = np.ones(n_freq, np.int64) if smear is None else np.broadcast_to(np.asarray(smear, np.int64), (n_freq,))
    if not sigma > 0.0 or not math.isfinite(sigma) or not math.isfinite(centre) or np.any(sm < 1):
        return None
    out = np.zeros((n_freq, W), np.float32)
    two_var = 2.0 * sigma * sigma
    i = np.arange(W, dtype=np.float64)
    for f in range(n_freq):
        s = int(sm[f])
        half = float(s - 1) / 2.0
        total = np.zeros(W, np.float64)
        for j in range(s):
            d = ((i - centre) - float(j)) + half
            total = total + np.exp(-(d * d) / two_var)
        g = (1.0 / float(s)) * total
        N = 0.0
        for v in g:
            N = N + float(v)
        if not N > 0.0 or not math.isfinite(N) or not math.isfinite(fl[f]):
            return None
        out[f] = (fl[f] * (g / N)).astype(np.float32)
    return out


def nearest_trial(ladder, delay):
    lad = np.asarray(ladder, np.int64)
    cost = np.abs(lad - np.asarray(delay, np.int64)[None, :]).sum(axis=1)
    return int(np.argmin(cost))                     # the first minimum


def match(truth, cands, t_tol=0, dm_tol=0):
    """truth: (t_lo, t_hi, trial, beam) tuples; cands: records with t_start, dm, beam, width, snr.  int32 [len(truth)]."""
    best = np.full(len(truth), -1, np.int32)
    for k, (t_lo, t_hi, trial, beam) in enumerate(truth):
        for c in range(len(cands)):
            cd = cands[c]
            c_lo, c_hi = int(cd["t_start"]), int(cd["t_start"]) + int(cd["width"]) - 1
            if int(cd["beam"]) != beam or abs(int(cd["dm"]) - trial) > dm_tol or c_lo > t_hi + t_tol or c_hi < t_lo - t_tol:
                continue
            if best[k] < 0 or cd["snr"] > cands[best[k]]["snr"]:
                best[k] = c
    return best
