"""numpy restatement of the periodicity search's running-median detrend and of the harmonic sift (docs/PERIODICITY.md sections 1a
and 1b), beside tests/support/ffa_oracle.py, which restates everything behind them.  No GPU, no libdsabf.  Segments are
[n_dm][n_seg][n_beams] float32, like ffa_oracle's.  Three MUTANTS of the detrend, for the CPU assertions that an input can tell a
wrong kernel from a right one: the upper median, a piecewise-constant trend, and r0 + a d with one rounding instead of three."""
from __future__ import annotations

import math

import numpy as np

import ffa_oracle

GROUP_FIELDS = ("n_members", "n_beams", "dm_lo", "dm_hi", "n_harmonic", "reserved")
# bf_ffa_group (include/dsabf.h), as the C compiler lays it out
GROUP_DTYPE = np.dtype([("head", ffa_oracle.CAND_DTYPE), ("n_members", np.int32), ("n_beams", np.int32), ("dm_lo", np.int32), ("dm_hi", np.int32),
                        ("n_harmonic", np.int32), ("reserved", np.int32)], align=True)


def check_params(n_seg, blk, win):
    assert 1 <= blk <= 256 and blk & (blk - 1) == 0 and n_seg % blk == 0 and 1 <= win <= 129 and win % 2 == 1, (n_seg, blk, win)


def keys(m):
    """The total order of the median: bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000), compared as uint32; -0 < +0."""
    bits = np.ascontiguousarray(m, np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkeys(k):
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def block_means(seg, blk):
    """m[c] = (((y[c blk] + y[c blk + 1]) + ...) + y[c blk + blk - 1]) 2^-log2(blk): an fp32 left fold, the first term as it is."""
    seg = np.ascontiguousarray(seg, np.float32)
    n_dm, n_seg, nb_ = seg.shape
    g = seg.reshape(n_dm, n_seg // blk, blk, nb_)
    acc = g[:, :, 0].copy()
    for i in range(1, blk):
        acc = acc + g[:, :, i]
    return acc * np.float32(1.0 / blk)


def running_median(m, win, upper=False):
    """r[c]: the element of rank (n - 1) >> 1 of m[max(0, c - h) .. min(nb - 1, c + h)] in the order of keys() -- a selection, to
    the bit.  `upper` (a mutant): rank n >> 1."""
    k = keys(m)                                   # [n_dm][nb][n_beams]
    nb, h = k.shape[1], (win - 1) // 2
    out = np.empty_like(k)
    done = np.zeros(nb, bool)
    if nb >= win:                                 # the full windows, c = h .. nb - 1 - h, in one sort
        w = np.lib.stride_tricks.sliding_window_view(k, win, axis=1)          # [n_dm][nb - win + 1][n_beams][win]
        out[:, h:nb - h] = np.sort(w, axis=-1)[..., win >> 1 if upper else (win - 1) >> 1]
        done[h:nb - h] = True
    for c in np.flatnonzero(~done):
        lo, hi = max(0, c - h), min(nb - 1, c + h)
        n = hi - lo + 1
        out[:, c] = np.sort(k[:, lo:hi + 1], axis=1)[:, n >> 1 if upper else (n - 1) >> 1]
    return unkeys(out)


def trend_of(r, n_seg, blk, constant=False, fused=False):
    """The piecewise linear trend through the block centres, [n_dm][n_seg][n_beams] float32: with k = 2u + 1 - blk, r[0] for k < 0,
    c0 = k // (2 blk), r[nb - 1] for c0 >= nb - 1, else a = (k - 2 blk c0) / (2 blk) (exact), d = fl(r[c0 + 1] - r[c0]),
    q = fl(a d), fl(r[c0] + q).  Mutants: `constant` r[u // blk]; `fused` r[c0] + a d with the product and the sum unrounded (fp64:
    a has 9 bits, d 24) and one rounding at the end."""
    nb = r.shape[1]
    u = np.arange(n_seg)
    if constant:
        return r[:, u // blk]
    k = 2 * u + 1 - blk
    c0 = np.clip(k // (2 * blk), 0, max(nb - 2, 0))
    c1 = np.minimum(c0 + 1, nb - 1)
    a = ((k - 2 * blk * c0) / (2.0 * blk)).astype(np.float32)[None, :, None]
    r0, r1 = r[:, c0], r[:, c1]
    with np.errstate(all="ignore"):
        if fused:
            lin = (r0.astype(np.float64) + a.astype(np.float64) * (r1.astype(np.float64) - r0.astype(np.float64))).astype(np.float32)
        else:
            d = r1 - r0
            q = a * d
            lin = r0 + q
    left, right = (k < 0)[None, :, None], (k // (2 * blk) >= nb - 1)[None, :, None]
    return np.where(left, r[:, :1], np.where(right, r[:, nb - 1:], lin)).astype(np.float32)


def detrend(seg, blk, win, mutant=None):
    """y' of one complete segment seg [n_dm][n_seg][n_beams] (a new array).  mutant: None, 'upper', 'constant' or 'fused'."""
    seg = np.ascontiguousarray(seg, np.float32)
    check_params(seg.shape[1], blk, win)
    assert mutant in (None, "upper", "constant", "fused")
    r = running_median(block_means(seg, blk), win, upper=mutant == "upper")
    with np.errstate(all="ignore"):
        return seg - trend_of(r, seg.shape[1], blk, constant=mutant == "constant", fused=mutant == "fused")


class Search:
    """ffa_oracle.Search with the detrend between the decimation and everything else: per complete segment the records, the
    statistics and the candidates bf_ffa_collect must give with bf_ffa_set_detrend(blk, win).  blk == 0: no detrend."""

    def __init__(self, x, tdec, n_seg, n_oct, p_lo, p_hi, n_widths, blk, win, dm_first=0, threshold=8.0, t_offset=0, mutant=None):
        self.y = ffa_oracle.decimate(x, tdec)
        self.cfg = (tdec, n_seg, n_oct, p_lo, p_hi, n_widths)
        self.blk, self.win, self.mutant = blk, win, mutant
        self.dm_first, self.threshold, self.t_offset = dm_first, threshold, t_offset

    def series(self):
        """The detrended segments, [n_dm][n_seg][n_beams] each."""
        n_seg = self.cfg[1]
        segs = [self.y[:, s * n_seg:(s + 1) * n_seg] for s in range(self.y.shape[1] // n_seg)]
        return [detrend(s, self.blk, self.win, self.mutant) if self.blk else s for s in segs]

    def segments(self):
        tdec, n_seg, n_oct, p_lo, p_hi, n_widths = self.cfg
        out = []
        for s, seg in enumerate(self.series()):
            value, shift, bin_ = ffa_oracle.segment_records(seg, n_oct, p_lo, p_hi, n_widths)
            ssum, ssq = ffa_oracle.segment_stats(seg)
            first_row = self.t_offset + s * n_seg * tdec
            out.append({"value": value, "shift": shift, "bin": bin_, "sum": ssum, "sumsq": ssq, "first_row": first_row, "n_rows": n_seg * tdec,
                        "cands": ffa_oracle.select(value, shift, bin_, ssum, ssq, tdec, n_seg, p_lo, first_row, self.dm_first, self.threshold)})
        return out


def mutant_changes(x, tdec, n_seg, blk, win, mutant):
    """Per segment of x: (bool [n_seg] -- the sample positions at which the mutant's y' has other bits than the contract's in any
    column, fraction of all samples changed)."""
    a = Search(x, tdec, n_seg, 1, 8, 9, 1, blk, win).series()
    b = Search(x, tdec, n_seg, 1, 8, 9, 1, blk, win, mutant=mutant).series()
    out = []
    for s, t in zip(a, b):
        diff = s.view(np.uint32) != t.view(np.uint32)
        out.append((diff.any(axis=(0, 2)), float(diff.mean())))
    return out


def sift(cands, tol, max_harm, dm_tol):
    """bf_ffa_sift, operation for operation: cands a list of ffa_oracle.CAND_FIELDS tuples (or a CAND_DTYPE array).  Returns a list
    of dicts {head (index into cands), n_members, n_beams, dm_lo, dm_hi, n_harmonic}, in creation order."""
    F = {f: i for i, f in enumerate(ffa_oracle.CAND_FIELDS)}
    rows = [tuple(c[f] for f in ffa_oracle.CAND_FIELDS) if isinstance(c, np.void) else tuple(c) for c in cands]
    order = sorted(range(len(rows)), key=lambda i: (-float(rows[i][F["snr"]]), i))
    groups = []
    for i in order:
        c = rows[i]
        period, dm = float(c[F["period_rows"]]), int(c[F["dm"]])
        hit = None
        for g in groups:
            hd = rows[g["head"]]
            if int(c[F["first_row"]]) != int(hd[F["first_row"]]) or int(c[F["n_rows"]]) != int(hd[F["n_rows"]]):
                continue
            if abs(dm - int(hd[F["dm"]])) > dm_tol:
                continue
            for a in range(1, max_harm + 1):
                for b in range(1, max_harm + 1):
                    if math.fabs((period * float(b)) / (float(hd[F["period_rows"]]) * float(a)) - 1.0) <= tol:
                        hit = (a, b)
                        break
                if hit:
                    break
            if hit:
                g["n_members"] += 1
                g["beams"].add(int(c[F["beam"]]))
                g["dm_lo"], g["dm_hi"] = min(g["dm_lo"], dm), max(g["dm_hi"], dm)
                g["n_harmonic"] += hit != (1, 1)
                break
        if hit is None:
            groups.append({"head": i, "n_members": 1, "beams": {int(c[F["beam"]])}, "dm_lo": dm, "dm_hi": dm, "n_harmonic": 0})
    for g in groups:
        g["n_beams"] = len(g.pop("beams"))
    return groups
