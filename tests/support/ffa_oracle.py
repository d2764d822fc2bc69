"""numpy restatement of the periodicity search (docs/PERIODICITY.md section 1): decimation, segments, octaves, the Fast Folding
Algorithm's merges, the circular boxcars, the peak records, the statistics and the candidate selection -- over a WHOLE series,
however the stage is given it.  No GPU, no libdsabf.  Series are [n_dm][T][n_beams] float32, like the DM stage's chunks."""
from __future__ import annotations

import math

import numpy as np

CAND_FIELDS = ("first_row", "n_rows", "period_rows", "dm", "beam", "octave", "p", "shift", "bin", "width", "snr", "value")
# bf_ffa_candidate (include/dsabf.h), as the C compiler lays it out
CAND_DTYPE = np.dtype([("first_row", np.uint64), ("n_rows", np.uint64), ("period_rows", np.float64), ("dm", np.int32), ("beam", np.int32),
                       ("octave", np.int32), ("p", np.int32), ("shift", np.int32), ("bin", np.int32), ("width", np.int32), ("snr", np.float64),
                       ("value", np.float32)], align=True)
PEAK_DTYPE = np.dtype([("value", np.float32), ("shift", np.uint16), ("bin", np.uint16)])
STAT_DTYPE = np.dtype([("sum", np.float64), ("sumsq", np.float64)])


def parity_input(seed, n_dm, n_t, n_beams):
    """N(0,1) * 2^e, e uniform in -20 .. 20: sums whose bits depend on the association of the adds."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-20, 21, size=(n_dm, n_t, n_beams))
    return (rng.standard_normal((n_dm, n_t, n_beams)) * np.exp2(e)).astype(np.float32)


def rows_of(length, p):
    """M: the largest power of two <= length // p (0: none)."""
    q = length // p if p > 0 else 0
    return 0 if q < 1 else 1 << (q.bit_length() - 1)


def decimate(x, tdec):
    """y[u] = ((x[u tdec] + x[u tdec + 1]) + ...) + x[u tdec + tdec - 1], fp32, the first term as it is; whole groups only."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[1] // tdec
    g = x[:, :n * tdec].reshape(x.shape[0], n, tdec, x.shape[2])
    y = g[:, :, 0].copy()
    for i in range(1, tdec):
        y = y + g[:, :, i]
    return y


def octaves(seg, n_oct):
    """[y_0, y_1, ...]: y_{o+1}[u] = y_o[2u] + y_o[2u + 1], fp32."""
    out = [np.ascontiguousarray(seg, np.float32)]
    for _ in range(1, n_oct):
        y = out[-1]
        assert y.shape[1] % 2 == 0
        out.append(y[:, 0::2] + y[:, 1::2])
    return out


def fold(y, p):
    """The M profiles of an octave y [n_dm][L][n_beams] at base period p: [n_dm][M][p][n_beams], by the contract's merges."""
    M = rows_of(y.shape[1], p)
    assert M >= 2
    cur = y[:, :M * p].reshape(y.shape[0], M, p, y.shape[2]).copy()
    g = 1
    while g < M:
        out = np.empty_like(cur)
        for base in range(0, M, 2 * g):
            for i in range(2 * g):
                a = cur[:, base + (i >> 1)]
                b = cur[:, base + g + (i >> 1)]
                out[:, base + i] = a + np.roll(b, -(((i + 1) >> 1) % p), axis=1)   # A's term is the left operand
        cur, g = out, 2 * g
    return cur


def fold_indices(M, p):
    """For every final row i and bin j, the sample indices (into the octave) the recursion adds, in the order of its operand
    tree: idx [M][p][M] (entry r comes from row r)."""
    cur = (np.arange(M)[:, None] * p + np.arange(p)[None, :])[:, :, None]
    g = 1
    while g < M:
        out = np.empty((M, p, 2 * g), np.int64)
        for base in range(0, M, 2 * g):
            for i in range(2 * g):
                a = cur[base + (i >> 1)]
                b = np.roll(cur[base + g + (i >> 1)], -(((i + 1) >> 1) % p), axis=0)
                out[base + i] = np.concatenate([a, b], axis=1)
        cur, g = out, 2 * g
    return cur


def row_shifts(M):
    """shift[i][r]: how far row r is rotated in final row i (before the reduction mod p)."""
    cur = [[0] for _ in range(M)]
    g = 1
    while g < M:
        out = [None] * M
        for base in range(0, M, 2 * g):
            for i in range(2 * g):
                s = (i + 1) >> 1
                out[base + i] = cur[base + (i >> 1)] + [v + s for v in cur[base + g + (i >> 1)]]
        cur, g = out, 2 * g
    return np.asarray(cur, np.int64)


def fold_left(y, p):
    """The same cells summed left to right over the same samples (row 0 first), fp32: another association, NOT the contract."""
    M = rows_of(y.shape[1], p)
    idx = fold_indices(M, p)
    acc = y[:, idx[:, :, 0]].copy()
    for r in range(1, M):
        acc = acc + y[:, idx[:, :, r]]
    return acc


def boxcars(prof, n_widths):
    """[C_0, C_1, ...] of profiles [n_dm][M][p][n_beams]: C_k[j] = C_{k-1}[j] + C_{k-1}[(j + 2^(k-1)) mod p], fp32."""
    out = [prof]
    for k in range(1, n_widths):
        c = out[-1]
        out.append(c + np.roll(c, -(1 << (k - 1)), axis=2))
    return out


def peak_of(c):
    """value, shift, bin [n_dm][n_beams] of C [n_dm][M][p][n_beams]: the maximum, the smallest row attaining it, the smallest bin there."""
    n_dm, M, p, nb = c.shape
    flat = c.reshape(n_dm, M * p, nb)
    arg = np.argmax(flat, axis=1)                      # first occurrence in (i, j) order
    val = np.take_along_axis(flat, arg[:, None, :], axis=1)[:, 0, :]
    return val, (arg // p).astype(np.uint16), (arg % p).astype(np.uint16)


def segment_records(seg, n_oct, p_lo, p_hi, n_widths, fold_fn=fold):
    """Records of one segment seg [n_dm][n_seg][n_beams] (decimated): value float32, shift, bin uint16 [n_oct][n_p][K][n_dm][n_beams]."""
    n_dm, _, nb = seg.shape
    shape = (n_oct, p_hi - p_lo, n_widths, n_dm, nb)
    value, shift, bin_ = np.empty(shape, np.float32), np.empty(shape, np.uint16), np.empty(shape, np.uint16)
    for o, y in enumerate(octaves(seg, n_oct)):
        for p in range(p_lo, p_hi):
            for k, c in enumerate(boxcars(fold_fn(y, p), n_widths)):
                value[o, p - p_lo, k], shift[o, p - p_lo, k], bin_[o, p - p_lo, k] = peak_of(c)
    return value, shift, bin_


def segment_stats(seg):
    """sum and sum of squares over time, [n_dm][n_beams] float64, EXACTLY summed and rounded once (math.fsum; the square of an
    fp32 is exact in fp64): the parity inputs cancel, and a plain fp64 sum is only good to n 2^-53 of the sum of magnitudes."""
    s = np.asarray(seg, np.float64)
    n_dm, _, nb = s.shape
    ssum, ssq = np.empty((n_dm, nb)), np.empty((n_dm, nb))
    for d in range(n_dm):
        cols, sq = s[d].T.tolist(), (s[d] * s[d]).T.tolist()
        ssum[d] = [math.fsum(c) for c in cols]
        ssq[d] = [math.fsum(c) for c in sq]
    return ssum, ssq


def select(value, shift, bin_, ssum, ssumsq, tdec, n_seg, p_lo, first_row=0, dm_first=0, threshold=8.0):
    """bf_ffa_select, operation for operation in fp64: list of CAND_FIELDS tuples in (d, b) order."""
    n_oct, n_p, n_widths, n_dm, n_beams = value.shape
    out = []
    for d in range(n_dm):
        for b in range(n_beams):
            mu = float(ssum[d, b]) / float(n_seg)
            var = float(ssumsq[d, b]) / float(n_seg) - mu * mu
            sigma = math.sqrt(var if var > 0.0 else 0.0)
            if sigma == 0.0:
                continue
            have, best, key = False, 0.0, None
            for o in range(n_oct):
                o2 = float(1 << o)
                mu_o, sigma_o = o2 * mu, sigma * math.sqrt(o2)
                for pi in range(n_p):
                    M = rows_of(n_seg >> o, p_lo + pi)
                    for k in range(n_widths):
                        wM = float(1 << k) * float(M)
                        snr = (float(value[o, pi, k, d, b]) - wM * mu_o) / (sigma_o * math.sqrt(wM))
                        if not have or snr > best:
                            have, best, key = True, snr, (o, pi, k, M)
            if not have or not best >= threshold:
                continue
            o, pi, k, M = key
            sh = int(shift[o, pi, k, d, b])
            period = (float(tdec) * float(1 << o)) * (float(p_lo + pi) + float(sh) / float(M - 1))
            out.append((int(first_row), n_seg * tdec, period, dm_first + d, b, o, p_lo + pi, sh, int(bin_[o, pi, k, d, b]), 1 << k, best,
                        float(value[o, pi, k, d, b])))
    return out


class Search:
    """The stage over a whole series x [n_dm][T][n_beams] (row 0 = the first sample the stage is given): segments() lists, per
    complete segment, the records, the statistics and the candidates bf_ffa_collect must give."""

    def __init__(self, x, tdec, n_seg, n_oct, p_lo, p_hi, n_widths, dm_first=0, threshold=8.0, t_offset=0, fold_fn=fold):
        self.y = decimate(x, tdec)
        self.cfg = (tdec, n_seg, n_oct, p_lo, p_hi, n_widths)
        self.dm_first, self.threshold, self.t_offset, self.fold_fn = dm_first, threshold, t_offset, fold_fn

    def segments(self):
        tdec, n_seg, n_oct, p_lo, p_hi, n_widths = self.cfg
        out = []
        for s in range(self.y.shape[1] // n_seg):
            seg = self.y[:, s * n_seg:(s + 1) * n_seg]
            value, shift, bin_ = segment_records(seg, n_oct, p_lo, p_hi, n_widths, self.fold_fn)
            ssum, ssq = segment_stats(seg)
            first_row = self.t_offset + s * n_seg * tdec
            out.append({"value": value, "shift": shift, "bin": bin_, "sum": ssum, "sumsq": ssq, "first_row": first_row, "n_rows": n_seg * tdec,
                        "cands": select(value, shift, bin_, ssum, ssq, tdec, n_seg, p_lo, first_row, self.dm_first, self.threshold)})
        return out


def association_matters(x, tdec, n_seg, n_oct, p_lo, p_hi, n_widths):
    """True if a left-to-right restatement of the fold gives other record bits than the contract on this input: the input can tell a
    wrongly associated kernel from a right one."""
    a = Search(x, tdec, n_seg, n_oct, p_lo, p_hi, n_widths).segments()
    b = Search(x, tdec, n_seg, n_oct, p_lo, p_hi, n_widths, fold_fn=fold_left).segments()
    return any(not np.array_equal(s["value"].view(np.uint32), t["value"].view(np.uint32)) for s, t in zip(a, b))


def assert_candidates_equal(got, want):
    """got: CAND_DTYPE array from the library; want: list of tuples from select().  Everything bit for bit."""
    assert len(got) == len(want), (len(got), len(want))
    if not len(want):
        return
    w = list(zip(*want))
    for i, f in enumerate(CAND_FIELDS):
        if f in ("period_rows", "snr"):
            assert np.array_equal(np.asarray(got[f], np.float64).view(np.uint64), np.asarray(w[i], np.float64).view(np.uint64)), f
        elif f == "value":
            assert np.array_equal(np.asarray(got[f], np.float32).view(np.uint32), np.asarray(w[i], np.float32).view(np.uint32)), f
        else:
            assert np.array_equal(np.asarray(got[f], np.int64), np.asarray(w[i], np.int64)), f


def read_candidates(path):
    """The text file of `beam --ffa-out` / bfh_ffa_sink: '#' header lines, then one line per candidate in CAND_FIELDS order.
    Returns (header dict of the 'key=value' words, list of tuples)."""
    head, rows = {}, []
    for line in open(path):
        line = line.strip()
        if not line:
            continue
        if line.startswith("#"):
            for word in line[1:].split():
                if "=" in word:
                    k, v = word.split("=", 1)
                    head[k] = v
            continue
        f = line.split()
        assert len(f) == len(CAND_FIELDS), line
        rows.append((int(f[0]), int(f[1]), float(f[2])) + tuple(int(v) for v in f[3:10]) + (float(f[10]), float(np.float32(f[11]))))
    return head, rows
