"""numpy restatement of the pulsar fold's contract (docs/PULSAR_FOLDING.md section 1; include/dsabf.h: bf_psr_*): the fixed-point
phase model and its bins, the fold (every cell summed in ascending row order, fp64, one rounding per add), bf_psr_model_from_spin
and bf_psr_beam_snr operation for operation, and a reader of psr_file_sink's file.  Integers wrap modulo 2^64 as uint64 ARRAYS do in
numpy; nothing here reads the library."""
import math
import struct

import numpy as np

M64 = (1 << 64) - 1
HEADER_BYTES = 4096
RECORD_HEADER = struct.Struct("<QQIIII")     # first_row, n_rows, n_psr, n_freq, n_bins, n_beams


def _frac_u64(x):
    fr = x - math.floor(x)
    return 0 if fr >= 1.0 else int(math.ldexp(fr, 64))


def model_from_spin(f0_hz, f1_hz_s, phase0_turns, row_seconds, epoch_row=0):
    """(phase0, dphase, ddphase, epoch_row) as Python ints (ddphase signed), or None where the library refuses."""
    args = (f0_hz, f1_hz_s, phase0_turns, row_seconds)
    if not all(math.isfinite(v) for v in args) or not row_seconds > 0.0:
        return None
    x = f0_hz * row_seconds
    dd = math.ldexp((f1_hz_s * row_seconds) * row_seconds, 64)
    dd = float(round(dd)) if abs(dd) < 2.0 ** 53 else dd      # nearbyint: half to even; beyond 2^53 every double is an integer
    if not abs(dd) < 2.0 ** 62:
        return None
    ddphase = int(dd)
    dphase = (_frac_u64(x) + ((ddphase >> 1) & M64)) & M64
    return (_frac_u64(phase0_turns), dphase, ddphase, int(epoch_row))


def phases(model, delays_k, first_row, n_rows):
    """uint64 [n_rows][n_freq]: the phase of every (row, channel) of rows first_row .. first_row + n_rows - 1 for one pulsar."""
    phase0, dphase, ddphase, epoch = model
    r = np.arange(first_row, first_row + n_rows, dtype=np.int64)[:, None]
    n = r - np.int64(epoch) - np.asarray(delays_k, np.int64)[None, :]
    assert np.all(np.abs(n) < 2 ** 31)
    tri = n * (n - 1) // 2
    one = np.ones_like(n, dtype=np.uint64)
    return one * np.uint64(phase0) + n.astype(np.uint64) * np.uint64(dphase) + tri.astype(np.uint64) * np.uint64(ddphase & M64)


def bins(model, delays_k, first_row, n_rows, n_bins):
    """int64 [n_rows][n_freq]: bin = ((phase >> 32) * n_bins) >> 32."""
    ph = phases(model, delays_k, first_row, n_rows)
    return (((ph >> np.uint64(32)) * np.uint64(n_bins)) >> np.uint64(32)).astype(np.int64)


def fold(x, models, delays, n_bins, first_row=0, reverse=False):
    """x float32 [n_rows][n_freq][n_beams], rows first_row .. of the series -> (profile float64 [n_psr][f][bin][beam], hits uint64
    [n_psr][f][bin]) of ONE integration: every cell the left fold acc = acc + (double)x over its rows in ascending row order from
    +0.0 (reverse=True: descending -- what the tests use to show that their input makes the order matter)."""
    x = np.asarray(x, np.float32)
    n_rows, n_f, n_b = x.shape
    delays = np.asarray(delays, np.int32).reshape(len(models), n_f)
    prof = np.zeros((len(models), n_f, n_bins, n_b), np.float64)
    hits = np.zeros((len(models), n_f, n_bins), np.uint64)
    chan = np.arange(n_f)
    for k, m in enumerate(models):
        bk = bins(m, delays[k], first_row, n_rows, n_bins)
        for r in (range(n_rows - 1, -1, -1) if reverse else range(n_rows)):
            prof[k, chan, bk[r]] = prof[k, chan, bk[r]] + x[r].astype(np.float64)     # (channel, its bin): distinct cells, one add each
            hits[k, chan, bk[r]] += np.uint64(1)
    return prof, hits


def _median(v):
    s = np.sort(v)
    n = len(s)
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) * 0.5


def beam_snr(profile_k, hits_k, chan_mask=None):
    """(snr float64 [n_beams], peak_bin int32 [n_beams]) of one pulsar's profile [f][bin][beam] and hits [f][bin]."""
    p = np.asarray(profile_k, np.float64)
    h = np.asarray(hits_k, np.uint64)
    n_f, n_bins, n_b = p.shape
    keep = [f for f in range(n_f) if chan_mask is None or not chan_mask[f]]
    H = np.zeros(n_bins, np.uint64)
    S = np.zeros((n_bins, n_b), np.float64)
    for f in keep:
        H = H + h[f]
        S = S + p[f]
    live = np.flatnonzero(H > 0)
    snr, peak = np.zeros(n_b, np.float64), np.full(n_b, -1, np.int32)
    if len(live) < 4:
        return snr, peak
    for b in range(n_b):
        m = S[live, b] / H[live].astype(np.float64)
        best = 0
        for i in range(1, len(m)):
            if m[i] > m[best]:
                best = i
        med = _median(m)
        sigma = 1.4826 * _median(np.abs(m - med))
        if not sigma > 0.0:
            continue
        snr[b] = (m[best] - med) / sigma
        peak[b] = live[best]
    return snr, peak


def read_file(path):
    """psr_file_sink's file -> (header dict of its `KEY value` lines, list of records dict(first_row, n_rows, hits, profile))."""
    raw = open(path, "rb").read()
    assert len(raw) >= HEADER_BYTES
    header = {}
    for line in raw[:HEADER_BYTES].split(b"\0", 1)[0].decode().splitlines():
        key, _, value = line.partition(" ")
        header[key] = value
    recs, at = [], HEADER_BYTES
    while at < len(raw):
        first_row, n_rows, n_psr, n_f, n_bins, n_b = RECORD_HEADER.unpack_from(raw, at)
        at += RECORD_HEADER.size
        n_h = n_psr * n_f * n_bins
        hits = np.frombuffer(raw, "<u8", n_h, at).reshape(n_psr, n_f, n_bins)
        at += 8 * n_h
        prof = np.frombuffer(raw, "<f8", n_h * n_b, at).reshape(n_psr, n_f, n_bins, n_b)
        at += 8 * n_h * n_b
        recs.append(dict(first_row=first_row, n_rows=n_rows, hits=hits, profile=prof))
    assert at == len(raw)
    return header, recs
