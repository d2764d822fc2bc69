"""Reference of the voltage cut (include/dsabf.h: bf_vhist_cut; docs/VOLTAGE_CUTS.md section 1): the contract's formula as numpy fancy
indexing over the WHOLE pushed series, the status rule, and a writer of the voltage file.  No arithmetic: bytes are moved.

units: uint8 [unit][freq][S][B] -- every unit ever pushed, B = n_pol * n_ant bytes per sample.
delays: int32 [n_dm][n_freq], samples.  requests: (t0 in samples, row of delays)."""
import struct

import numpy as np

SENTINEL = 0xA5


def series_of(units):
    """[unit][freq][S][B] -> the series [sample][freq][B]."""
    n_u, n_f, S, B = units.shape
    return np.ascontiguousarray(units.transpose(0, 2, 1, 3)).reshape(n_u * S, n_f, B)


def span(delays, dm, n_units_out, S):
    """Samples request (t0, dm) needs from t0 on."""
    return n_units_out * S + int(np.max(delays[dm]))


def status(delays, t0, dm, n_units_out, S, oldest_unit, next_unit):
    """0 cut; 1 a sample lies in a unit older than oldest_unit; 2 a sample is not pushed yet; 1 where both hold."""
    if t0 < oldest_unit * S:
        return 1
    return 2 if t0 + span(delays, dm, n_units_out, S) > next_unit * S else 0


def window(units, delays, t0, dm, n_units_out, series=None):
    """out[u][f][j][:] = v[t0 + u S + j + delays[dm][f]][f][:] as uint8 [n_units_out][freq][S][B] (series: series_of(units), if at hand)."""
    n_u, n_f, S, B = units.shape
    v = series_of(units) if series is None else series
    t = int(t0) + np.arange(n_units_out * S, dtype=np.int64)[:, None] + np.asarray(delays[dm], np.int64)[None, :]   # [time][freq]
    got = v[t, np.arange(n_f)[None, :]]                                                                             # [time][freq][B]
    return np.ascontiguousarray(got.reshape(n_units_out, S, n_f, B).transpose(0, 2, 1, 3))


def cut(units, delays, requests, n_units_out, oldest_unit, next_unit):
    """(out uint8 [n_req][n_units_out][freq][S][B] with SENTINEL bytes where nothing is written, status int32 [n_req])."""
    n_u, n_f, S, B = units.shape
    out = np.full((len(requests), n_units_out, n_f, S, B), SENTINEL, np.uint8)
    st = np.zeros(len(requests), np.int32)
    v = series_of(units[:next_unit])
    for r, (t0, dm) in enumerate(requests):
        st[r] = status(delays, int(t0), int(dm), n_units_out, S, oldest_unit, next_unit)
        if st[r] == 0:
            out[r] = window(units[:next_unit], delays, t0, dm, n_units_out, v)
    return out, st


def window_by_loop(units, delays, t0, dm, n_units_out, cap_units):
    """The same window byte by byte THROUGH A RING of cap_units physical units, as the contract places the samples: sample s lies in
    physical unit (s / S) mod cap_units at sample s % S.  The ring holds the newest cap_units units of `units`."""
    n_u, n_f, S, B = units.shape
    ring = np.zeros((cap_units, n_f, S, B), np.uint8)
    for u in range(n_u):
        ring[u % cap_units] = units[u]
    out = np.zeros((n_units_out, n_f, S, B), np.uint8)
    for u in range(n_units_out):
        for f in range(n_f):
            for j in range(S):
                s = int(t0) + u * S + j + int(delays[dm][f])
                for b in range(B):
                    out[u, f, j, b] = ring[(s // S) % cap_units, f, s % S, b]
    return out


HEADER_BYTES = 4096
RECORD = struct.Struct("<Qiiid")   # uint64 t0; int32 dm, beam, width; double snr


def write_file(path, n_ant, n_freq, n_pol, n_avg, n_out, units, first_channel, records):
    """The voltage file: the project's 4096-byte text header, then per cut the record and its bytes.
    records: (t0, dm, beam, width, snr, data uint8 [units][freq][S][n_pol n_ant])."""
    hdr = ("HDR_SIZE 4096\nCONTENT voltages\nDTYPE packed4+4\nNANT %d\nNFREQ %d\nNPOL %d\nNAVG %d\nNOUT %d\nUNITS %d\nFIRST_CHANNEL %d\n"
           "LAYOUT unit,freq,time,pol,ant\nRECORD_HEADER_BYTES 28\n" % (n_ant, n_freq, n_pol, n_avg, n_out, units, first_channel)).encode()
    with open(path, "wb") as fp:
        fp.write(hdr + b"\0" * (HEADER_BYTES - len(hdr)))
        for t0, dm, beam, width, snr, data in records:
            fp.write(RECORD.pack(int(t0), int(dm), int(beam), int(width), float(snr)))
            fp.write(np.ascontiguousarray(data, np.uint8).tobytes())
