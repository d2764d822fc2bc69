"""The incoherent beam restated in numpy (docs/INCOHERENT_BEAM.md; include/dsabf.h: bf_incoherent_device): per packed byte
re^2 + im^2 of its two's-complement nibbles (high = re, low = im) from a 256-entry table, summed over the n_ipo * n_ant bytes of every
output window.  Integers throughout, so the float32 result is exact wherever 128 * n_ant * n_ipo <= 2^24 -- the bound the feature
is defined for -- and the device has to match it bit for bit."""
from __future__ import annotations

import numpy as np


def _nibble(v: int) -> int:
    return v - 16 if v >= 8 else v


TABLE = np.array([_nibble(b >> 4) ** 2 + _nibble(b & 15) ** 2 for b in range(256)], np.int64)

_TABLE8 = TABLE.astype(np.uint8)      # (at most 128: the lookup of a large input stays one byte per sample)

KNOWN_BYTES, KNOWN_SUM = bytes([0xD7, 0x25, 0xA8, 0x70]), 236   # 58 + 29 + 100 + 49


def supported(n_ant: int, n_ipo: int) -> bool:
    return 128 * n_ant * n_ipo <= 2 ** 24


def incoherent(packed, n_out: int, n_ipo: int) -> np.ndarray:
    """packed uint8 [unit][freq][n_out * n_ipo][ant] -> float32 [unit][n_out][freq]."""
    p = np.asarray(packed, np.uint8)
    n_units, n_freq, n_time, n_ant = p.shape
    assert n_time == n_out * n_ipo and supported(n_ant, n_ipo)
    s = _TABLE8[p].reshape(n_units, n_freq, n_out, n_ipo * n_ant).sum(axis=3, dtype=np.int64)     # [unit][freq][o]
    return np.ascontiguousarray(s.transpose(0, 2, 1)).astype(np.float32)


def with_column(detected, packed, beam: int, n_ipo: int) -> np.ndarray:
    """A copy of the detected powers [unit][o][freq][beam] with beam column `beam` replaced by the incoherent beam of `packed`."""
    d = np.array(detected, np.float32, copy=True)
    d[..., beam] = incoherent(packed, d.shape[1], n_ipo)
    return d


def dm0_row(column) -> np.ndarray:
    """The DM-0 collapse of one beam column [.. ][freq] of output 0: the ascending-f sum, one float32 add after the other."""
    c = np.asarray(column, np.float32)
    acc = np.zeros(c.shape[:-1], np.float32)
    for f in range(c.shape[-1]):
        acc = (acc + c[..., f]).astype(np.float32)
    return acc
