"""The full-Stokes follow-up beams restated in numpy (docs/STOKES.md section 1): exact int64, so every comparison with the device is
np.array_equal.  Written from the contract, not from the kernel: a 256-entry nibble table, an int64 einsum and a reshape-sum."""
from collections import namedtuple

import numpy as np

_N = np.arange(256)
RE = np.where((_N >> 4) >= 8, (_N >> 4) - 16, _N >> 4).astype(np.int64)      # high nibble, two's complement
IM = np.where((_N & 15) >= 8, (_N & 15) - 16, _N & 15).astype(np.int64)      # low nibble

Geometry = namedtuple("Geometry", "n_ant n_freq n_out_per_gemm n_avg n_beams")   # n_pol is 2


def geometry(cfg):
    assert cfg.n_pol == 2
    return Geometry(cfg.n_ant, cfg.n_freq, cfg.n_out_per_gemm, cfg.n_avg, cfg.n_beams)


# The hand-computed case: 4 antennas, one channel, one sample (columns X, Y), one beam.
#   X column 0x12 0xF0 0x7F 0x88 = (1, 2) (-1, 0) (7, -1) (-8, -8)      Y column 0x31 0x0E 0xC4 0x50 = (3, 1) (0, -2) (-4, 4) (5, 0)
#   weights (1, 0) (0, 1) (-128, 127) (2, -3)
#   X = (1 + 2i) + (-1)(i) + (7 - i)(-128 + 127i) + (-8 - 8i)(2 - 3i) = (1, 2) + (0, -1) + (-769, 1017) + (-40, 8) = (-808, 1026)
#   Y = (3 + i) + (-2i)(i) + (-4 + 4i)(-128 + 127i) + 5 (2 - 3i)     = (3, 1) + (2, 0) + (4, -1020) + (10, -15) = (19, -1034)
#   |X|^2 = 652864 + 1052676 = 1705540      |Y|^2 = 361 + 1069156 = 1069517
#   I = 2775057   Q = 636023   U = 2 (-808 * 19 + 1026 * -1034) = 2 (-15352 - 1060884) = -2152472
#   V = 2 (1026 * 19 - (-808)(-1034)) = 2 (19494 - 835472) = -1631956
KNOWN_PACKED = np.array([[0x12, 0xF0, 0x7F, 0x88], [0x31, 0x0E, 0xC4, 0x50]], np.uint8).reshape(1, 1, 2, 4)
KNOWN_WEIGHTS = np.array([[1, 0], [0, 1], [-128, 127], [2, -3]], np.int8).reshape(1, 4, 1, 2)
KNOWN_GEOMETRY = Geometry(4, 1, 1, 1, 1)
KNOWN = (2775057, 636023, -2152472, -1631956)


def beam_samples(packed, w, beams):
    """packed uint8 [unit][freq][column][ant], w int8 [freq][ant][beam][2], beams: indices -> (re, im), int64 [unit][freq][column][k]:
    n = sum over a of v * w, no conjugation."""
    packed = np.asarray(packed, np.uint8)
    sel = np.asarray(w, np.int8)[:, :, list(beams), :].astype(np.int64)       # [f][a][k][2]
    vr, vi = RE[packed], IM[packed]                                            # [u][f][c][a]
    wr, wi = sel[..., 0], sel[..., 1]
    re = np.einsum("ufca,fak->ufck", vr, wr) - np.einsum("ufca,fak->ufck", vi, wi)
    im = np.einsum("ufca,fak->ufck", vi, wr) + np.einsum("ufca,fak->ufck", vr, wi)
    return re, im


def stokes(packed, w, beams, n_int, geom):
    """int64 [unit][t][freq][k][4] = {I, Q, U, V} summed over windows of n_int samples; sample j is the column pair (2j, 2j + 1)."""
    S = geom.n_out_per_gemm * geom.n_avg
    assert n_int >= 1 and S % n_int == 0
    packed = np.asarray(packed, np.uint8).reshape(-1, geom.n_freq, 2 * S, geom.n_ant)
    re, im = beam_samples(packed, w, beams)
    xr, yr, xi, yi = re[:, :, 0::2], re[:, :, 1::2], im[:, :, 0::2], im[:, :, 1::2]   # [u][f][j][k]
    px, py = xr * xr + xi * xi, yr * yr + yi * yi
    iquv = np.stack([px + py, px - py, 2 * (xr * yr + xi * yi), 2 * (xi * yr - xr * yi)], axis=-1)   # [u][f][j][k][4]
    u, f, _, k, _ = iquv.shape
    return iquv.reshape(u, f, S // n_int, n_int, k, 4).sum(axis=3).transpose(0, 2, 1, 3, 4).copy()


def pack(re, im):
    """Integer arrays -8 ... 7 -> packed bytes, re in the high nibble."""
    return (((np.asarray(re) & 15) << 4) | (np.asarray(im) & 15)).astype(np.uint8)


def scene(seed, geom, n_units=1, relation="random"):
    """Voltages -7 ... 7 (so that i * v is representable) and weights over all of int8.  relation: "random" (Y independent of X),
    "equal" (Y = X: Q = V = 0, U = I) or "quarter" (Y = i X: Q = U = 0, V = -I).  Returns (packed [unit][freq][2 S][ant], w)."""
    rng = np.random.default_rng(seed)
    S = geom.n_out_per_gemm * geom.n_avg
    shape = (n_units, geom.n_freq, S, geom.n_ant)
    xr, xi = rng.integers(-7, 8, size=shape), rng.integers(-7, 8, size=shape)
    if relation == "equal":
        yr, yi = xr, xi
    elif relation == "quarter":
        yr, yi = -xi, xr                                                       # i (xr + i xi)
    else:
        yr, yi = rng.integers(-7, 8, size=shape), rng.integers(-7, 8, size=shape)
    packed = np.empty((n_units, geom.n_freq, 2 * S, geom.n_ant), np.uint8)
    packed[:, :, 0::2], packed[:, :, 1::2] = pack(xr, xi), pack(yr, yi)
    w = rng.integers(-128, 128, size=(geom.n_freq, geom.n_ant, geom.n_beams, 2), dtype=np.int8)
    return packed, w


def write_stokes_file(path, geom, first_channel, beams, n_int, records, n_gemms_per_block=4):
    """A file in the format `beam -x` writes (docs/STOKES.md section 4), by hand: records = [(first_unit, int64 [n_units][T][f][k][4])]."""
    head = ("HDR_VERSION 1.0\nHDR_SIZE 4096\nINSTRUMENT DSA\nCONTENT stokes\nDTYPE int64\nENDIAN little\nLAYOUT unit,time,freq,beam,iquv\n"
            "RECORD_HEADER_BYTES 16\nNANT %d\nNPOL 2\nNFREQ %d\nFIRST_CHANNEL %d\nN_OUTPUTS_PER_GEMM %d\nN_GEMMS_PER_BLOCK %d\nN_AVERAGING %d\n"
            "NINT %d\nNSEL %d\nBEAMS %s\nGPU 0\n" % (geom.n_ant, geom.n_freq, first_channel, geom.n_out_per_gemm, n_gemms_per_block, geom.n_avg,
                                                    n_int, len(beams), ",".join(str(b) for b in beams))).encode()
    with open(path, "wb") as f:
        f.write(head + b"\0" * (4096 - len(head)))
        for first_unit, data in records:
            f.write(np.array([first_unit, data.shape[0]], "<u8").tobytes())
            f.write(np.ascontiguousarray(data, "<i8").tobytes())
