"""The correlator's reference (docs/CORRELATOR.md): a nibble table and an int64 einsum.

    V[f][p][a1][a2] = sum over the units and the columns c = p (mod n_pol) of v[u][f][c][a1] * conj(v[u][f][c][a2]),   a2 <= a1

on the packed voltages uint8 [unit][freq][time][ant] (high nibble re, low nibble im, two's complement), stored as the packed lower
triangle [freq][pol][bl][2] (re, im), bl = a1 (a1 + 1) / 2 + a2, int64.  Every sum is an exact integer, so the device result is
compared with np.array_equal.
"""
import numpy as np

_n = np.arange(256, dtype=np.int64)
_sx = lambda v: np.where(v & 8, v - 16, v)   # noqa: E731
RE, IM = _sx(_n >> 4), _sx(_n & 15)          # signed nibbles of every byte code

MAX_ANT = 256
MAX_COLUMNS = 2 ** 24 - 1                    # 128 * N <= 2^31 - 1


def bl(a1, a2):
    """The triangular index of (a1, a2), a2 <= a1."""
    return a1 * (a1 + 1) // 2 + a2


def n_baselines(n_ant):
    return n_ant * (n_ant + 1) // 2


def supported(n_ant, columns_per_pol):
    return 0 < n_ant <= MAX_ANT and n_ant % 4 == 0 and 0 < columns_per_pol <= MAX_COLUMNS


def _square(packed, n_pol, dtype):
    """re, im of V as full squares [f][p][a1][a2], computed in `dtype`."""
    packed = np.asarray(packed)
    n_u, n_f, n_t, n_a = packed.shape
    assert packed.dtype == np.uint8 and n_t % n_pol == 0
    shape = (n_u, n_f, n_t // n_pol, n_pol, n_a)                 # time = column * n_pol + polarisation: polarisation fastest
    r, m = RE[packed].reshape(shape).astype(dtype), IM[packed].reshape(shape).astype(dtype)
    if dtype == np.int64:
        prod = lambda x, y: np.einsum("ufcpa,ufcpb->fpab", x, y)   # noqa: E731
    else:                                                         # (u, c) -> one K axis, one matrix product per (f, p)
        xs = lambda x: x.transpose(1, 3, 0, 2, 4).reshape(n_f, n_pol, -1, n_a)   # noqa: E731
        prod = lambda x, y: np.matmul(xs(x).transpose(0, 1, 3, 2), xs(y))   # noqa: E731
    return prod(r, r) + prod(m, m), prod(m, r) - prod(r, m)


def _triangle(re, im):
    a1, a2 = np.tril_indices(re.shape[-1])                         # row-major over the lower triangle: bl order
    return np.stack([re[..., a1, a2], im[..., a1, a2]], axis=-1).astype(np.int64)


def visibilities(packed, n_pol):
    """The restatement: int64 [freq][pol][bl][2]."""
    return _triangle(*_square(packed, n_pol, np.int64))


def visibilities_f64(packed, n_pol):
    """The same numbers through float64 matrix products (BLAS): every product and partial sum is an integer below 128 * N < 2^53,
    so float64 arithmetic is exact and the result equals `visibilities` to the bit -- tests/test_corr_cpu.py holds the two together.
    For inputs of hundreds of MiB (a whole observation block), where the int64 einsum takes minutes."""
    return _triangle(*_square(packed, n_pol, np.float64))


def to_square(tri, n_ant):
    """[...][bl][2] -> the full Hermitian complex128 array [...][a1][a2]."""
    tri = np.asarray(tri)
    assert tri.shape[-2:] == (n_baselines(n_ant), 2)
    a1, a2 = np.tril_indices(n_ant)
    z = tri[..., 0].astype(np.float64) + 1j * tri[..., 1].astype(np.float64)
    sq = np.zeros(tri.shape[:-2] + (n_ant, n_ant), np.complex128)
    sq[..., a2, a1] = np.conj(z)
    sq[..., a1, a2] = z
    return sq


KNOWN_BYTES = bytes([0x25, 0xD7, 0x00, 0x00])   # antenna 0: 2+5i, antenna 1: -3+7i, in one column of four antennas
KNOWN = {(1, 0): (29, 29), (1, 1): (58, 0), (0, 0): (29, 0)}
