"""Oracle of the voltage moments and of the spectral-kurtosis flag rule (include/dsabf.h: bf_sk_device, bf_sk_select;
docs/SPECTRAL_KURTOSIS.md).  moments(): a 256-entry table of p = re^2 + im^2 per byte code and an int64 reshape-sum.  select(): the
operation order of include/dsabf.h in float64, one rounding per operation, which the library (built without contraction) reproduces
to the bit.  scene(): the test scene of four kinds of antenna."""
import numpy as np

_N = np.arange(256)
RE = np.where((_N >> 4) >= 8, (_N >> 4) - 16, _N >> 4).astype(np.int64)      # high nibble, two's complement
IM = np.where((_N & 15) >= 8, (_N & 15) - 16, _N & 15).astype(np.int64)      # low nibble
P = RE * RE + IM * IM                                                        # 0 ... 128
P2 = P * P

KNOWN_BYTES = bytes([0xD7, 0x25, 0xA8, 0x70])                                # four columns of one antenna, n_pol = 1
KNOWN = (236, 16606)                                                         # 58 + 29 + 100 + 49, 58^2 + 29^2 + 100^2 + 49^2

DEAD, LOW, HIGH = 1, 2, 4
DEFAULTS = dict(centre=1.0, n_sigma=5.0, max_bad_fraction_ant=0.5, max_bad_fraction_chan=0.5)


def moments(packed, n_pol):
    """packed uint8 [unit][freq][n_cols * n_pol][ant] -> int64 [freq][n_pol][ant][2] = {M1, M2}; column c belongs to polarisation
    c % n_pol."""
    packed = np.asarray(packed, np.uint8)
    n_units, n_freq, n_time, n_ant = packed.shape
    assert n_time % n_pol == 0
    out = np.empty((n_freq, n_pol, n_ant, 2), np.int64)
    for k, table in enumerate((P, P2)):
        v = table[packed].reshape(n_units, n_freq, n_time // n_pol, n_pol, n_ant)
        out[..., k] = v.sum(axis=(0, 2), dtype=np.int64)
    return out


def select(mom, M, centre=1.0, n_sigma=5.0, max_bad_fraction_ant=0.5, max_bad_fraction_chan=0.5):
    """mom int64 [freq][pol][ant][2] over M >= 2 columns per polarisation -> (sk float64 [freq][pol][ant], cell uint8, ant_flags uint8
    [ant], chan_flags uint8 [freq])."""
    mom = np.asarray(mom, np.int64)
    n_freq, n_pol, n_ant, _ = mom.shape
    assert M >= 2
    m1, m2 = mom[..., 0].astype(np.float64), mom[..., 1].astype(np.float64)
    Md = np.float64(M)
    dead = mom[..., 0] == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (Md * m2) / (m1 * m1)
        sk = (np.float64(M + 1) / np.float64(M - 1)) * (r - np.float64(1.0))
    sk = np.where(dead, np.float64(0.0), sk)
    half_width = np.float64(n_sigma) * np.float64(2.0) / np.sqrt(Md)
    lo, hi = np.float64(centre) - half_width, np.float64(centre) + half_width
    cell = np.where(dead, DEAD, np.where(sk < lo, LOW, 0) | np.where(sk > hi, HIGH, 0)).astype(np.uint8)
    bad = cell != 0
    bad_a = bad.sum(axis=(0, 1))
    ant_flags = (bad_a.astype(np.float64) > np.float64(max_bad_fraction_ant) * np.float64(n_freq * n_pol)).astype(np.uint8)
    good = ant_flags == 0
    n_good = int(good.sum())
    bad_f = bad[:, :, good].sum(axis=(1, 2))
    chan_flags = (bad_f.astype(np.float64) > np.float64(max_bad_fraction_chan) * np.float64(n_good * n_pol)).astype(np.uint8)
    if n_good == 0:
        chan_flags[:] = 1
    return sk, cell, ant_flags, chan_flags


def pack(z):
    """complex array -> packed bytes: both parts rounded and clipped to -8 ... 7, re in the high nibble."""
    re = np.clip(np.rint(z.real), -8, 7).astype(np.int64)
    im = np.clip(np.rint(z.imag), -8, 7).astype(np.int64)
    return (((re & 15) << 4) | (im & 15)).astype(np.uint8)


SCENE_BAD = (5, 9, 12)


def scene(seed, n_freq=3, n_pol=2, n_ant=16, n_cols=4096, common=0.0):
    """The scene of docs/SPECTRAL_KURTOSIS.md as ONE unit [1][freq][n_cols * n_pol][ant]: Gaussian noise of sigma = 2 levels per part;
    antenna 5 carries 5 exp(2 pi i 0.1234 t) plus sigma = 0.5 noise, antenna 9 is all zero, every 10th sample of antenna 12 is scaled
    by 3.  `common`: the amplitude of one more Gaussian term that every antenna but 9 shares (a point source at the phase centre), so
    that the visibilities have a solution."""
    rng = np.random.default_rng(seed)
    T = n_cols * n_pol
    shape = (1, n_freq, T, n_ant)
    z = 2.0 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    t = np.arange(T, dtype=np.float64)
    carrier = 5.0 * np.exp(2j * np.pi * 0.1234 * t)
    z[..., 5] = carrier[None, None, :] + 0.5 * (rng.standard_normal(shape[:3]) + 1j * rng.standard_normal(shape[:3]))
    z[:, :, (np.arange(T) // n_pol) % 10 == 0, 12] *= 3.0   # every 10th sample of either polarisation
    if common:
        s = common * (rng.standard_normal(shape[:3]) + 1j * rng.standard_normal(shape[:3]))
        z += s[..., None]
    z[..., 9] = 0.0
    return pack(z)


def write_moments_file(path: str, first_channel: int, records) -> None:
    """A file of voltage moments in the format `beam -Y` writes (docs/SPECTRAL_KURTOSIS.md), for `beam -e`: records is a list of
    (first_block, n_columns_per_pol, moments [n_freq][n_pol][n_ant][2])."""
    n_freq, n_pol, n_ant, _ = np.shape(records[0][2])
    text = ("HDR_VERSION 1.0\nHDR_SIZE %d\nINSTRUMENT DSA\nCONTENT voltage_moments\nDTYPE int64\nENDIAN little\nLAYOUT %s\n"
            "RECORD_HEADER_BYTES 16\nNANT %d\nNPOL %d\nNFREQ %d\nFIRST_CHANNEL %d\n"
            % (4096, "freq,pol,ant,m1m2", n_ant, n_pol, n_freq, first_channel)).encode()
    with open(path, "wb") as fp:
        fp.write(text.ljust(4096, b"\0"))
        for first_block, n_columns, moments in records:
            m = np.ascontiguousarray(moments, "<i8")
            assert m.shape == (n_freq, n_pol, n_ant, 2)
            fp.write(np.array([first_block, n_columns], "<u8").tobytes() + m.tobytes())
