"""The coherent dedispersion stage restated in numpy (docs/COHERENT_DEDISPERSION.md sections 1 and 2).

Two restatements of the same overlap-save segments:
  * ``dedisperse`` -- float32, in the operation order the document fixes (radix-2 decimation in frequency forward, the multiply by the
    table in bit-reversed order, radix-2 decimation in time with the conjugated twiddles back), every numpy operation on float32 arrays
    rounding on its own: the device is compared with it bit for bit;
  * ``dedisperse64`` -- complex128 on numpy.fft: what the float32 order is an approximation of.
Written from the contract: stage loops over reshaped arrays, no knowledge of how the kernel groups stages or lays out its memory."""
import numpy as np

DISPERSION = 4.15   # ms GHz^2 per pc cm^-3, the project's constant (dm_delays)


# ---- host helpers, from the formulas of include/dsabf.h ---------------------------------------------------------------------------
def sweep_samples(dm, f_ghz, bw_mhz):
    return DISPERSION * 1e3 * dm * ((f_ghz - bw_mhz / 2000.0) ** -2 - (f_ghz + bw_mhz / 2000.0) ** -2) * bw_mhz


def edge(dm, freq_ghz, bw_mhz):
    return int(max(np.ceil(sweep_samples(dm, f, bw_mhz)) for f in np.atleast_1d(freq_ghz)))


def chirp_phase(dm, freq_ghz, bw_mhz, sideband, n):
    """phi [chan][n], float64: nu = sideband (j < n/2 ? j : j - n) bw / n MHz, phi = 2 pi 4.15e9 dm nu^2 / (F^2 (F + nu)), F in MHz."""
    j = np.arange(n)
    nu = sideband * np.where(j < n // 2, j, j - n).astype(np.float64) * bw_mhz / n
    F = 1000.0 * np.atleast_1d(np.asarray(freq_ghz, np.float64))[:, None]
    return 2.0 * np.pi * DISPERSION * 1e9 * dm * nu * nu / (F * F * (F + nu))


def chirp(dm, freq_ghz, bw_mhz, sideband, n):
    """complex64 [chan][n]: (cos phi, sin phi) / n, each part rounded to float32."""
    phi = chirp_phase(dm, freq_ghz, bw_mhz, sideband, n)
    out = np.empty(phi.shape, np.complex64)
    out.real, out.imag = (np.cos(phi) / n).astype(np.float32), (np.sin(phi) / n).astype(np.float32)
    return out


# ---- the segments -----------------------------------------------------------------------------------------------------------------
def n_segments(n_time, n, n_edge):
    v = n - 2 * n_edge
    return (n_time + v - 1) // v


def segments(x, n, n_edge):
    """x [..., n_time] -> [..., n_seg, n]: segment g holds the samples [g V - n_edge, g V - n_edge + n), zero outside the series."""
    n_time = x.shape[-1]
    v, g = n - 2 * n_edge, n_segments(n_time, n, n_edge)
    padded = np.zeros(x.shape[:-1] + (n_edge + g * v + n,), x.dtype)
    padded[..., n_edge:n_edge + n_time] = x
    idx = (np.arange(g) * v)[:, None] + np.arange(n)[None, :]
    return padded[..., idx]


def overlap_save(y, n_time, n_edge):
    """y [..., n_seg, n] -> [..., n_time]: the samples [n_edge, n - n_edge) of every segment, in order."""
    n = y.shape[-1]
    return y[..., n_edge:n - n_edge].reshape(y.shape[:-2] + (-1,))[..., :n_time]


# ---- float32, the fixed order -----------------------------------------------------------------------------------------------------
def twiddles(n):
    """(cos, -sin)(2 pi k / n), k < n / 2: computed in float64, rounded to float32."""
    a = -2.0 * np.pi * np.arange(n // 2) / n
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def bit_reverse(n):
    m = n.bit_length() - 1
    p = np.arange(n)
    r = np.zeros(n, np.int64)
    for b in range(m):
        r |= ((p >> b) & 1) << (m - 1 - b)
    return r


def _cmul(ar, ai, br, bi):
    """(ar + i ai)(br + i bi): four products, one subtraction, one addition, each rounded."""
    return ar * br - ai * bi, ar * bi + ai * br


def forward(re, im):
    """Radix-2 decimation in frequency along the last axis, half-lengths n/2 ... 1: natural order in, bit-reversed order out.
    A butterfly of half-length h at offset j: lower' = lower + upper, upper' = (lower - upper) * w[j n / (2 h)]."""
    n = re.shape[-1]
    wr, wi = twiddles(n)
    re, im = re.astype(np.float32), im.astype(np.float32)
    h = n // 2
    while h >= 1:
        shape = re.shape[:-1] + (n // (2 * h), 2, h)
        r, i = re.reshape(shape), im.reshape(shape)
        tr, ti = wr[::n // (2 * h)], wi[::n // (2 * h)]
        sr, si = r[..., 0, :] + r[..., 1, :], i[..., 0, :] + i[..., 1, :]
        dr, di = r[..., 0, :] - r[..., 1, :], i[..., 0, :] - i[..., 1, :]
        ur, ui = _cmul(dr, di, tr, ti)
        re, im = np.stack([sr, ur], axis=-2).reshape(re.shape), np.stack([si, ui], axis=-2).reshape(im.shape)
        h //= 2
    return re, im


def inverse(re, im):
    """Radix-2 decimation in time with the conjugated twiddles, half-lengths 1 ... n/2: bit-reversed order in, natural order out, no
    scale.  A butterfly: t = upper * conj(w)[j n / (2 h)], lower' = lower + t, upper' = lower - t."""
    n = re.shape[-1]
    wr, wi = twiddles(n)
    wi = -wi
    h = 1
    while h < n:
        shape = re.shape[:-1] + (n // (2 * h), 2, h)
        r, i = re.reshape(shape), im.reshape(shape)
        tr, ti = _cmul(r[..., 1, :], i[..., 1, :], wr[::n // (2 * h)], wi[::n // (2 * h)])
        re = np.stack([r[..., 0, :] + tr, r[..., 0, :] - tr], axis=-2).reshape(re.shape)
        im = np.stack([i[..., 0, :] + ti, i[..., 0, :] - ti], axis=-2).reshape(im.shape)
        h *= 2
    return re, im


def filter_segments(seg, table):
    """seg complex64 [chan][...][n], table complex64 [chan][n] -> IDFT(DFT(seg) * table) in the fixed float32 order."""
    n = seg.shape[-1]
    t = table[(slice(None),) + (None,) * (seg.ndim - 2) + (bit_reverse(n),)]
    fr, fi = forward(seg.real, seg.imag)
    mr, mi = _cmul(fr, fi, t.real.astype(np.float32), t.imag.astype(np.float32))
    yr, yi = inverse(mr, mi)
    out = np.empty(seg.shape, np.complex64)
    out.real, out.imag = yr, yi
    return out


def dedisperse(x, table, n_edge):
    """x complex64 [chan][k][pol][n_time], table complex64 [chan][n] -> the same shape: what bf_cdd_voltages_device writes."""
    x = np.asarray(x, np.complex64)
    n = table.shape[-1]
    return overlap_save(filter_segments(segments(x, n, n_edge), table), x.shape[-1], n_edge)


def dedisperse64(x, table, n_edge):
    """The same segments in complex128 on numpy.fft (ifft's own 1 / n undone: the table carries the scale)."""
    x = np.asarray(x, np.complex128)
    n = table.shape[-1]
    seg = segments(x, n, n_edge)
    t = np.asarray(table, np.complex128)[(slice(None),) + (None,) * (seg.ndim - 2)]
    return overlap_save(np.fft.ifft(np.fft.fft(seg, axis=-1) * t, axis=-1) * n, x.shape[-1], n_edge)


def stokes(y, n_int):
    """y complex64 [chan][k][pol][n_time] -> float32 [n_time / n_int][chan][k]{I, Q, U, V}, the window summed in ascending order
    starting FROM its first sample (no zero is added): what bf_cdd_stokes_device writes behind ``dedisperse``."""
    y = np.asarray(y, np.complex64)
    xr, xi, yr, yi = y[:, :, 0].real, y[:, :, 0].imag, y[:, :, 1].real, y[:, :, 1].imag
    px, py = xr * xr + xi * xi, yr * yr + yi * yi
    uu, vv = xr * yr + xi * yi, xi * yr - xr * yi
    cells = np.stack([px + py, px - py, np.float32(2) * uu, np.float32(2) * vv], axis=-1)   # [chan][k][n][4]
    c, k, n_time, _ = cells.shape
    assert n_time % n_int == 0
    w = cells.reshape(c, k, n_time // n_int, n_int, 4)
    acc = w[:, :, :, 0]
    for s in range(1, n_int):
        acc = acc + w[:, :, :, s]
    return np.ascontiguousarray(acc.transpose(2, 0, 1, 3), np.float32)


# ---- physics, float64 only --------------------------------------------------------------------------------------------------------
def dispersed_impulse(dm, f_ghz, bw_mhz, sideband, at, length=8192):
    """An impulse at sample ``at`` of a series of ``length``, dispersed by ONE long transform with the conjugate chirp (float64)."""
    phi = chirp_phase(dm, [f_ghz], bw_mhz, sideband, length)[0]
    x = np.zeros(length, np.complex128)
    x[at] = 1.0
    return np.fft.ifft(np.fft.fft(x) * np.exp(-1j * phi))


def chirp64(dm, freq_ghz, bw_mhz, sideband, n):
    return np.exp(1j * chirp_phase(dm, freq_ghz, bw_mhz, sideband, n)) / n


# ---- the file `beam --coherent` writes, by hand ----------------------------------------------------------------------------------------
def write_coherent_file(path, n_freq, first_channel, n_fft, n_int, sideband, n_time, records):
    """records = [(t0, dm, beam, width, snr, dm_value, n_edge, n_fft, float32 [n_time / n_int][n_freq][4])]."""
    head = ("HDR_SIZE 4096\nCONTENT coherent_stokes\nDTYPE float32\nNFREQ %d\nFIRST_CHANNEL %d\nNFFT %d\nNINT %d\nSIDEBAND %d\nNTIME %d\n"
            "LAYOUT time,freq,iquv\nRECORD_HEADER_BYTES 44\n" % (n_freq, first_channel, n_fft, n_int, sideband, n_time)).encode()
    with open(path, "wb") as f:
        f.write(head + b"\0" * (4096 - len(head)))
        for t0, dm, beam, width, snr, dm_value, n_edge, n, data in records:
            f.write(np.array([t0], "<u8").tobytes() + np.array([dm, beam, width], "<i4").tobytes() + np.array([snr, dm_value], "<f8").tobytes()
                    + np.array([n_edge, n], "<i4").tobytes())
            f.write(np.ascontiguousarray(data, "<f4").tobytes())
