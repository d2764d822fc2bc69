"""The Faraday synthesis stage restated in numpy (docs/FARADAY.md sections 1 and 2).

  * ``fma32`` -- the float32 fused multiply-add, exactly, by round-to-odd: the product of two float32 is exact in float64 (24 + 24
    bits), TwoSum gives the error of adding the addend, and where the float64 sum is inexact and its last bit even it is moved one
    step toward the error, so that the second rounding (to float32) cannot land on a false tie (done only for the elements whose
    float64 sum can be such a tie at all);
  * ``synthesize`` -- float32, in the operation order the document fixes: the device is compared with it bit for bit;
  * ``synthesize64`` -- the same float32 operands in float64: what the chain approximates;
  * the host helpers from the formulas of include/dsabf.h, and what `beam --faraday` makes of one record of its input.
Written from the contract: no knowledge of tiles, lanes or table layouts."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LIGHT = 0.299792458   # m GHz

PEAK = np.dtype([("p", np.int32), ("pow_lo", np.float32), ("pow_pk", np.float32), ("pow_hi", np.float32), ("re", np.float32),
                 ("im", np.float32), ("isum", np.float32), ("zero", np.int32)])


def _fma64(a, b, c):
    """fmaf of float32 values held in float64 arrays (broadcast against each other) -> float32.  s = a b + c in float64 rounds the
    exact value once; rounding s again to float32 goes wrong only if s sits exactly on the midpoint of two float32 (or of two
    subnormal float32) while the exact value does not: then the low 28 bits of s are zero.  Only those elements take TwoSum."""
    p = a * b                                # exact: 24 + 24 bits
    s = p + c
    ties = (s.view(np.int64) & 0x0FFFFFFF) == 0
    if ties.any():
        at = np.nonzero(ties)
        pt, ct, st = p[at], np.broadcast_to(c, s.shape)[at], s[at]
        bb = st - pt
        e = (pt - (st - bb)) + (ct - bb)     # TwoSum: st + e = pt + ct exactly
        need = (e != 0) & ((st.view(np.int64) & 1) == 0)
        s[at] = np.where(need, np.nextafter(st, np.where(e > 0, np.inf, -np.inf)), st)   # round to odd
    return s.astype(np.float32)


def fma32(a, b, c):
    """float32 fmaf(a, b, c), elementwise, for finite operands."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    return _fma64(*np.broadcast_arrays(a, b, c)) if np.ndim(a) or np.ndim(b) or np.ndim(c) else _fma64(a.reshape(1), b.reshape(1), c.reshape(1))[0]


# ---- host helpers -------------------------------------------------------------------------------------------------------------------
def lambda2(f_ghz):
    return (LIGHT / np.asarray(f_ghz, np.float64)) ** 2


def lambda0_2(freq_ghz, w):
    w = np.asarray(w, np.float64)
    return float(np.sum(w * lambda2(freq_ghz)) / np.sum(w))


def resolution(freq_ghz, w):
    l2, w = lambda2(freq_ghz), np.asarray(w, np.float64)
    used = l2[w > 0]
    return 2.0 * np.sqrt(3.0) / (used.max() - used.min()), np.sqrt(3.0) / np.abs(np.diff(l2)).max()


def angles(freq_ghz, w, phi0, dphi, n_phi):
    """2 phi_p (lambda_c^2 - lambda_0^2), float64 [n_phi][n_chan]."""
    phi = phi0 + np.arange(n_phi) * dphi
    return 2.0 * phi[:, None] * (lambda2(freq_ghz) - lambda0_2(freq_ghz, w))[None, :]


def table(freq_ghz, w, phi0, dphi, n_phi):
    """(rot complex64 [n_phi][n_chan] = wn (cos - i sin), wn float32 [n_chan], lambda_0^2)."""
    w = np.asarray(w, np.float64)
    wn = w / w.sum()
    a = angles(freq_ghz, w, phi0, dphi, n_phi)
    rot = np.empty(a.shape, np.complex64)
    rot.real, rot.imag = (wn * np.cos(a)).astype(np.float32), (wn * -np.sin(a)).astype(np.float32)
    return rot, wn.astype(np.float32), lambda0_2(freq_ghz, w)


def rmsf(freq_ghz, w, phi0, dphi, n_phi):
    w = np.asarray(w, np.float64)
    return np.sum((w / w.sum()) * np.exp(-1j * angles(freq_ghz, w, phi0, dphi, n_phi)), axis=1)


# ---- the stage ----------------------------------------------------------------------------------------------------------------------
def cells(s, base=None):
    """s float32 [n_rows][n_chan][K][4] -> (i, q, u) float32 [n_rows * K][n_chan], the baseline [n_chan][K][4] subtracted if given."""
    s = np.asarray(s, np.float32)
    if base is not None:
        s = s - np.asarray(base, np.float32)[None]          # float32 - float32: one rounding
    n_rows, n_chan, K, _ = s.shape
    m = s.transpose(0, 2, 1, 3).reshape(n_rows * K, n_chan, 4)
    return m[..., 0], m[..., 1], m[..., 2]


def spectrum(q, u, rot):
    """q, u float32 [M][n_chan], rot complex64 [n_phi][n_chan] -> (re, im) float32 [M][n_phi]: the two fmaf chains."""
    r, s = np.ascontiguousarray(rot.real.T, np.float64), np.ascontiguousarray(rot.imag.T, np.float64)   # [n_chan][n_phi]
    q, u = np.asarray(q, np.float32).astype(np.float64), np.asarray(u, np.float32).astype(np.float64)
    M, n_chan = q.shape
    re, im = np.empty((M, r.shape[1]), np.float32), np.empty((M, r.shape[1]), np.float32)
    block = max(1, 32768 // r.shape[1])                     # rows at a time: the temporaries stay in the cache

    def rows(m0):
        a_re, a_im = np.zeros((min(block, M - m0), r.shape[1])), np.zeros((min(block, M - m0), r.shape[1]))
        for c in range(n_chan):
            qc, uc = q[m0:m0 + block, c:c + 1], u[m0:m0 + block, c:c + 1]
            a_re = _fma64(uc, -s[c][None, :], _fma64(qc, r[c][None, :], a_re).astype(np.float64)).astype(np.float64)
            a_im = _fma64(uc, r[c][None, :], _fma64(qc, s[c][None, :], a_im).astype(np.float64)).astype(np.float64)
        re[m0:m0 + block], im[m0:m0 + block] = a_re, a_im    # (float32 values: the cast is exact)

    starts = range(0, M, block)
    if len(starts) > 2:                                     # rows are independent: a few threads (numpy releases the lock)
        with ThreadPoolExecutor(max_workers=4) as pool:
            list(pool.map(rows, starts))
    else:
        for m0 in starts:
            rows(m0)
    return re, im


def intensity(i, wn):
    acc = np.zeros(i.shape[0], np.float32)
    for c in range(i.shape[1]):
        acc = fma32(i[:, c], np.float32(wn[c]), acc)
    return acc


def peaks_of(re, im, isum):
    """The records of spectra (re, im) [M][n_phi]: the first maximum of re re + im im, its neighbours (0 outside the grid), F there."""
    power = re * re + im * im                               # float32: two products and one addition, each rounded
    M, n_phi = power.shape
    p = np.argmax(power, axis=1)                            # (the first of equal maxima)
    rows = np.arange(M)
    out = np.zeros(M, PEAK)
    out["p"] = p
    out["pow_pk"] = power[rows, p]
    out["pow_lo"] = np.where(p > 0, power[rows, np.maximum(p - 1, 0)], np.float32(0))
    out["pow_hi"] = np.where(p < n_phi - 1, power[rows, np.minimum(p + 1, n_phi - 1)], np.float32(0))
    out["re"], out["im"], out["isum"] = re[rows, p], im[rows, p], isum
    return out


def synthesize(s, rot, wn, base=None):
    """-> (spec complex64 [n_rows][K][n_phi], peaks PEAK [n_rows][K]): what bf_rm_device writes."""
    n_rows, _, K, _ = np.shape(s)
    i, q, u = cells(s, base)
    re, im = spectrum(q, u, np.asarray(rot, np.complex64))
    spec = np.empty(re.shape, np.complex64)
    spec.real, spec.imag = re, im
    return spec.reshape(n_rows, K, -1), peaks_of(re, im, intensity(i, np.asarray(wn, np.float32))).reshape(n_rows, K)


def synthesize64(s, rot, base=None):
    """The spectrum of the same float32 operands in float64, complex128 [n_rows * K][n_phi]."""
    _, q, u = cells(s, base)
    return (q.astype(np.float64) + 1j * u.astype(np.float64)) @ np.asarray(rot, np.complex64).astype(np.complex128).T


def refine(peaks, phi0, dphi, n_phi, l0):
    """-> (rm, pa, lin, frac) float64 arrays, from the formulas of include/dsabf.h."""
    pk = np.asarray(peaks)
    lo, mid, hi = pk["pow_lo"].astype(np.float64), pk["pow_pk"].astype(np.float64), pk["pow_hi"].astype(np.float64)
    den = lo - 2.0 * mid + hi
    inner = (pk["p"] > 0) & (pk["p"] < n_phi - 1) & (den != 0)
    delta = np.where(inner, 0.5 * (lo - hi) / np.where(den != 0, den, 1.0), 0.0)
    rm = phi0 + (pk["p"] + delta) * dphi
    pa = 0.5 * np.arctan2(pk["im"].astype(np.float64), pk["re"].astype(np.float64)) - rm * l0
    pa = (pa + np.pi / 2) % np.pi - np.pi / 2
    lin = np.sqrt(mid)
    isum = pk["isum"].astype(np.float64)
    return rm, pa, lin, np.where(isum > 0, lin / np.where(isum > 0, isum, 1.0), 0.0)


# ---- `beam --faraday`, per record ---------------------------------------------------------------------------------------------------
MIN_BASELINE_ROWS = 8


def default_grid(freq_ghz, w):
    """(phi0, dphi, n_phi): +-phi_max in steps of fwhm / 8, at most 4096 depths, centred on 0."""
    fwhm, phi_max = resolution(freq_ghz, w)
    dphi = fwhm / 8.0
    half = np.ceil(phi_max / dphi)
    n_phi = 4096 if half >= 2047.5 else 2 * int(half) + 1
    return -0.5 * (n_phi - 1) * dphi, dphi, n_phi


def window_of(data, w):
    """data float32 [n_rows][n_chan][4] -> lo: the FIRST maximum of a boxcar of w rows over sum_c I[t][c], float64, every sum in
    ascending order."""
    n_rows, n_chan, _ = data.shape
    series = np.zeros(n_rows, np.float64)
    for c in range(n_chan):
        series = series + data[:, c, 0].astype(np.float64)
    n = n_rows - w + 1
    box = series[:n].copy()
    for j in range(1, w):
        box = box + series[j:j + n]
    return int(np.argmax(box))


def _mean32(rows):
    """The mean of float32 rows [n][...] summed in float64 in ascending order, rounded to float32."""
    acc = np.zeros(rows.shape[1:], np.float64)
    for r in rows:
        acc = acc + r.astype(np.float64)
    return (acc / len(rows)).astype(np.float32)


def sparse_rows(lo, w, n_rows):
    """Row 0 (the window's mean), the rows of the window and their neighbours, the first and the last row, and every 16th."""
    keep = {0, 1, n_rows} | set(range(max(1, lo), min(n_rows, lo + w + 1) + 1)) | set(range(1, n_rows + 1, 16))
    return sorted(keep)


def faraday_record(data, w, rot, wn, rows=None):
    """One record of a coherent file -> None if it has fewer than 8 baseline rows, else (lo, spec complex64 [n_phi] of row 0, peaks PEAK
    [1 + n_rows]): row 0 is the mean of the window [lo, lo + w), the baseline the mean of the rows outside [lo - w, lo + 2 w).
    ``rows``: a function (lo, w, n_rows) -> ascending indices into the 1 + n_rows rows of the launch, 0 first -- only their peaks are
    computed and returned, in that order (sparse_rows, for a grid too long to take every row through numpy)."""
    data = np.asarray(data, np.float32)
    n_rows = data.shape[0]
    w = max(1, min(int(w), n_rows))
    lo = window_of(data, w)
    t = np.arange(n_rows)
    off = (t < lo - w) | (t >= lo + 2 * w)
    if off.sum() < MIN_BASELINE_ROWS:
        return None
    base = _mean32(data[off])
    launch = np.concatenate([_mean32(data[lo:lo + w])[None], data], axis=0)
    if rows is not None:
        idx = np.asarray(rows(lo, w, n_rows))
        assert idx[0] == 0 and (np.diff(idx) > 0).all() and idx[-1] <= n_rows
        launch = launch[idx]
    spec, peaks = synthesize(launch[:, :, None, :], rot, wn, base[:, None, :])
    return lo, spec[0, 0], peaks[:, 0]
