"""The spatial null's reference (docs/NULLING.md): deflated power iteration on the visibility matrix and the projection of the weights,
in numpy float64 with every sum over antennas in the ONE fixed order of docs/CALIBRATION.md section 2 (OSUM).

    x = V (Hermitian, diagonal kept),   u_j = dominant eigenvectors,   w' = w - sum_j conj(u_j) (u_j^T w)

Every complex product is written out in real arithmetic, (ar br - ai bi, ar bi + ai br), so that numpy performs exactly the IEEE
operations the device does, one rounding each.  `solve` is batched over the channels; `solve_slow` restates one channel element by
element in Python floats and shares no code with it.  `project` is the weight projection, `scene` the interferer field of the tests.
Nothing here imports the product.
"""
import math

import numpy as np

from cal_oracle import bl, osum

MAX_ANT = 256
MAX_NULL = 4
SCALED, CLIP = 0, 1


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def squares(vis, n_ant, pol=-1):
    """int64 [freq][pol][bl][2] -> (xr, xi) float64 [freq][p][q], Hermitian, the diagonal (re, +0.0).  pol -1: the integers of the
    polarisations are added first; otherwise that one polarisation."""
    vis = np.asarray(vis)
    assert vis.dtype == np.int64 and vis.shape[2:] == (n_ant * (n_ant + 1) // 2, 2) and -1 <= pol < vis.shape[1]
    v = vis.sum(axis=1, dtype=np.int64) if pol < 0 else vis[:, pol]
    a1, a2 = np.tril_indices(n_ant)
    re, im = v[..., 0].astype(np.float64), v[..., 1].astype(np.float64)
    xr = np.zeros((v.shape[0], n_ant, n_ant), np.float64)
    xi = np.zeros_like(xr)
    xr[:, a2, a1], xi[:, a2, a1] = re, -im
    xr[:, a1, a2], xi[:, a1, a2] = re, im
    d = np.arange(n_ant)
    xi[:, d, d] = 0.0
    return xr, xi


def solve(vis, n_ant, flags=None, n_null=1, min_ratio=4.0, tol=1e-6, max_iter=200, pol=-1, summer=osum):
    """-> (vecs float64 [freq][n_null][ant][2], eig float64 [freq][n_null + 1], info int32 [freq][1 + 2 n_null]).  `summer(terms, axis)`
    replaces OSUM (the CPU test uses it to show that another association gives other bits)."""
    assert n_ant % 4 == 0 and 0 < n_ant <= MAX_ANT and 1 <= n_null <= MAX_NULL and max_iter >= 1 and tol >= 0 and min_ratio >= 0
    xr, xi = squares(vis, n_ant, pol)
    n_f = xr.shape[0]
    flagged = np.zeros(n_ant, bool) if flags is None else np.asarray(flags).astype(bool)
    live = ~flagged
    m = int(live.sum())
    keep = live[:, None] & live[None, :]
    xr, xi = np.where(keep, xr, 0.0), np.where(keep, xi, 0.0)
    d = np.arange(n_ant)
    diag = xr[:, d, d]
    tr = summer(diag, -1)
    if m:
        star = np.argmax(np.where(live, diag, -np.inf), axis=1)      # the first maximum: the lowest index on ties
        y0r, y0i = xr[np.arange(n_f), :, star], xi[np.arange(n_f), :, star]
    else:
        y0r, y0i = np.zeros((n_f, n_ant)), np.zeros((n_f, n_ant))
    vecs = np.zeros((n_f, n_null, n_ant, 2))
    eig = np.zeros((n_f, n_null + 1))
    info = np.zeros((n_f, 1 + 2 * n_null), np.int32)
    eig[:, n_null] = tr
    ended = np.zeros(n_f, bool)
    found = []
    for j in range(n_null):
        act = ~ended
        ur, ui = np.zeros((n_f, n_ant)), np.zeros((n_f, n_ant))
        lam_j, it_j, st_j = np.zeros(n_f), np.zeros(n_f, np.int32), np.where(ended, 2, 0).astype(np.int32)
        k = 0
        while act.any():
            if k == 0:
                yr, yi = y0r.copy(), y0i.copy()
            else:
                yr = summer(xr * ur[:, None, :] - xi * ui[:, None, :], -1)
                yi = summer(xr * ui[:, None, :] + xi * ur[:, None, :], -1)
            for er, ei in found:
                tr_, ti_ = _cmul(er, -ei, yr, yi)
                cr, ci = summer(tr_, -1)[:, None], summer(ti_, -1)[:, None]
                pr, pi = _cmul(er, ei, cr, ci)
                yr, yi = yr - pr, yi - pi
            lam = np.sqrt(summer(yr * yr + yi * yi, -1))
            zero = lam == 0
            hit = act & zero
            st_j[hit], it_j[hit] = 2, k
            ended |= hit
            act = act & ~zero
            safe = np.where(zero, 1.0, lam)[:, None]
            nr, ni = yr / safe, yi / safe
            if k >= 1:
                dr, di = nr - ur, ni - ui
                delta = summer(dr * dr + di * di, -1)
            ur[act], ui[act], lam_j[act], it_j[act] = nr[act], ni[act], lam[act], k
            if k >= 1:
                conv = act & (delta <= tol * tol)
                st_j[conv] = 1
                act = act & ~conv
                if k == max_iter:
                    act = np.zeros(n_f, bool)
            k += 1
        gone = st_j == 2
        ur[gone], ui[gone], lam_j[gone] = 0.0, 0.0, 0.0
        found.append((ur, ui))
        eig[:, j] = lam_j
        info[:, 1 + 2 * j], info[:, 2 + 2 * j] = it_j, st_j
    used = np.ones(n_f, bool)
    rem = tr.copy()
    for j in range(n_null):
        rem = rem - eig[:, j]
        if m > j + 1:
            rest = rem / (m - j - 1)
            used = used & (eig[:, j] > 0) & (eig[:, j] >= min_ratio * np.maximum(rest, 0.0))
        else:
            used = np.zeros(n_f, bool)
        vecs[used, j, :, 0], vecs[used, j, :, 1] = found[j][0][used], found[j][1][used]
        info[:, 0] += used
    return vecs, eig, info


def solve_slow(tri, n, flags=None, n_null=1, min_ratio=4.0, tol=1e-6, max_iter=200):
    """ONE channel, element by element in Python floats: tri int64 [bl][2] (already summed over the polarisations if pol is -1).
    -> (vecs: n_null lists of (re, im), eig: list of n_null + 1, info: list of 1 + 2 n_null)."""
    fl = [False] * n if flags is None else [bool(f) for f in flags]
    x = [[(0.0, 0.0)] * n for _ in range(n)]
    for p in range(n):
        for q in range(n):
            if fl[p] or fl[q]:
                continue
            if q < p:
                x[p][q] = (float(int(tri[bl(p, q)][0])), float(int(tri[bl(p, q)][1])))
            elif q > p:
                x[p][q] = (float(int(tri[bl(q, p)][0])), -float(int(tri[bl(q, p)][1])))
            else:
                x[p][p] = (float(int(tri[bl(p, p)][0])), 0.0)

    def tree(terms):
        part = [0.0] * 64
        for i, t in enumerate(terms):
            part[i % 64] = part[i % 64] + t
        w = 32
        while w:
            part = [part[i] + part[i + w] for i in range(w)]
            w //= 2
        return part[0]

    m = sum(1 for f in fl if not f)
    tr = tree([x[p][p][0] for p in range(n)])
    star = -1
    for p in range(n):
        if not fl[p] and (star < 0 or x[p][p][0] > x[star][star][0]):
            star = p
    found, eig, info, ended = [], [], [0], False
    for j in range(n_null):
        if ended:
            found.append([(0.0, 0.0)] * n)
            eig.append(0.0)
            info += [0, 2]
            continue
        u, it, status, lam = None, 0, 0, 0.0
        while True:
            if it == 0:
                y = [x[p][star] if star >= 0 else (0.0, 0.0) for p in range(n)]
            else:
                y = [(tree([x[p][q][0] * u[q][0] - x[p][q][1] * u[q][1] for q in range(n)]),
                      tree([x[p][q][0] * u[q][1] + x[p][q][1] * u[q][0] for q in range(n)])) for p in range(n)]
            for e in found:
                cr = tree([e[p][0] * y[p][0] - (-e[p][1]) * y[p][1] for p in range(n)])
                ci = tree([e[p][0] * y[p][1] + (-e[p][1]) * y[p][0] for p in range(n)])
                y = [(y[p][0] - (e[p][0] * cr - e[p][1] * ci), y[p][1] - (e[p][0] * ci + e[p][1] * cr)) for p in range(n)]
            lam = math.sqrt(tree([a * a + b * b for a, b in y]))
            if lam == 0:
                status, ended, lam, u = 2, True, 0.0, [(0.0, 0.0)] * n
                break
            new = [(a / lam, b / lam) for a, b in y]
            if it >= 1:
                delta = tree([(a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) for a, b in zip(new, u)])
                u = new
                if delta <= tol * tol:
                    status = 1
                    break
                if it == max_iter:
                    break
            else:
                u = new
            it += 1
        found.append(u)
        eig.append(lam)
        info += [it, status]
    eig.append(tr)
    used, rem, vecs = True, tr, []
    for j in range(n_null):
        rem = rem - eig[j]
        used = used and m > j + 1 and eig[j] > 0 and eig[j] >= min_ratio * max(rem / (m - j - 1), 0.0)
        vecs.append(found[j] if used else [(0.0, 0.0)] * n)
        info[0] += int(used)
    return vecs, eig, info


def project(w, vecs, info, flags=None, mode=SCALED, return_float=False):
    """w int8 [freq][ant][beam][2], vecs float64 [freq][n_null][ant][2], info int32 [freq][1 + 2 n_null] -> (int8 weights, scale
    float64 [freq]); with return_float the unquantised w' (complex parts [freq][ant][beam][2]) as a third value."""
    w, vecs, info = np.asarray(w), np.asarray(vecs, np.float64), np.asarray(info)
    n_f, n_ant, n_b = w.shape[:3]
    n_null = vecs.shape[1]
    assert w.dtype == np.int8 and vecs.shape == (n_f, n_null, n_ant, 2) and info.shape == (n_f, 1 + 2 * n_null) and mode in (SCALED, CLIP)
    flagged = np.zeros(n_ant, bool) if flags is None else np.asarray(flags).astype(bool)
    out = w.copy()
    out[:, flagged] = 0
    scale = np.ones(n_f)
    wf = w.astype(np.float64)
    wf[:, flagged] = 0.0
    for f in range(n_f):
        n_used = min(max(int(info[f, 0]), 0), n_null)
        if n_used == 0:
            continue
        wr, wi = w[f, :, :, 0].astype(np.float64), w[f, :, :, 1].astype(np.float64)       # [ant][beam]
        cs = []
        for j in range(n_used):
            ur, ui = vecs[f, j, :, 0:1], vecs[f, j, :, 1:2]
            tr_, ti_ = _cmul(ur, ui, wr, wi)
            cs.append((osum(tr_, 0), osum(ti_, 0)))
        pr, pi = wr, wi
        for j in range(n_used):
            ur, ui = vecs[f, j, :, 0:1], vecs[f, j, :, 1:2]
            tr_, ti_ = _cmul(ur, -ui, cs[j][0][None, :], cs[j][1][None, :])
            pr, pi = pr - tr_, pi - ti_
        pr, pi = np.where(flagged[:, None], 0.0, pr), np.where(flagged[:, None], 0.0, pi)
        k = 1.0
        if mode == SCALED:
            big = max(np.abs(pr).max(), np.abs(pi).max())
            k = min(1.0, 127.0 / big) if big > 0 else 1.0
        scale[f] = k
        out[f, :, :, 0] = np.clip(np.rint(k * pr), -127, 127)
        out[f, :, :, 1] = np.clip(np.rint(k * pi), -127, 127)
        wf[f, :, :, 0], wf[f, :, :, 1] = pr, pi
    return (out, scale, wf) if return_float else (out, scale)


def pack(v):
    """complex [...] -> the 4-bit two's-complement bytes (re in the high nibble), rounded and clipped to -8 ... 7."""
    re, im = np.clip(np.rint(v.real), -8, 7).astype(np.int64), np.clip(np.rint(v.imag), -8, 7).astype(np.int64)
    return (((re & 15) << 4) | (im & 15)).astype(np.uint8)


def scene(seed, n_ant, n_freq, n_units, n_time, signatures, amplitudes, noise=1.0):
    """Interferers of fixed antenna signatures plus noise, as 4-bit voltages: v[u][f][t][a] = sum_i amp[i][f] sig[i][a] s_i[u][f][t] +
    noise n[u][f][t][a], s and n unit complex Gaussians.  signatures complex [n_int][ant], amplitudes [n_int][freq].
    -> (packed uint8 [unit][freq][time][ant], packed_interferers: the same without the noise)."""
    rng = np.random.default_rng(seed)
    sig, amp = np.asarray(signatures, np.complex128).reshape(-1, n_ant), np.asarray(amplitudes, np.float64).reshape(-1, n_freq)
    shape = (n_units, n_freq, n_time)
    cg = lambda s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)   # noqa: E731
    rfi = np.zeros(shape + (n_ant,), np.complex128)
    for i in range(sig.shape[0]):
        rfi += (amp[i][None, :, None] * cg(shape))[..., None] * sig[i]
    return pack(rfi + noise * cg(shape + (n_ant,))), pack(rfi)


def exact_vis(signatures, powers, n_ant, n_freq, n_pol, noise=0, seed=0):
    """Visibilities of interferers at the visibility level: V = rint(sum_i P[i][f] s_i s_i^H) + noise on the diagonal and integer noise
    of +-`noise` elsewhere.  -> int64 [freq][pol][bl][2]."""
    rng = np.random.default_rng(seed)
    sig, pw = np.asarray(signatures, np.complex128).reshape(-1, n_ant), np.asarray(powers, np.float64).reshape(-1, n_freq)
    a1, a2 = np.tril_indices(n_ant)
    v = np.zeros((n_freq, n_pol, a1.size), np.complex128)
    for i in range(sig.shape[0]):
        v += pw[i][:, None, None] * (sig[i][a1] * np.conj(sig[i][a2]))[None, None, :]
    vis = np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1).astype(np.int64)
    if noise:
        vis += rng.integers(-noise, noise + 1, size=vis.shape)
        vis[:, :, [bl(a, a) for a in range(n_ant)], 0] += 64 * noise
    vis[:, :, [bl(a, a) for a in range(n_ant)], 1] = 0
    return vis
