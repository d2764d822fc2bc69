"""The gain solver's reference (docs/CALIBRATION.md): StEFCal in numpy float64, every sum in the ONE fixed order the contract names.

    V[a1][a2] ~ g[a1] conj(g[a2]) M[a1][a2],   M[p][q] = s_p conj(s_q)

`osum` is the contract's OSUM: 64 partial sums (partial l adds the terms l, l + 64, l + 128, l + 192 that exist, ascending, onto +0.0),
then six halving steps (64 -> 32 adds elements l and l + 32, then 16, 8, 4, 2, 1).  Every complex product is written out in real
arithmetic, (ar br - ai bi, ar bi + ai br), so that numpy performs exactly the IEEE operations the device does, one rounding each.

`solve` is batched over the (pol_out, freq) problems; `solve_slow` restates one problem element by element in Python floats and
shares no code with it.  `calibrate_weights` is the elementwise weight correction.  Nothing here imports the product.
"""
import math

import numpy as np

MAX_ANT = 256
PHASE, FULL = 0, 1


def bl(a1, a2):
    return a1 * (a1 + 1) // 2 + a2


_scratch = {}


def _buf(tag, shape):
    """A reusable float64 work array (fresh 16 MiB temporaries cost more in page faults than the arithmetic on them)."""
    b = _scratch.get(tag)
    if b is None or b.shape != tuple(shape):
        b = _scratch[tag] = np.empty(shape, np.float64)
    return b


def osum(t, axis=-1):
    """OSUM over one axis (length n <= 256) of a float64 array."""
    t = np.moveaxis(np.asarray(t, np.float64), axis, 0)
    n = t.shape[0]
    assert 0 < n <= MAX_ANT
    s = _buf("osum", (64,) + t.shape[1:])
    s[...] = 0.0
    for k in range((n + 63) // 64):                      # ascending: l, l + 64, l + 128, l + 192
        m = min(64, n - 64 * k)
        np.add(s[:m], t[64 * k:64 * k + m], out=s[:m])
    w = 32
    while w >= 1:                                        # 64 -> 32 -> 16 -> 8 -> 4 -> 2 -> 1
        np.add(s[:w], s[w:2 * w], out=s[:w])
        w //= 2
    return s[0].copy()


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def squares(vis, n_ant, joint_pol):
    """int64 [freq][pol][bl][2] -> (xr, xi, diag): float64 squares [pol_out][freq][p][q] with a zero diagonal, and the integer
    diagonal [pol_out][freq][p] (with joint_pol the integers of the polarisations are added first)."""
    vis = np.asarray(vis)
    assert vis.dtype == np.int64 and vis.shape[2:] == (n_ant * (n_ant + 1) // 2, 2)
    v = vis.transpose(1, 0, 2, 3)                        # [pol][freq][bl][2]
    if joint_pol:
        v = v.sum(axis=0, dtype=np.int64, keepdims=True)
    a1, a2 = np.tril_indices(n_ant)
    re, im = v[..., 0].astype(np.float64), v[..., 1].astype(np.float64)
    xr = np.zeros(v.shape[:2] + (n_ant, n_ant), np.float64)
    xi = np.zeros_like(xr)
    xr[..., a1, a2], xi[..., a1, a2] = re, im
    xr[..., a2, a1], xi[..., a2, a1] = re, -im           # (written second: the diagonal is zeroed below anyway)
    d = np.arange(n_ant)
    diag = v[..., [bl(a, a) for a in range(n_ant)], 0]
    xr[..., d, d] = 0.0
    xi[..., d, d] = 0.0
    return xr, xi, diag


def solve(vis, n_ant, model=None, flags=None, tol=1e-10, max_iter=200, ref_ant=-1, joint_pol=False, summer=osum):
    """-> (gains float64 [pol_out][freq][ant][2], info int32 [pol_out][freq][2] = iterations, status).  `summer(terms, axis)`
    replaces OSUM (the CPU test uses it to show that another association gives other bits)."""
    assert n_ant % 4 == 0 and 0 < n_ant <= MAX_ANT and max_iter >= 1 and tol >= 0
    xr, xi, diag = squares(vis, n_ant, joint_pol)
    n_po, n_f = xr.shape[:2]
    flagged = np.zeros(n_ant, bool) if flags is None else np.asarray(flags).astype(bool)
    live = ~flagged
    if ref_ant < 0:
        ref_ant = int(np.argmax(live)) if live.any() else -1
    else:
        assert ref_ant < n_ant and live[ref_ant]
    keep = live[:, None] & live[None, :]
    xr, xi = np.where(keep, xr, 0.0), np.where(keep, xi, 0.0)
    if model is not None:                                # x <- (x conj(s_p)) s_q
        s = np.asarray(model, np.float64).reshape(n_f, n_ant, 2)
        sr, si = s[..., 0], s[..., 1]
        tr, ti = _cmul(xr, xi, sr[None, :, :, None], -si[None, :, :, None])
        xr, xi = _cmul(tr, ti, sr[None, :, None, :], si[None, :, None, :])
    ok = live & (diag > 0)
    gr = np.where(ok, np.sqrt(np.where(ok, diag, 0).astype(np.float64)), 0.0)
    gi = np.zeros_like(gr)
    iters = np.zeros((n_po, n_f), np.int32)
    status = np.zeros((n_po, n_f), np.int32)
    active = np.ones((n_po, n_f), bool)
    off = (1.0 - np.eye(n_ant))[:, None, None, :]        # m * 1.0 is m, m * 0.0 is +0.0 (m is finite and not negative)
    # the squares with q in front, [q][pol_out][freq][p]: the sums over q then add whole contiguous slabs
    xr, xi = np.ascontiguousarray(np.moveaxis(xr, -1, 0)), np.ascontiguousarray(np.moveaxis(xi, -1, 0))
    by_q = lambda v: np.moveaxis(v, -1, 0)[..., None]    # noqa: E731  ([pol_out][freq][q] -> [q][pol_out][freq][1])
    for it in range(1, max_iter + 1):
        t0, t1 = _buf("t0", xr.shape), _buf("t1", xr.shape)
        np.subtract(np.multiply(xr, by_q(gr), out=t0), np.multiply(xi, by_q(gi), out=t1), out=t0)   # re(x g) = xr gr - xi gi
        nr = summer(t0, 0)
        np.add(np.multiply(xr, by_q(gi), out=t0), np.multiply(xi, by_q(gr), out=t1), out=t0)        # im(x g) = xr gi + xi gr
        ni = summer(t0, 0)
        den = summer(np.multiply(by_q(gr * gr + gi * gi), off, out=t0), 0)
        good = (den != 0) & live
        safe = np.where(good, den, 1.0)
        hr, hi = np.where(good, nr / safe, 0.0), np.where(good, ni / safe, 0.0)
        stop = np.zeros_like(active)
        if it % 2 == 0:
            hr, hi = 0.5 * (hr + gr), 0.5 * (hi + gi)
            dr, di = hr - gr, hi - gi
            delta, nu = summer(dr * dr + di * di, -1), summer(hr * hr + hi * hi, -1)
            stop = delta <= tol * tol * nu
        upd = active[..., None]
        gr, gi = np.where(upd, hr, gr), np.where(upd, hi, gi)
        iters[active] = it
        status[active & stop] = 1
        active = active & ~stop
        if not active.any():
            break
    if ref_ant >= 0:                                     # the phase reference
        rr, ri = gr[..., ref_ant], gi[..., ref_ant]
        m = np.sqrt(rr * rr + ri * ri)
        has = m > 0
        safe = np.where(has, m, 1.0)
        cr, ci = (rr / safe)[..., None], (-ri / safe)[..., None]
        tr, ti = _cmul(gr, gi, cr, ci)
        gr, gi = np.where(has[..., None], tr, gr), np.where(has[..., None], ti, gi)
    return np.stack([gr, gi], axis=-1), np.stack([iters, status], axis=-1)


def solve_slow(tri, n, s=None, flags=None, tol=1e-10, max_iter=200, ref_ant=-1):
    """ONE problem, element by element in Python floats: tri int64 [bl][2] (already summed over the polarisations if joint),
    s float64 [ant][2] or None.  -> (list of (re, im), iterations, status)."""
    fl = [False] * n if flags is None else [bool(f) for f in flags]
    x = [[(0.0, 0.0)] * n for _ in range(n)]
    for p in range(n):
        for q in range(n):
            if p == q or fl[p] or fl[q]:
                continue
            if q < p:
                v = (float(int(tri[bl(p, q)][0])), float(int(tri[bl(p, q)][1])))
            else:
                v = (float(int(tri[bl(q, p)][0])), -float(int(tri[bl(q, p)][1])))
            if s is not None:
                a, b = float(s[p][0]), -float(s[p][1])
                v = (v[0] * a - v[1] * b, v[0] * b + v[1] * a)
                a, b = float(s[q][0]), float(s[q][1])
                v = (v[0] * a - v[1] * b, v[0] * b + v[1] * a)
            x[p][q] = v

    def tree(terms):
        part = [0.0] * 64
        for i, t in enumerate(terms):                    # ascending i: l, l + 64, ... land on partial l in order
            part[i % 64] = part[i % 64] + t
        w = 32
        while w:
            part = [part[i] + part[i + w] for i in range(w)]
            w //= 2
        return part[0]

    g = []
    for p in range(n):
        d = int(tri[bl(p, p)][0])
        g.append((math.sqrt(float(d)), 0.0) if d > 0 and not fl[p] else (0.0, 0.0))
    it, status = 0, 0
    for it in range(1, max_iter + 1):
        h = []
        for p in range(n):
            num_r = tree([x[p][q][0] * g[q][0] - x[p][q][1] * g[q][1] for q in range(n)])
            num_i = tree([x[p][q][0] * g[q][1] + x[p][q][1] * g[q][0] for q in range(n)])
            den = tree([0.0 if q == p or fl[q] else g[q][0] * g[q][0] + g[q][1] * g[q][1] for q in range(n)])
            h.append((0.0, 0.0) if den == 0 or fl[p] else (num_r / den, num_i / den))
        if it % 2 == 0:
            h = [(0.5 * (a[0] + b[0]), 0.5 * (a[1] + b[1])) for a, b in zip(h, g)]
            delta = tree([(a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) for a, b in zip(h, g)])
            nu = tree([a[0] * a[0] + a[1] * a[1] for a in h])
            g = h
            if delta <= tol * tol * nu:
                status = 1
                break
        else:
            g = h
    if ref_ant < 0:
        live = [p for p in range(n) if not fl[p]]
        ref_ant = live[0] if live else -1
    if ref_ant >= 0:
        rr, ri = g[ref_ant]
        m = math.sqrt(rr * rr + ri * ri)
        if m > 0:
            cr, ci = rr / m, -ri / m
            g = [(a * cr - b * ci, a * ci + b * cr) for a, b in g]
    return g, it, status


def calibrate_weights(w, gains_layer, flags=None, mode=PHASE):
    """w int8 [freq][ant][beam][2], gains_layer float64 [freq][ant][2] -> int8 [freq][ant][beam][2]: w times conj(g) / |g|
    (PHASE), times k_f / |g| as well (FULL: k_f the smallest non-zero |g| among the unflagged antennas of the channel)."""
    w = np.asarray(w)
    g = np.asarray(gains_layer, np.float64)
    n_f, n_ant = g.shape[:2]
    assert w.dtype == np.int8 and w.shape[:2] == (n_f, n_ant) and w.shape[3] == 2 and mode in (PHASE, FULL)
    flagged = np.zeros(n_ant, bool) if flags is None else np.asarray(flags).astype(bool)
    gr, gi = g[..., 0], g[..., 1]
    m = np.sqrt(gr * gr + gi * gi)
    use = (m > 0) & ~flagged[None, :]
    safe = np.where(use, m, 1.0)
    cr, ci = gr / safe, -gi / safe
    if mode == FULL:
        k = np.min(np.where(use, m, np.inf), axis=1, keepdims=True)
        k = np.where(np.isfinite(k), k, 0.0)
        cr, ci = cr * (k / safe), ci * (k / safe)
    cr, ci = np.where(use, cr, 0.0)[..., None], np.where(use, ci, 0.0)[..., None]
    wr, wi = w[..., 0].astype(np.float64), w[..., 1].astype(np.float64)
    outr, outi = _cmul(wr, wi, cr, ci)
    out = np.stack([np.clip(np.rint(outr), -127, 127), np.clip(np.rint(outi), -127, 127)], axis=-1)
    return out.astype(np.int8)


def synth_vis(rng, n_ant, n_freq, n_pol, k=2.0 ** 20, model=None, noise=0, same_gains=False):
    """Visibilities of one point source at the visibility level: V = rint(K (g s)(g s)^H), |g| in 0.5 ... 1.5, random phases, made
    Hermitian from the lower triangle, plus integer noise.  same_gains: the polarisations share one set of gains (what a joint solve
    assumes).  -> (vis int64 [freq][pol][bl][2], g_true complex [pol][freq][ant])."""
    amp = rng.uniform(0.5, 1.5, size=(1 if same_gains else n_pol, n_freq, n_ant))
    g = np.repeat(amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape)), n_pol if same_gains else 1, axis=0)
    z = g if model is None else g * (np.asarray(model)[..., 0] + 1j * np.asarray(model)[..., 1])[None]
    a1, a2 = np.tril_indices(n_ant)
    v = k * z[..., a1] * np.conj(z[..., a2])             # [pol][freq][bl]
    vis = np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1).astype(np.int64)
    if noise:
        vis += rng.integers(-noise, noise + 1, size=vis.shape)
    vis[..., [bl(a, a) for a in range(n_ant)], 1] = 0
    return np.ascontiguousarray(vis.transpose(1, 0, 2, 3)), g
