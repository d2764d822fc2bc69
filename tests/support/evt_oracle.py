"""Event oracle (docs/EVENTS.md section 1): the contract of bf_evt_* restated over the WHOLE candidate list at once -- all-pairs links,
a union-find, then the record rules.  The library is fed the same list cut into pushes; equality shows that the events do not depend
on the cutting."""
import numpy as np

IB_ONLY, WIDE, INCOHERENT = 1, 2, 4
DEFAULTS = dict(t_tol=0, dm_tol=1, max_width=128, max_beams=4, ib_beam=-1, ib_ratio=0.5)


def candidates(rows):
    """rows of (t_start, dm, beam, width, snr[, peak]) -> the structured array the library takes."""
    dt = np.dtype([("t_start", np.uint64), ("dm", np.int32), ("beam", np.int32), ("width", np.int32), ("peak", np.float32),
                   ("snr", np.float64)], align=True)
    out = np.zeros(len(rows), dt)
    for k, r in enumerate(rows):
        out[k] = (r[0], r[1], r[2], r[3], r[5] if len(r) > 5 else 1.0, r[4])
    return out


def links(c, t_tol, dm_tol):
    """[n][n] bool: A and B are linked (the three inequalities, as the issue states them)."""
    a0 = c["t_start"].astype(np.int64)
    a1 = a0 + c["width"].astype(np.int64) - 1
    dm = c["dm"].astype(np.int64)
    return (a0[:, None] <= a1[None, :] + t_tol) & (a0[None, :] <= a1[:, None] + t_tol) & (np.abs(dm[:, None] - dm[None, :]) <= dm_tol)


def components(link):
    n = len(link)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(np.triu(link, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    groups = {}
    for k in range(n):
        groups.setdefault(find(k), []).append(k)
    return list(groups.values())


def _best(c, idx):
    """Largest snr; ties: smaller t_start, dm, beam, width."""
    return min(idx, key=lambda k: (-float(c["snr"][k]), int(c["t_start"][k]), int(c["dm"][k]), int(c["beam"][k]), int(c["width"][k])))


def record(c, idx, opt):
    """One cluster (indices into c) -> the event as a dict."""
    ib = [k for k in idx if opt["ib_beam"] >= 0 and c["beam"][k] == opt["ib_beam"]]
    coh = [k for k in idx if k not in set(ib)]
    best = _best(c, coh if coh else ib)
    a0 = c["t_start"][idx].astype(np.int64)
    a1 = a0 + c["width"][idx].astype(np.int64) - 1
    n_beams = len(set(int(c["beam"][k]) for k in coh))
    snr_ib = max(float(c["snr"][k]) for k in ib) if ib else 0.0
    flags = 0
    if not coh:
        flags |= IB_ONLY
    if n_beams > opt["max_beams"]:
        flags |= WIDE
    if opt["ib_beam"] >= 0 and (not coh or snr_ib >= np.float64(opt["ib_ratio"]) * np.float64(c["snr"][best])):
        flags |= INCOHERENT
    return dict(best=c[best], t_lo=int(a0.min()), t_hi=int(a1.max()), dm_lo=int(c["dm"][idx].min()), dm_hi=int(c["dm"][idx].max()),
                n_members=len(idx), n_beams=n_beams, snr_ib=snr_ib, flags=flags)


def events(c, **options):
    """Every event of the candidate list c, sorted by (best.t_start, best.dm, best.beam)."""
    opt = dict(DEFAULTS, **options)
    if len(c) == 0:
        return []
    ev = [record(c, np.array(idx), opt) for idx in components(links(c, opt["t_tol"], opt["dm_tol"]))]
    return sorted(ev, key=lambda e: (int(e["best"]["t_start"]), int(e["best"]["dm"]), int(e["best"]["beam"])))


def assert_events_equal(got, want, snr_rtol=0.0):
    """got: the library's structured array(s); want: events().  Integers exactly; snr exactly unless snr_rtol says otherwise."""
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        for f in ("t_start", "dm", "beam", "width"):
            assert int(g["best"][f]) == int(w["best"][f]), (k, f, g, w)
        for f in ("t_lo", "t_hi", "dm_lo", "dm_hi", "n_members", "n_beams", "flags"):
            assert int(g[f]) == int(w[f]), (k, f, g, w)
        if snr_rtol:
            assert np.isclose(g["best"]["snr"], w["best"]["snr"], rtol=snr_rtol, atol=0) and np.isclose(g["snr_ib"], w["snr_ib"], rtol=snr_rtol, atol=0)
        else:
            assert g["best"]["snr"] == w["best"]["snr"] and g["snr_ib"] == w["snr_ib"] and g["best"]["peak"] == w["best"]["peak"], (k, g, w)
