"""The inputs of the pulse injector's GPU tests (tests/test_gpu_inj.py), made here so that tests/test_inj_cpu.py can hold the oracle
to its own conditions on exactly these inputs: that the order of two overlapping pulses shows in the bits, that the planted -0.0 and
NaN lie outside every window, that a train's bins are the folder's.  numpy only."""
import numpy as np

import inj_oracle

N_ROWS = 203
SIZES = [1, 7, 33, 64]               # cuts at rows 1, 8, 41, 105, 106, 113, 146
ONE = 1 << 64
NAN_BITS = np.uint32(0xFFC54321)     # a negative quiet NaN with a payload

# (n_beams, n_freq_total, W): between them every value of every axis
BURST_CASES = [(4, 1, 1), (60, 3, 7), (64, 40, 64), (68, 1, 257), (256, 3, 1), (260, 40, 7), (4, 40, 257), (60, 1, 64), (64, 3, 257),
               (68, 40, 1), (256, 40, 64), (260, 3, 7)]
# (n_beams, n_freq_total, n_bins, trains, the one train's model kind)
TRAIN_CASES = [(4, 1, 2, 1, "fast"), (60, 3, 5, 3, None), (64, 40, 64, 1, "slow"), (256, 3, 4096, 4, None), (260, 3, 5, 2, None),
               (68, 1, 64, 1, "still"), (64, 3, 4096, 1, "creep"), (256, 40, 64, 3, None)]


def wide(rng, shape, span=20):
    """N(0, 1) * 2^e, e uniform in -span .. span: sums of these round differently in another order."""
    return (rng.standard_normal(shape) * 2.0 ** rng.integers(-span, span + 1, shape)).astype(np.float32)


def cuts_of(n_rows, sizes):
    cuts, at, k = [], 0, 0
    while at < n_rows:
        n = min(sizes[k % len(sizes)], n_rows - at)
        cuts.append((at, n))
        at, k = at + n, k + 1
    return cuts


def response_of(rng, n_b):
    r = wide(rng, n_b, 3)
    r[1] = 0.0                       # a zero response: the add is made all the same
    return r


def plant(x, touched):
    """-0.0 in every beam of the first (row, channel) no window touches, the NaN in every beam of the last; returns the two places."""
    free = np.argwhere(~touched)
    assert len(free) >= 2
    a, b = tuple(free[0]), tuple(free[-1])
    x[a] = np.float32(-0.0)
    x[b].view(np.uint32)[:] = NAN_BITS
    return a, b


def burst_case(case):
    """x [203][f][b] and three bursts (t0, delay, profile, response), ids 0 1 2:
    0 starts exactly on the cut at row 105 (delay 0 in channel 0) and runs over the cut at 106 (W >= 2);
    1 shares 0's delays and starts (W - 1) // 2 rows earlier (W = 257: at row 8, so that rows 0 .. 7 stay free): the two overlap in
      cells, and from W = 3 it straddles the cuts at 105 and 106;
    2 runs off the end of the series, and its delay in channel n_f // 2 is larger than the whole series: never touched."""
    n_b, n_f, W = case
    rng = np.random.default_rng(1000 * n_b + 10 * n_f + W)
    x = wide(rng, (N_ROWS, n_f, n_b))
    d0 = rng.integers(0, 25, n_f).astype(np.int32)
    d0[0] = 0
    d2 = rng.integers(0, 25, n_f).astype(np.int32)
    d2[n_f // 2] = N_ROWS + 50
    bursts = [(105, d0, wide(rng, (n_f, W), 6), response_of(rng, n_b)),
              (max(8, 105 - (W - 1) // 2), d0.copy(), wide(rng, (n_f, W), 6), response_of(rng, n_b)),
              (N_ROWS - 1 - (W - 1) // 2, d2, wide(rng, (n_f, W), 6), response_of(rng, n_b))]
    planted = plant(x, touched_by(n_f, bursts))
    return dict(x=x, bursts=bursts, trains=[], planted=planted, max_width=max(W, 1))


def touched_by(n_f, bursts, trains=(), n_rows=N_ROWS):
    """bool [n_rows][f]: the (row, channel) pairs inside some window."""
    t = np.zeros((n_rows, n_f), bool)
    r = np.arange(n_rows)[:, None]
    for t0, delay, profile, _ in bursts:
        i = r - t0 - np.asarray(delay, np.int64)[None, :]
        t |= (i >= 0) & (i < profile.shape[1])
    for _, _, _, _, first, n in trains:
        t[first:(n_rows if n is None else min(n_rows, first + n))] = True
    return t


def models_for(n_tr, n_bins, n_rows, which):
    """The four kinds of model of tests/test_gpu_psr.py, as (phase0, dphase, ddphase, epoch_row): fast (bins are skipped, ddphase > 0),
    slow (about 30 rows per bin, ddphase < 0, the epoch in mid-series: negative n), still (one bin per channel), creep (three rows per bin)."""
    pool = {"fast": (int(0.1 * ONE), int(0.37 * ONE), 3 << 40, 0),
            "slow": (int(0.9 * ONE), ONE // (30 * n_bins), -(5 << 36), n_rows // 2),
            "still": (int(0.77 * ONE), 0, 0, -12),
            "creep": (ONE // 2, ONE // (3 * n_bins), 0, 7)}
    return [pool[k] for k in {1: (which,), 2: ("slow", "creep"), 3: ("fast", "slow", "still"), 4: ("fast", "slow", "still", "creep")}[n_tr]]


def train_case(case):
    """x and n_tr trains (model, delay, profile, response, first_row, n_rows) behind one burst (id 0) on the same cells.  Train k starts
    at row 10 + 3 k, inside the cut [8, 41); the odd ones end after 150 rows, inside the cut [146, 203); the even ones run to the end.
    The last train's delay in channel n_f // 2 is larger than the whole series (a negative oscillator index throughout).  Rows 0 .. 9 lie
    in front of every train and of the burst: the -0.0 and the NaN are planted in the first and the last (row, channel) there."""
    n_b, n_f, n_bins, n_tr, which = case
    rng = np.random.default_rng(7000 + 1000 * n_b + 10 * n_f + n_tr)
    x = wide(rng, (N_ROWS, n_f, n_b))
    models = models_for(n_tr, n_bins, N_ROWS, which)
    trains = []
    for k, m in enumerate(models):
        d = rng.integers(0, 25, n_f).astype(np.int32)
        if k == n_tr - 1:
            d[n_f // 2] = N_ROWS + 50
        trains.append((m, d, wide(rng, (n_f, n_bins), 6), response_of(rng, n_b), 10 + 3 * k, 150 if k % 2 else None))
    W = 7
    bursts = [(50, rng.integers(0, 25, n_f).astype(np.int32), wide(rng, (n_f, W), 6), response_of(rng, n_b))]
    touched = touched_by(n_f, bursts, trains)
    touched[10:] = True              # (plant in front of the trains only, also where a gated train leaves rows free behind it)
    planted = plant(x, touched)
    return dict(x=x, bursts=bursts, trains=trains, planted=planted, max_width=max(W, n_bins))


def expected(c, cuts=None, reverse=False):
    return inj_oracle.inject(c["x"], c["bursts"], c["trains"], cuts=cuts, reverse=reverse)


# ---- the scenario of "attached, and the point of it all": one burst in noise that the search must find --------------------------
FOUND = dict(T=640, n_f=16, n_b=8, n_dm=8, push=64, t0=301, trial=5, W=8, sigma=1.0, centre=3.5, fluence=6.0, beam=3, n_widths=5, threshold=8.0)


def found_case():
    s = dict(FOUND)
    s["x"] = np.random.default_rng(7).standard_normal((s["T"], s["n_f"], s["n_b"])).astype(np.float32)
    s["ladder"] = np.array([[d * (s["n_f"] - 1 - f) for f in range(s["n_f"])] for d in range(s["n_dm"])], np.int32)
    s["profile"] = inj_oracle.burst_profile(s["n_f"], s["W"], s["centre"], s["sigma"], s["fluence"])
    resp = np.zeros(s["n_b"], np.float32)
    resp[3], resp[4] = 1.0, 0.25
    s["response"] = resp
    s["burst"] = (s["t0"], s["ladder"][s["trial"]].copy(), s["profile"], resp)
    # the truth at the burst's own trial: the dedispersed pulse occupies output times t0 .. t0 + W - 1
    s["truth"] = [(s["t0"], s["t0"] + s["W"] - 1, s["trial"], s["beam"])]
    return s
