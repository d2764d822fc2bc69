"""GPU tests (-m gpu) of the conditioning stage in front of the DM stage (include/dsabf.h: bf_cond_*; docs/CONDITIONING.md), through
the C-ABI.  The reference is tests/support/cond_oracle.py, a numpy restatement of the contract; everything the device writes is
compared with it bit for bit (.view(np.uint32): a -0.0 cannot hide)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cond_oracle  # noqa: E402
import cond_scenario  # noqa: E402
import dm_side  # noqa: E402
import sps_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
SENTINEL = np.uint32(0x7FC0DEAD)      # a NaN with a payload: nothing the stage computes has these bits
GUARD = 64                            # floats of sentinel in front of, between and behind the pushes' rows


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


@pytest.fixture(scope="module")
def hip():
    from dsabeamformer_amd import _lib

    return _lib._preload_hip_runtime()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def band(rng, n_rows, n_f, n_b):
    """Detected powers with a bandpass: positive, a different level in every channel."""
    gain = (1.0 + 3.0 * rng.random(n_f)).astype(np.float32)
    return ((rng.random((n_rows, n_f, n_b), dtype=np.float32) * np.float32(1e3) + np.float32(10.0)) * gain[None, :, None]).astype(np.float32)


def run_pushes(torch, hip, cond, orc, x, sizes):
    """x [T][f][b] through `cond` in pushes of `sizes` rows (cycled), alternating over two streams with no host synchronisation
    between the pushes; every push's rows lie in their own stretch of ONE sentinel-framed device buffer, and the mask of every push
    is copied aside on its stream (the next push's stream waits for that copy, on the device).  Output and mask of every push are
    compared with the oracle's afterwards, and the frame must be intact."""
    T, n_f, n_b = x.shape
    row = n_f * n_b
    cuts, at, k = [], 0, 0
    while at < T:
        n = min(sizes[k % len(sizes)], T - at)
        cuts.append((at, n))
        at, k = at + n, k + 1
    total = GUARD + sum(n * row + GUARD for _, n in cuts)
    host = np.full(total, SENTINEL, np.uint32)
    offs, o = [], GUARD
    for at, n in cuts:
        host[o:o + n * row] = bits(x[at:at + n]).reshape(-1)
        offs.append(o)
        o += n * row + GUARD
    d_buf = torch.from_numpy(host.view(np.int32)).cuda()
    d_masks = torch.full((len(cuts), n_f), 0x55, dtype=torch.uint8).cuda()
    p_mask = C.c_void_p()
    assert cond._lib.bf_cond_mask_device(cond._c, C.byref(p_mask)) == 0
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    prev_copy = None
    for k, ((at, n), o) in enumerate(zip(cuts, offs)):
        st = streams[k % 2]
        if prev_copy is not None:
            st.wait_event(prev_copy)             # (a device-side dependency: the mask is one buffer, the next push rewrites it)
        cond.push(d_buf.data_ptr() + 4 * o, n, st.cuda_stream)
        assert hip.hipMemcpyAsync(C.c_void_p(d_masks[k].data_ptr()), p_mask, C.c_size_t(n_f), 3, C.c_void_p(st.cuda_stream)) == 0
        prev_copy = torch.cuda.Event()
        prev_copy.record(st)
    torch.cuda.synchronize()
    got = d_buf.cpu().numpy().view(np.uint32)
    masks = d_masks.cpu().numpy()
    frame = np.ones(total, bool)
    for k, ((at, n), o) in enumerate(zip(cuts, offs)):
        want = orc.push(x[at:at + n])
        frame[o:o + n * row] = False
        assert np.array_equal(masks[k], orc.mask), (k, n, np.flatnonzero(masks[k] != orc.mask))
        bad = np.flatnonzero(got[o:o + n * row] != bits(want).reshape(-1))
        assert bad.size == 0, (k, n, bad.size, np.unravel_index(bad[0], want.shape))
    assert np.all(got[frame] == SENTINEL)
    return masks


SIZES = [1, 31, 32, 33, 65, 100]      # below, at and above a segment; two segments and one row; three and a ragged fourth
# (n_beams, n_freq_total, baseline_pushes, zero_dm, what): every n_beams (below a wave, ragged below and above one, four per lane),
# every n_freq_total, the window of 1, 2 and 3 pushes under 12 pushes (it wraps), zero-DM on and off.  260 and 516 beams: cond_totals_kernel
# walks the beams 256 at a time -- a second trip of 4 live lanes, and three trips (a lane of the zero-DM sums owns 9 beams); BASELINE config
# 5 has 512 beams.
CASES = [(4, 1, 1, True, "plain"), (4, 3, 2, False, "dead"), (4, 40, 3, True, "static"), (4, 300, 2, True, "dead"),
         (60, 1, 3, False, "plain"), (60, 3, 1, True, "dead"), (60, 40, 2, True, "all_masked"), (60, 300, 3, False, "static"),
         (64, 1, 2, True, "dead_cell"), (64, 3, 3, True, "static"), (64, 40, 1, False, "dead"), (64, 300, 2, True, "plain"),
         (68, 1, 1, False, "all_masked"), (68, 3, 2, True, "plain"), (68, 40, 3, True, "dead"), (68, 300, 1, False, "dead"),
         (256, 1, 3, True, "plain"), (256, 3, 1, False, "all_masked"), (256, 40, 2, False, "plain"), (256, 40, 3, True, "dead"),
         (256, 300, 3, True, "dead"), (256, 3, 2, True, "dead"),
         (260, 3, 2, True, "dead"), (260, 1, 3, False, "plain"), (516, 3, 1, True, "dead_cell"), (516, 1, 2, False, "dead")]


@pytest.mark.sweep_cap(26)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d-f%d-w%d-%s-%s" % (c[0], c[1], c[2], "zdm" if c[3] else "nozdm", c[4]))
def test_every_shape_to_the_bit(torch, bfmod, hip, case):
    """Output and mask of every push equal the oracle's, bit for bit.  "dead": a constant channel and an all-zero one (both masked:
    no variance, no mean) and a constant cell inside a live channel (+0.0f stored, the channel stays); "static": a caller's mask;
    "all_masked": every channel masked, n_good == 0."""
    from dsabeamformer_amd import api

    n_b, n_f, window, zero_dm, what = case
    assert len(CASES) <= 26 and {260, 516} <= {c[0] for c in CASES}
    rng = np.random.default_rng(1000 * n_b + 10 * n_f + window)
    T = sum(SIZES)
    x = band(rng, T, n_f, n_b)
    static = np.zeros(n_f, np.uint8)
    if what in ("dead", "dead_cell"):
        x[:, n_f // 2, n_b // 3] = np.float32(77.0)           # a dead cell inside a live channel
        if n_f >= 3 and what == "dead":
            x[:, 0, :] = np.float32(5.0)                       # constant: a mean, no variance
            x[:, n_f - 1, :] = np.float32(0.0)                 # all zero: no mean either
    if what == "static":
        static[::3] = 1
    if what == "all_masked":
        static[:] = 1
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    for rot in (0, 3):
        sizes = SIZES[rot:] + SIZES[:rot]
        cond = api.Conditioner(bf, n_f, max(SIZES), baseline_pushes=window, zero_dm=zero_dm, mask=static if static.any() else None)
        orc = cond_oracle.Conditioner(n_f, n_b, window, zero_dm, 0.0, static)
        masks = run_pushes(torch, hip, cond, orc, x, sizes + sizes)
        if what == "all_masked":
            assert masks.all()
        if what == "dead" and n_f >= 3:
            assert masks[:, 0].all() and masks[:, -1].all() and not masks[:, n_f // 2].all()   # (a window of ONE row has no variance anywhere)
        assert np.array_equal(cond.mask(), orc.mask)
        cond.close()
    bf.close()


def _two_level(n_f, n_b, levels):
    """One push of two rows: channel f is a - d, a + d in every beam -- mu = a, var = d^2, so q[f] = (d / a)^2 is what `levels` says,
    up to the roundings the oracle and the device share."""
    x = np.zeros((2, n_f, n_b), np.float32)
    for f, (a, d) in enumerate(levels):
        x[0, f, :], x[1, f, :] = np.float32(a - d), np.float32(a + d)
    return x


def test_auto_mask_and_medians(torch, bfmod, hip):
    """The automatic mask: the lower median with an even and an odd number of eligible channels, ties in q, mad == 0 (nothing beyond
    dead and static is masked), and the limit med + k mad hit from both sides by one ulp of q -- by tuning the threshold, which
    the host turns into k once, until the limit IS the q of a channel (not masked: only q > limit is) and its lower neighbour (masked)."""
    from dsabeamformer_amd import api

    n_b = 8
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    rng = np.random.default_rng(5)

    def both(x, thr, static=None, window=2):
        n_f = x.shape[1]
        cond = api.Conditioner(bf, n_f, x.shape[0], baseline_pushes=window, auto_threshold=thr, mask=static)
        orc = cond_oracle.Conditioner(n_f, n_b, window, True, thr, static)
        masks = run_pushes(torch, hip, cond, orc, x, [x.shape[0]])
        cond.close()
        return masks[-1]

    # ---- noise with three loud channels: found, whatever the parity of the eligible count (a static mask takes one away)
    for n_f in (40, 41):
        x = band(rng, 64, n_f, n_b)
        for f in (3, 20, 33):
            x[:, f, :] += (rng.gamma(0.5, 4000.0, 64).astype(np.float32))[:, None]
        for static in (None, np.eye(1, n_f, 7, dtype=np.uint8)[0]):
            m = both(x, 5.0, static)
            assert set(np.flatnonzero(m)) == {3, 20, 33} | ({7} if static is not None else set())
    # ---- 2049 channels: one more than the summary kernel keeps in LDS -- the medians then run over device memory
    x = band(rng, 16, 2049, n_b)
    for f in (0, 1000, 2048):
        x[:, f, :] += (rng.gamma(0.5, 4000.0, 16).astype(np.float32))[:, None]
    m = both(x, 6.0)                                   # (bit-equal to the oracle, mask included: checked in there)
    assert m.any() and not m.all()
    # ---- ties: pairs of channels with the same q, the median among them; one channel far out
    levels = [(100.0, 10.0), (100.0, 10.0), (200.0, 20.0), (100.0, 12.0), (100.0, 12.0), (100.0, 11.0), (100.0, 11.0), (100.0, 60.0)]
    m = both(_two_level(8, n_b, levels), 5.0)
    assert list(np.flatnonzero(m)) == [7]
    # ---- mad == 0: more than half of the channels share one q -- nothing is masked, however far out the others are
    levels = [(100.0, 10.0)] * 5 + [(100.0, 90.0), (100.0, 50.0), (50.0, 40.0)]
    m = both(_two_level(8, n_b, levels), 1.0)
    assert not m.any()
    m = both(_two_level(8, n_b, levels), 1.0, static=np.array([0, 0, 0, 0, 0, 0, 1, 0], np.uint8))
    assert list(np.flatnonzero(m)) == [6]
    # ---- the limit from both sides: find thresholds whose limit is exactly q[6] and exactly the double below it
    levels = [(100.0, 10.0), (100.0, 11.0), (100.0, 12.0), (100.0, 13.0), (100.0, 14.0), (100.0, 15.0), (100.0, 31.0)]
    x = _two_level(7, n_b, levels)
    S, Q = cond_oracle.push_totals(x)
    mu = S / 2.0
    var = Q / 2.0 - mu * mu
    cm, cv = cond_oracle.osum(mu) / n_b, cond_oracle.osum(var) / n_b
    q = cv / (cm * cm)
    med = cond_oracle.lower_median(q)
    mad = cond_oracle.lower_median(np.abs(q - med))
    target, below = q[6], np.nextafter(q[6], 0.0)
    found = {}
    lo = hi = (target - med) / mad / 1.4826
    for _ in range(20000):
        for t in (lo, hi):
            limit = med + (t * 1.4826) * mad
            if limit == target:
                found.setdefault("at", t)
            if limit == below:
                found.setdefault("below", t)
        if len(found) == 2:
            break
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    assert len(found) == 2, found
    assert list(np.flatnonzero(both(x, float(found["at"])))) == []          # q == limit: not masked
    assert list(np.flatnonzero(both(x, float(found["below"])))) == [6]      # q one ulp above the limit: masked
    bf.close()


# ---- behind the DM stage -------------------------------------------------------------------------------------------------------
DM_SIZES = [32, 1, 7, 32, 3, 19, 2, 32, 31, 11]
THRESHOLD, N_WIDTHS = 4.0, 3


@pytest.fixture(scope="module")
def ladder(orc):
    """A band of 24 channels x 64 beams, 150 rows, 12 trials (largest delay 20), cut into the ragged pushes of the DM stage's own
    test; conditioned by the oracle push by push (window 3, automatic mask, a static mask, zero-DM), then dedispersed whole."""
    rng = np.random.default_rng(21)
    n_t, n_f, n_b, n_dm, max_rows = 150, 24, 64, 12, 32
    x = (np.arange(n_f) / (n_f - 1.0)) ** 2
    delays = np.rint(20.0 * np.arange(n_dm)[:, None] / (n_dm - 1.0) * x[None, :]).astype(np.int32)
    D = int(delays.max())
    series = band(rng, n_t, n_f, n_b)
    series[:, 9, :] += rng.gamma(0.5, 4000.0, n_t).astype(np.float32)[:, None]
    static = np.zeros(n_f, np.uint8)
    static[2] = 1
    cuts, at, k = [], 0, 0
    while at < n_t:
        n = min(DM_SIZES[k % len(DM_SIZES)], n_t - at)
        cuts.append((at, n))
        at, k = at + n, k + 1
    kw = dict(baseline_pushes=3, zero_dm=True, auto_threshold=5.0)
    c = cond_oracle.Conditioner(n_f, n_b, mask=static, **kw)
    cooked = np.concatenate([c.push(series[a:a + n]) for a, n in cuts])
    return dict(n_t=n_t, n_f=n_f, n_b=n_b, n_dm=n_dm, max_rows=max_rows, delays=delays, D=D, series=series, static=static, cuts=cuts, kw=kw,
                cooked=cooked, want=orc.dedisperse_dm(cooked, delays, n_t - D), last_mask=c.mask.copy())


def test_behind_the_dm_stage(torch, bfmod, hip, orc, ladder):
    """Attached to a bf_dm_stream: with the zero-copy and the copy feed, the ring and the linear buffer, pushes alternating over two
    streams, every chunk is bit-equal to orc.dedisperse_dm of the oracle-conditioned series and the candidates of the attached
    search are sps_oracle's on those chunks (integers exactly; snr to 1e-9, the bound tests/test_gpu_sps.py derives for chunks of up
    to 250 times).  The copy feed leaves the caller's rows untouched.  Detached in mid-stream, the rows from there on are raw."""
    from dsabeamformer_amd import api

    L = ladder
    n_dm, n_b, n_f, D, max_rows = L["n_dm"], L["n_b"], L["n_f"], L["D"], L["max_rows"]
    row_bytes = n_f * n_b * 4
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    detach_at = 6                                   # the push in front of which the second pass detaches the conditioner
    mixed = np.concatenate([L["cooked"][:L["cuts"][detach_at][0]], L["series"][L["cuts"][detach_at][0]:]])
    want_mixed = orc.dedisperse_dm(mixed, L["delays"], L["n_t"] - D)
    for feed, ring, detach in (("reserve", 1, False), ("copy", 1, False), ("reserve", 0, False), ("copy", 0, False), ("reserve", 1, True), ("copy", 0, True)):
        bf.set_switch("dm_ring", ring)
        d_series = torch.from_numpy(L["series"]).cuda()
        dm = api.DmStream(bf, L["delays"], n_f, max_rows)
        cond = api.Conditioner(bf, n_f, max_rows, mask=L["static"], **L["kw"])
        sps = api.SinglePulseSearch(bf, n_dm, N_WIDTHS, max_rows, min_samples=16, threshold=THRESHOLD)
        dm.attach_conditioner(cond)
        dm.attach_search(sps)
        want = want_mixed if detach else L["want"]
        so = sps_oracle.Search(want, N_WIDTHS, min_samples=16, threshold=THRESHOLD)
        host = torch.full((n_dm * max_rows * n_b,), float("nan"), dtype=torch.float32).pin_memory()
        parts, n_cands = [], 0
        for k, (at, n) in enumerate(L["cuts"]):
            if detach and k == detach_at:
                dm.attach_conditioner(None)
            st = streams[k % 2]
            src = d_series.data_ptr() + at * row_bytes
            if feed == "reserve":
                dst = dm.reserve(n, st.cuda_stream)
                assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(n * row_bytes), 3, C.c_void_p(st.cuda_stream)) == 0
                src = dst
            first_t, n_out = dm.push(src, n, host, st.cuda_stream)
            assert (first_t, n_out) == (max(0, at - D), max(0, at + n - D) - max(0, at - D))
            if not n_out:
                continue
            st.synchronize()
            parts.append(host[:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b).copy())
            cands = sps.collect()
            sps_oracle.assert_candidates_equal(cands, so.push(n_out)["cands"], rtol=1e-9)
            n_cands += len(cands)
        torch.cuda.synchronize()
        got = np.concatenate(parts, axis=1)
        assert np.array_equal(bits(got), bits(want)), (feed, ring, detach)
        assert n_cands > 0
        if not detach:
            assert np.array_equal(cond.mask(), L["last_mask"]) and set(np.flatnonzero(L["last_mask"])) == {2, 9}
        if feed == "copy":
            assert np.array_equal(bits(d_series.cpu().numpy()), bits(L["series"]))     # the caller's rows stay raw
        sps.close()
        cond.close()
        dm.close()
    bf.set_switch("dm_ring", 1)
    bf.close()


def test_the_pulse_beats_the_interference(torch, bfmod, hip):
    """The scenario of tests/support/cond_scenario.py through reserve + push with the search attached: conditioned, the mask is
    exactly the three interference channels and the pulse is the best candidate by a factor 1.5 (the assertions of the CPU test);
    raw, the best candidate is not the pulse."""
    from dsabeamformer_amd import api

    sc = cond_scenario
    x, d = sc.make()
    D = int(d.max())
    row_bytes = sc.F * sc.B * 4
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=sc.B, n_freq=sc.F))
    d_x = torch.from_numpy(x).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = {}
    for conditioned in (True, False):
        dm = api.DmStream(bf, d, sc.F, sc.PUSH_ROWS)
        sps = api.SinglePulseSearch(bf, sc.N_DM, sc.N_WIDTHS, sc.PUSH_ROWS, min_samples=sc.MIN_SAMPLES, threshold=-1e300)
        cond = api.Conditioner(bf, sc.F, sc.PUSH_ROWS, baseline_pushes=sc.BASELINE_PUSHES, auto_threshold=sc.AUTO_THRESHOLD)
        if conditioned:
            dm.attach_conditioner(cond)
        dm.attach_search(sps)
        cands = []
        for k in range(sc.N_PUSHES):
            st = streams[k % 2]
            dst = dm.reserve(sc.PUSH_ROWS, st.cuda_stream)
            assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(d_x.data_ptr() + k * sc.PUSH_ROWS * row_bytes), C.c_size_t(sc.PUSH_ROWS * row_bytes), 3,
                                      C.c_void_p(st.cuda_stream)) == 0
            _, n_out = dm.push(dst, sc.PUSH_ROWS, None, st.cuda_stream)
            assert n_out == sc.chunk_sizes(d)[k]
            cands += [tuple(c) for c in sps.collect().tolist()]
        out[conditioned] = (cands, cond.mask() if conditioned else None)
        sps.close()
        cond.close()
        dm.close()
    bf.close()
    sc.check(out[True][0], d, out[True][1])
    raw = out[False][0]
    best = max(raw, key=lambda c: c[5])
    print("raw: best candidate", best, "the pulse's best %.3f" % max(c[5] for c in raw if sc.is_pulse(c, d)))
    assert not sc.is_pulse(best, d)


def test_invalid_arguments_and_lifetime(torch, bfmod, hip):
    from dsabeamformer_amd import _lib, api

    lib = _lib.load()
    n_f, n_b, max_rows = 5, 8, 4
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    other = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))

    def create(n_freq=n_f, rows=max_rows, baseline=8, thr=0.0, handle=bf._h, opt=True, out=True):
        o = _lib.BfCondOptions(baseline, 1, thr)
        c = C.c_void_p()
        rc = lib.bf_cond_create(handle, n_freq, rows, C.byref(o) if opt else None, C.byref(c) if out else None)
        assert (rc == 0) == bool(c.value)
        return rc, c

    for kw in (dict(n_freq=0), dict(rows=0), dict(baseline=0), dict(baseline=65), dict(thr=-1.0), dict(thr=float("nan")), dict(handle=None),
               dict(opt=False), dict(out=False)):
        assert create(**kw)[0] == BF_ERR_INVALID, kw
    for kw in (dict(baseline=64), dict(baseline=1, thr=0.5)):
        rc, c = create(**kw)
        assert rc == 0 and lib.bf_cond_destroy(c) == 0
    # ---- pushes that must launch nothing: the rows keep their sentinel
    cond = api.Conditioner(bf, n_f, max_rows)
    buf = torch.from_numpy(np.full((max_rows + 2) * n_f * n_b, SENTINEL, np.uint32).view(np.int32)).cuda()
    for args in ((cond._c, buf.data_ptr(), 0), (cond._c, buf.data_ptr(), max_rows + 1), (cond._c, buf.data_ptr(), -3), (cond._c, None, 1),
                 (None, buf.data_ptr(), 1)):
        assert lib.bf_cond_push(args[0], args[1], args[2], None) == BF_ERR_INVALID, args
    assert lib.bf_cond_set_mask(cond._c, None) == BF_ERR_INVALID and lib.bf_cond_mask_device(cond._c, None) == BF_ERR_INVALID
    torch.cuda.synchronize()
    assert np.all(buf.cpu().numpy().view(np.uint32) == SENTINEL)
    # ---- a mismatched attach
    delays = np.zeros((2, n_f), np.int32)
    dm = api.DmStream(bf, delays, n_f, max_rows)
    for bad, msg in ((api.Conditioner(bf, n_f + 1, max_rows), "channels"), (api.Conditioner(bf, n_f, max_rows - 1), "max_rows_per_push"),
                     (api.Conditioner(other, n_f, max_rows), "different handles")):
        with pytest.raises(bfmod.DsabfError, match=msg) as e:
            dm.attach_conditioner(bad)
        assert e.value.code == BF_ERR_INVALID
        bad.close()
    dm.attach_conditioner(cond)
    dm2 = api.DmStream(bf, delays, n_f, max_rows)
    with pytest.raises(bfmod.DsabfError, match="another DM stage") as e:
        dm2.attach_conditioner(cond)
    assert e.value.code == BF_ERR_STATE
    # ---- destroying an attached stage detaches it: the DM stage goes on, raw
    x = band(np.random.default_rng(3), 2 * max_rows, n_f, n_b)
    d_x = torch.from_numpy(x).cuda()
    host = torch.zeros(2 * max_rows * n_b, dtype=torch.float32).pin_memory()
    cond.close()
    assert dm.push(d_x, max_rows, host, 0) == (0, max_rows)
    torch.cuda.synchronize()
    got = host[:2 * max_rows * n_b].numpy().reshape(2, max_rows, n_b)
    want = np.zeros((max_rows, n_b), np.float32)
    for f in range(n_f):
        want = want + x[:max_rows, f, :]
    assert np.array_equal(bits(got[0]), bits(want))
    # ---- the handle destroyed before the stage: BF_ERR_STATE, and the stage can still be destroyed
    cond = api.Conditioner(bf, n_f, max_rows)
    dm.attach_conditioner(cond)
    bf.close()
    for call in (lambda: cond.push(d_x, 1, 0), lambda: cond.set_mask(np.zeros(n_f, np.uint8)), cond.mask, lambda: dm.attach_conditioner(None)):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE
    cond.close()
    dm.close()
    dm2.close()
    other.close()


def test_beam_cli_n_z(tmp_path):
    """`beam -j 29 -M 40 -N 4 -T 0.02 -n 3 -z -U 5 -F mask -v -w raw.bin -W dm.bin`: 25 burn-in reads + 4 analysed blocks of the
    production geometry (the window of 3 wraps at the fourth).  The -w file keeps the RAW stream; the oracle conditions it block by
    block (window 3, zero-DM, automatic mask, the file's static mask), and the oracle's dedispersion of that over the driver's delays
    must be the -W file bit for bit; the masked count the driver prints under -v is the oracle's for the last block."""
    from dsabeamformer_amd import build

    n_an, tsamp = 4, 0.02
    raw_file, dm_file, mask_file = tmp_path / "raw.bin", tmp_path / "dm.bin", tmp_path / "mask.txt"
    mask_file.write_text("# two channels\n7\n200  # and a comment\n")
    r = subprocess.run([build.BEAM, "-j", str(25 + n_an), "-M", "40", "-N", "4", "-T", str(tsamp), "-n", "3", "-z", "-U", "5", "-F", str(mask_file), "-v",
                        "-w", str(raw_file), "-W", str(dm_file)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    raw = dm_side.read_rows(raw_file)                                # [gemm][output][f][b]: rows in time order
    n_f, n_b = raw.shape[1], raw.shape[2]
    assert raw.shape[0] % n_an == 0 and (n_f, n_b) == (256, 256)
    # what `beam -M 40 -N 4 -T 0.02` computes (csrc/beam_main.cpp): the notebook's ladder, evenly picked
    _, _, delays = dm_side.beam_ladder(40.0, 4, n_f, tsamp)
    static = np.zeros(n_f, np.uint8)
    static[[7, 200]] = 1
    # (the conditioning push by push and the comparison: tests/support/dm_side.py, shared with tests/test_gpu_trial_split.py)
    cooked, c = dm_side.conditioned_rows(raw, raw.shape[0] // n_an, 3, True, 5.0, static)
    dm_side.check_dm_file(dm_file, cooked, delays)
    assert ("Conditioner: %d of %d channels masked in the last push" % (int(c.mask.sum()), n_f)) in r.stdout, r.stdout[-2000:]
    assert c.mask[7] and c.mask[200] and not c.mask.all()
