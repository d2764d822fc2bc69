"""CPU tests of the event builder (include/dsabf.h: bf_evt_*; docs/EVENTS.md section 1) against tests/support/evt_oracle.py, which
sees the WHOLE candidate list at once (all-pairs links, union-find, the record rules).  The library is fed the same list cut into
pushes: equality shows that the events do not depend on the cutting.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import evt_oracle as eo  # noqa: E402

BF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def api():
    from dsabeamformer_amd import build as b

    b.build()
    from dsabeamformer_amd import api as a

    return a


def feed_in_pushes(api, c, push_len, **options):
    """The list c through an EventBuilder in pushes of push_len samples: a candidate belongs to the push that holds the END of its
    boxcar (that is when the search reports it), next_t = the end of that push; empty pushes are fed too.  Returns (events in the
    order they left, the feed each left at -- the flush counts as one more)."""
    opt = dict(eo.DEFAULTS, **options)
    a1 = c["t_start"].astype(np.int64) + c["width"] - 1
    n_push = int(a1.max()) // push_len + 1 if len(c) else 0
    out, left_at = [], []
    with api.EventBuilder(**opt) as eb:
        for p in range(n_push):
            ev = eb.feed(c[a1 // push_len == p], (p + 1) * push_len)
            out.extend(ev)
            left_at.extend([p] * len(ev))
        ev = eb.flush()
        assert eb.open == 0
        out.extend(ev)
        left_at.extend([n_push] * len(ev))
    return out, left_at


def by_best(events):
    return sorted(events, key=lambda e: (int(e["best"]["t_start"]), int(e["best"]["dm"]), int(e["best"]["beam"])))


def check(api, rows, push_lens=(16, 50, 1000), **options):
    c = eo.candidates(rows)
    want = eo.events(c, **options)
    for push_len in push_lens:
        got, _ = feed_in_pushes(api, c, push_len, max_width=options.get("max_width", 8), **{k: v for k, v in options.items() if k != "max_width"})
        eo.assert_events_equal(by_best(got), want)
    return want


# rows: (t_start, dm, beam, width, snr)
def test_a_chain_is_one_event_though_its_ends_are_not_linked(api):
    rows = [(100, 5, 1, 4, 9.0), (104, 5, 2, 4, 12.0), (108, 5, 3, 4, 8.0)]           # t_tol 0: [100,103] [104,107] [108,111]
    c = eo.candidates(rows)
    link = eo.links(c, 1, 0)
    assert link[0, 1] and link[1, 2] and not link[0, 2]
    want = check(api, rows, t_tol=1, dm_tol=0)
    assert len(want) == 1 and want[0]["n_members"] == 3 and int(want[0]["best"]["beam"]) == 2 and (want[0]["t_lo"], want[0]["t_hi"]) == (100, 111)
    rows = [(100, 5, 1, 4, 9.0), (100, 6, 2, 4, 12.0), (100, 7, 3, 4, 8.0)]           # the same along the trials
    want = check(api, rows, t_tol=0, dm_tol=1)
    assert len(want) == 1 and (want[0]["dm_lo"], want[0]["dm_hi"]) == (5, 7)


@pytest.mark.parametrize("t_tol,dm_tol", [(0, 0), (3, 2), (7, 1)])
def test_tolerances_met_exactly_and_exceeded_by_one(api, t_tol, dm_tol):
    a = (100, 10, 0, 4, 9.0)                                                           # [100, 103]
    for gap, ddm, n_events in ((t_tol, dm_tol, 1), (t_tol + 1, dm_tol, 2), (t_tol, dm_tol + 1, 2), (t_tol + 1, dm_tol + 1, 2)):
        for sign in (1, -1):
            b = (103 + gap, 10 + sign * ddm, 1, 2, 8.0)                                # b0 = a1 + gap: linked iff gap <= t_tol
            want = check(api, [a, b], t_tol=t_tol, dm_tol=dm_tol)
            assert len(want) == n_events, (gap, ddm, sign)
            b = (100 - gap - 2 + 1, 10 + sign * ddm, 1, 2, 8.0)                        # b1 = a0 - gap, on the other side
            want = check(api, [b, a], t_tol=t_tol, dm_tol=dm_tol)
            assert len(want) == n_events, (gap, ddm, sign)


def test_a_cluster_spanning_three_pushes_and_fed_without_pause_stays_one_event(api):
    rows = [(10 + 6 * k, 3 + (k % 2), k % 5, 8, 7.0 + k) for k in range(8)]           # each overlaps the next: t 10 .. 59
    c = eo.candidates(rows)
    want = eo.events(c, max_width=8)
    assert len(want) == 1 and want[0]["n_members"] == 8
    got, left_at = feed_in_pushes(api, c, 20, max_width=8)
    assert len(set((c["t_start"] + c["width"] - 1) // 20)) == 3
    eo.assert_events_equal(got, want)
    assert left_at == [3]                                                              # nothing left before the cluster fell silent


@pytest.mark.parametrize("t_tol", [0, 5])
def test_the_closing_boundary(api, t_tol):
    """An event must NOT leave at the feed whose next_t - (max_width - 1) equals t_hi + t_tol, and must leave at the next one."""
    max_width = 16
    c = eo.candidates([(200, 4, 1, 8, 9.0)])                                           # t_hi = 207
    with api.EventBuilder(t_tol=t_tol, max_width=max_width) as eb:
        none = c[:0]
        assert len(eb.feed(c, 208)) == 0 and eb.open == 1
        assert len(eb.feed(none, 207 + t_tol + max_width - 1)) == 0 and eb.open == 1   # a candidate at t_start == t_hi + t_tol may still come
        ev = eb.feed(none, 207 + t_tol + max_width)
        assert len(ev) == 1 and eb.open == 0 and int(ev[0]["t_hi"]) == 207
    with api.EventBuilder(t_tol=t_tol, max_width=max_width) as eb:                     # ... and if it comes, it joins
        eb.feed(c, 208)
        late = eo.candidates([(207 + t_tol, 4, 2, 1, 5.0)])
        assert len(eb.feed(late, 207 + t_tol + max_width - 1)) == 0
        ev = eb.flush()
        assert len(ev) == 1 and int(ev[0]["n_members"]) == 2


def test_every_tie_rule_of_best(api):
    base = (100, 5, 3, 4, 9.0)
    for other, winner in (((100, 5, 3, 4, 9.5), 1), ((99, 5, 3, 4, 9.0), 1), ((101, 5, 3, 4, 9.0), 0), ((100, 4, 3, 4, 9.0), 1),
                          ((100, 6, 3, 4, 9.0), 0), ((100, 5, 2, 4, 9.0), 1), ((100, 5, 4, 4, 9.0), 0), ((100, 5, 3, 2, 9.0), 1),
                          ((100, 5, 3, 8, 9.0), 0)):
        for rows in ([base, other], [other, base]):
            want = check(api, rows)
            assert len(want) == 1
            w = (base, other)[winner]
            assert tuple(int(want[0]["best"][f]) for f in ("t_start", "dm", "beam", "width")) == w[:4] and want[0]["best"]["snr"] == w[4]


def test_the_incoherent_flags(api):
    IB = 7
    # only ib_beam members: best is the best of those
    want = check(api, [(100, 5, IB, 4, 9.0), (101, 5, IB, 4, 11.0)], ib_beam=IB)
    assert want[0]["flags"] == eo.IB_ONLY | eo.INCOHERENT and want[0]["n_beams"] == 0 and want[0]["snr_ib"] == 11.0 and want[0]["best"]["snr"] == 11.0
    # snr_ib equal to ib_ratio * snr: set; one ulp below: not
    want = check(api, [(100, 5, 1, 4, 10.0), (100, 5, IB, 4, 5.0)], ib_beam=IB, ib_ratio=0.5)
    assert want[0]["flags"] == eo.INCOHERENT and want[0]["n_beams"] == 1 and int(want[0]["best"]["beam"]) == 1
    want = check(api, [(100, 5, 1, 4, 10.0), (100, 5, IB, 4, float(np.nextafter(5.0, 0.0)))], ib_beam=IB, ib_ratio=0.5)
    assert want[0]["flags"] == 0 and want[0]["snr_ib"] < 5.0
    want = check(api, [(100, 5, 1, 4, 7.0), (100, 5, IB, 4, 7.0 * 0.3)], ib_beam=IB, ib_ratio=0.3)    # the product as the library forms it
    assert want[0]["flags"] == eo.INCOHERENT
    # a louder ib member is never `best`
    want = check(api, [(100, 5, 1, 4, 6.0), (100, 5, IB, 4, 60.0)], ib_beam=IB)
    assert int(want[0]["best"]["beam"]) == 1 and want[0]["snr_ib"] == 60.0 and want[0]["flags"] == eo.INCOHERENT
    # no ib member: snr_ib 0.0, not flagged
    want = check(api, [(100, 5, 1, 4, 6.0)], ib_beam=IB)
    assert want[0]["snr_ib"] == 0.0 and want[0]["flags"] == 0
    # ib_beam -1: that column is a beam like any other, and nothing is ever INCOHERENT
    want = check(api, [(100, 5, 1, 4, 6.0), (100, 5, IB, 4, 60.0)], ib_beam=-1)
    assert int(want[0]["best"]["beam"]) == IB and want[0]["n_beams"] == 2 and want[0]["flags"] == 0 and want[0]["snr_ib"] == 0.0


def test_wide_at_max_beams_and_one_more(api):
    for n_b, flag in ((3, 0), (4, eo.WIDE)):
        rows = [(100, 5, b, 4, 9.0 + b) for b in range(n_b)] + [(100, 5, 0, 2, 3.0), (100, 5, 200, 4, 1.0)]   # a beam twice; the ib column does not count
        want = check(api, rows, max_beams=3, ib_beam=200)
        assert want[0]["n_beams"] == n_b and want[0]["flags"] & eo.WIDE == flag and want[0]["n_members"] == n_b + 2
    want = check(api, [(100, 5, 0, 4, 9.0)], max_beams=0)
    assert want[0]["flags"] == eo.WIDE


def test_the_emission_order(api):
    """The events one call closes leave sorted by (best.t_start, best.dm, best.beam), whatever order their candidates came in."""
    rows = [(50, 30, 2, 2, 9.0), (50, 10, 9, 2, 9.0), (40, 20, 1, 2, 9.0), (50, 10 + 5, 3, 2, 9.0), (40, 0, 4, 2, 9.0), (60, 0, 0, 1, 9.0)]
    c = eo.candidates(rows)
    with api.EventBuilder(max_width=32) as eb:
        assert len(eb.feed(c, 61)) == 0
        ev = eb.flush()
    keys = [(int(e["best"]["t_start"]), int(e["best"]["dm"]), int(e["best"]["beam"])) for e in ev]
    assert keys == sorted(keys) and len(keys) == 6
    eo.assert_events_equal(ev, eo.events(c))


@pytest.mark.parametrize("ib_beam,n_beams", [(-1, 256), (255, 255)])
def test_a_storm_in_every_trial_and_beam_is_one_event(api, ib_beam, n_beams):
    """64 x 256 coincident candidates in one feed (the production ladder under interference): one event -- and no all-pairs loop
    (2.7e8 pairs would take this test out of the suite)."""
    import time

    rng = np.random.default_rng(5)
    d, b = np.divmod(np.arange(64 * 256), 256)
    c = eo.candidates([])
    c = np.zeros(64 * 256, c.dtype)
    c["t_start"], c["dm"], c["beam"], c["width"], c["peak"] = 1000 + rng.integers(0, 4, c.size), d, b, 1 << rng.integers(2, 5, c.size), 1.0
    c["snr"] = 8.0 + rng.random(c.size)
    c = c[rng.permutation(c.size)]
    with api.EventBuilder(ib_beam=ib_beam, max_width=16) as eb:
        t = time.perf_counter()
        assert len(eb.feed(c, 1024)) == 0
        dt = time.perf_counter() - t
        ev = eb.flush()
    print("bf_evt_feed, 16384 candidates: %.1f ms" % (1e3 * dt))
    assert len(ev) == 1 and int(ev[0]["n_members"]) == 16384 and int(ev[0]["n_beams"]) == n_beams
    coh = c[c["beam"] != ib_beam]
    best = coh[eo._best(coh, range(len(coh)))]
    assert ev[0]["best"] == best and (int(ev[0]["dm_lo"]), int(ev[0]["dm_hi"])) == (0, 63)
    assert int(ev[0]["flags"]) & eo.WIDE and int(ev[0]["t_lo"]) == int(c["t_start"].min())
    assert int(ev[0]["t_hi"]) == int((c["t_start"] + c["width"] - 1).max())
    assert ev[0]["snr_ib"] == (c["snr"][c["beam"] == ib_beam].max() if ib_beam >= 0 else 0.0)
    assert dt < 10.0                                                                   # (all pairs, 2.7e8 link tests, take far longer)


def test_random_candidates_do_not_depend_on_the_cutting(api):
    """2000 random candidates under four different cuttings (and as one push): identical events, equal to the oracle's."""
    rng = np.random.default_rng(11)
    n = 2000
    rows = [(int(t), int(d), int(b), int(w), float(s)) for t, d, b, w, s in zip(
        rng.integers(0, 6000, n), rng.integers(0, 24, n), rng.integers(0, 32, n), 1 << rng.integers(0, 6, n), np.round(6.0 + 6.0 * rng.random(n), 1))]
    opts = dict(t_tol=3, dm_tol=2, max_width=32, max_beams=2, ib_beam=31, ib_ratio=0.9)
    c = eo.candidates(rows)
    want = eo.events(c, **opts)
    assert 100 < len(want) < n and max(e["n_members"] for e in want) > 4 and len(set(e["flags"] for e in want)) >= 4
    for push_len in (40, 250, 977, 2048, 10 ** 6):
        got, left_at = feed_in_pushes(api, c, push_len, **opts)
        eo.assert_events_equal(by_best(got), want)
        if push_len < 2048:
            assert len(set(left_at)) > 5                                               # they leave as the stream goes, not at the flush


def test_every_refusal_and_null_handles(api):
    from dsabeamformer_amd import _lib

    lib = _lib.load()
    opt = _lib.BfEvtOptions()
    lib.bf_evt_default_options(C.byref(opt))
    assert (opt.t_tol, opt.dm_tol, opt.max_width, opt.max_beams, opt.ib_beam, opt.ib_ratio) == (0, 1, 128, 4, -1, 0.5)
    lib.bf_evt_default_options(None)
    for bad in (dict(t_tol=-1), dict(dm_tol=-1), dict(max_width=0), dict(max_beams=-1), dict(ib_ratio=float("nan")), dict(ib_ratio=-0.5)):
        with pytest.raises(_lib.DsabfError) as e:
            api.EventBuilder(**bad)
        assert e.value.code == BF_ERR_INVALID, bad
    with pytest.raises(TypeError):
        api.EventBuilder(no_such_option=1)
    e = C.c_void_p()
    assert lib.bf_evt_create(C.byref(opt), None) == BF_ERR_INVALID
    assert lib.bf_evt_create(None, C.byref(e)) == 0 and e.value                         # NULL options: the defaults
    n_out = C.c_size_t(99)
    c = eo.candidates([(10, 1, 1, 2, 9.0), (10, 40, 1, 2, 9.0)])
    out = np.zeros(4, api.event_dtype())
    assert lib.bf_evt_feed(None, c.ctypes.data, 2, 100, out.ctypes.data, 4, C.byref(n_out)) == BF_ERR_INVALID
    assert lib.bf_evt_feed(e, None, 2, 100, out.ctypes.data, 4, C.byref(n_out)) == BF_ERR_INVALID
    assert lib.bf_evt_feed(e, c.ctypes.data, 2, 100, out.ctypes.data, 4, None) == BF_ERR_INVALID
    assert lib.bf_evt_feed(e, c.ctypes.data, 2, 100, None, 4, C.byref(n_out)) == BF_ERR_INVALID
    assert lib.bf_evt_flush(None, out.ctypes.data, 4, C.byref(n_out)) == BF_ERR_INVALID
    assert lib.bf_evt_flush(e, out.ctypes.data, 4, None) == BF_ERR_INVALID
    assert lib.bf_evt_open(None) == BF_ERR_INVALID and lib.bf_evt_open(e) == 0
    assert lib.bf_evt_feed(e, c.ctypes.data, 2, 12, out.ctypes.data, 4, C.byref(n_out)) == 0 and n_out.value == 0 and lib.bf_evt_open(e) == 2
    # max_out too small: refused, nothing consumed -- the same call with room gives both events
    assert lib.bf_evt_feed(e, None, 0, 10 ** 6, out.ctypes.data, 1, C.byref(n_out)) == BF_ERR_INVALID and n_out.value == 0
    assert b"nothing was consumed" in lib.bf_last_error() and lib.bf_evt_open(e) == 2
    assert lib.bf_evt_flush(e, out.ctypes.data, 1, C.byref(n_out)) == BF_ERR_INVALID and lib.bf_evt_open(e) == 2
    assert lib.bf_evt_feed(e, None, 0, 10 ** 6, out.ctypes.data, 2, C.byref(n_out)) == 0 and n_out.value == 2 and lib.bf_evt_open(e) == 0
    assert [int(d) for d in out["best"]["dm"][:2]] == [1, 40]
    assert lib.bf_evt_destroy(e) == 0 and lib.bf_evt_destroy(None) == 0
    # the DM stage's new exports: NULL handles and pointers (no device is touched)
    u = C.c_uint64()
    s = C.c_void_p()
    st = (C.c_int32 * 1)()
    req = _lib.BfStampRequest(0, 0, 0)
    assert lib.bf_dm_stream_history(None, C.byref(u), C.byref(u), C.byref(u)) == BF_ERR_INVALID
    assert lib.bf_dm_stream_cut(None, C.byref(req), 1, 1, 1, 1, None, st, None) == BF_ERR_INVALID
    assert lib.bf_dm_stream_create_history(None, None, 1, 1, 1, 0, C.byref(s)) == BF_ERR_INVALID and not s.value
    assert lib.bf_dm_stream_create_history(None, None, 1, 1, 1, 0, None) == BF_ERR_INVALID


def test_the_lib_table_and_the_api_surface(api):
    from dsabeamformer_amd import _lib

    names = ["bf_evt_default_options", "bf_evt_create", "bf_evt_destroy", "bf_evt_feed", "bf_evt_flush", "bf_evt_open",
             "bf_dm_stream_create_history", "bf_dm_stream_history", "bf_dm_stream_cut"]
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert _lib.SIGNATURES["bf_evt_feed"][1][3] is C.c_uint64 and len(_lib.SIGNATURES["bf_dm_stream_cut"][1]) == 9
    assert C.sizeof(_lib.BfEvtEvent) == 80 == api.event_dtype().itemsize and C.sizeof(_lib.BfStampRequest) == 16 and C.sizeof(_lib.BfEvtOptions) == 32
    assert (api.EVT_IB_ONLY, api.EVT_WIDE, api.EVT_INCOHERENT) == (eo.IB_ONLY, eo.WIDE, eo.INCOHERENT) == (1, 2, 4)
    for cls, members in ((api.EventBuilder, ("feed", "flush", "open", "close")), (api.DmStream, ("history", "cut", "reserve", "push"))):
        for m in members:
            assert hasattr(cls, m), (cls, m)
    import inspect

    assert inspect.signature(api.DmStream.__init__).parameters["history_rows"].default == 0
    assert list(inspect.signature(api.DmStream.cut).parameters)[1:] == ["requests", "n_tau", "tbin", "fbin", "d_out", "stream"]
    header = open(os.path.join(ROOT, "include", "dsabf.h")).read()
    for n in names:
        assert n + "(" in header, n


# ---- the layers above: the `beam` command line and the two files ------------------------------------------------------------------
USAGE_ERRORS = [
    (["--events", "ev.txt"], "--events groups the candidates"),                                       # --events without -S
    (["-M", "250", "--events", "ev.txt"], "--events groups the candidates"),
    (["-M", "250", "-S", "6", "--stamps", "st.bin"], "give --events FILE"),                          # --stamps without --events
    (["-M", "250", "-S", "6", "--event-tol", "2"], "give --events FILE"),                            # the others without their parent
    (["-M", "250", "-S", "6", "--event-veto", "3"], "give --events FILE"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamp-shape", "32"], "give --stamps FILE"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamp-flagged"], "give --stamps FILE"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-tol", "-1"], "malformed or negative"),   # malformed or negative numbers
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-tol", "2,-1"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-tol", "2;1"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-tol", "x"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-veto", "-4"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-veto", "4:nan"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-veto", "4:-0.5"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--event-veto", "4:0.5x"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamps", "st.bin", "--stamp-shape", "0"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamps", "st.bin", "--stamp-shape", "64:-2"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamps", "st.bin", "--stamp-shape", "64:2:0"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamps", "st.bin", "--stamp-shape", "64:2:1:1"], "malformed or negative"),
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamps", "st.bin", "--stamp-shape", "64:2:3"], "does not divide the band"),   # FBIN
    (["-M", "250", "-S", "6", "--events", "ev.txt", "--stamps", "st.bin", "--stamp-shape", "64:2:512"], "does not divide the band"),
]


@pytest.mark.parametrize("args,message", USAGE_ERRORS, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_every_usage_error_comes_before_a_device_is_touched(api, tmp_path, args, message):
    import subprocess

    from dsabeamformer_amd import build

    r = subprocess.run([build.BEAM, "-j", "27"] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)
    assert "GPUassert" not in r.stderr and not os.listdir(tmp_path)            # no device was asked for, no file was created


def test_beam_H_lists_the_long_options_and_h_stays_the_references_text(api):
    import subprocess

    from dsabeamformer_amd import build

    big = subprocess.run([build.BEAM, "-H"], capture_output=True, text=True, timeout=60)
    small = subprocess.run([build.BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert big.returncode == 0 and small.returncode == 0
    for name in ("--events FILE", "--event-tol T[,D]", "--event-veto MAXBEAMS[:IB_RATIO]", "--stamps FILE", "--stamp-shape BINS[:TBIN[:FBIN]]", "--stamp-flagged"):
        assert name in big.stdout and name not in small.stdout, name
    assert big.stdout.startswith(small.stdout) and "--" not in small.stdout.replace("---", "")


WRITER = r"""
#include "dsabf_host.hpp"
int main(int argc, char** argv)
{
    dsabf::event_file_sink ev(argv[1]);
    dsabf::stamp_file_sink st(argv[2], 3, 5, 2);
    if (!ev.is_open() || !st.is_open()) return 2;
    bf_evt_event e[2] = {};
    e[0].best = {123456789012345ull, 7, 255, 32, 3.5f, 12.345678901234567};
    e[0].t_lo = 123456789012340ull; e[0].t_hi = 123456789012400ull; e[0].dm_lo = 5; e[0].dm_hi = 9; e[0].n_members = 16384; e[0].n_beams = 255;
    e[0].snr_ib = 1.0 / 3.0; e[0].flags = BF_EVT_WIDE | BF_EVT_INCOHERENT;
    e[1].best = {0, 0, 0, 1, -0.25f, 8.0};
    e[1].n_members = 1; e[1].n_beams = 1; e[1].flags = 0;
    if (!ev.deliver(e, 2) || !ev.deliver(e, 0)) return 3;
    float data[2][15];
    for (int k = 0; k < 15; k++) { data[0][k] = 1.0f / (float)(k + 1); data[1][k] = -(float)k; }
    if (!st.deliver(42, 7, 255, 16, 32, 12.345678901234567, data[0], 3, 5) || !st.deliver(0, 0, 0, 1, 1, 8.0, data[1], 3, 5)) return 4;
    if (st.deliver(0, 0, 0, 1, 1, 8.0, data[1], 5, 3)) return 5;   // another shape than the header's: refused
    return ev.get_events_written() == 2 && st.get_stamps_written() == 2 ? 0 : 6;
}
"""


def test_both_files_round_trip(api, tmp_path):
    """event_file_sink and stamp_file_sink (header-only, like sps_file_sink) written by a small C++ program, read by host.read_*."""
    import subprocess

    from dsabeamformer_amd import host

    src, exe = tmp_path / "writer.cpp", tmp_path / "writer"
    src.write_text(WRITER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ev_path, st_path = str(tmp_path / "ev.txt"), str(tmp_path / "st.bin")
    assert subprocess.run([str(exe), ev_path, st_path]).returncode == 0
    ev = host.read_event_file(ev_path)
    assert ev.dtype == api.event_dtype() and len(ev) == 2
    b = ev[0]["best"]
    assert (int(b["t_start"]), int(b["dm"]), int(b["beam"]), int(b["width"]), float(b["peak"]), float(b["snr"])) == (123456789012345, 7, 255, 32, 3.5, 12.345678901234567)
    assert (int(ev[0]["t_lo"]), int(ev[0]["t_hi"]), int(ev[0]["dm_lo"]), int(ev[0]["dm_hi"]), int(ev[0]["n_members"]), int(ev[0]["n_beams"])) == \
        (123456789012340, 123456789012400, 5, 9, 16384, 255)
    assert float(ev[0]["snr_ib"]) == 1.0 / 3.0 and int(ev[0]["flags"]) == api.EVT_WIDE | api.EVT_INCOHERENT
    assert float(ev[1]["best"]["peak"]) == -0.25 and int(ev[1]["flags"]) == 0 and int(ev[1]["best"]["t_start"]) == 0
    assert open(ev_path).readline().startswith("# t_start dm beam width snr peak n_members")
    hdr, stamps = host.read_stamp_file(st_path)
    assert (hdr["CONTENT"], hdr["DTYPE"], hdr["NFREQ_OUT"], hdr["NBINS"], hdr["FBIN"], hdr["LAYOUT"]) == ("stamps", "float32", "3", "5", "2", "freq,time")
    assert os.path.getsize(st_path) == 4096 + 2 * (32 + 4 * 15) and len(stamps) == 2
    s = stamps[0]
    assert (s["t0"], s["dm"], s["beam"], s["tbin"], s["width"], s["snr"]) == (42, 7, 255, 16, 32, 12.345678901234567)
    assert np.array_equal(s["data"], (np.float32(1) / np.arange(1, 16, dtype=np.float32)).reshape(3, 5))
    assert np.array_equal(stamps[1]["data"], -np.arange(15, dtype=np.float32).reshape(3, 5)) and stamps[1]["t0"] == 0


def test_both_files_round_trip_through_the_c_wrappers(api, tmp_path):
    """bfh_event_sink_* / bfh_stamp_sink_* (include/dsabf_host.h): the events an EventBuilder closed and two stamps, written from Python,
    come back from host.read_* unchanged; NULL arguments, an unwritable path and a stamp of another shape are refused."""
    from dsabeamformer_amd import _lib, host

    lib = _lib.load()
    rows = [(100 + 40 * k, 3 * k, k % 7, 1 << (k % 5), 6.5 + k / 3.0, 1.5 * k) for k in range(12)] + [(100, 1, 200, 4, 30.0, 2.0)]
    with api.EventBuilder(max_width=16, ib_beam=200) as eb:
        ev = np.concatenate([eb.feed(eo.candidates(rows), 700), eb.flush()])
    assert len(ev) >= 10 and len(set(int(f) for f in ev["flags"])) >= 2
    ev_path, st_path = str(tmp_path / "ev.txt"), str(tmp_path / "st.bin")
    s = C.c_void_p()
    assert lib.bfh_event_sink_create(None, C.byref(s)) == BF_ERR_INVALID and lib.bfh_event_sink_create(ev_path.encode(), None) == BF_ERR_INVALID
    assert lib.bfh_event_sink_create(b"/nonexistent/dir/ev.txt", C.byref(s)) == BF_ERR_INVALID and not s.value
    assert lib.bfh_event_sink_create(ev_path.encode(), C.byref(s)) == 0
    assert lib.bfh_event_sink_deliver(s, ev[:4].ctypes.data, 4) == 0 and lib.bfh_event_sink_deliver(s, None, 0) == 0
    assert lib.bfh_event_sink_deliver(s, None, 1) == BF_ERR_INVALID and lib.bfh_event_sink_deliver(None, ev.ctypes.data, 1) == BF_ERR_INVALID
    assert lib.bfh_event_sink_deliver(s, ev[4:].ctypes.data, len(ev) - 4) == 0
    assert lib.bfh_event_sink_destroy(s) == 0 and lib.bfh_event_sink_destroy(None) == 0
    back = host.read_event_file(ev_path)
    assert back.dtype == ev.dtype and len(back) == len(ev)
    for f in ("t_lo", "t_hi", "dm_lo", "dm_hi", "n_members", "n_beams", "snr_ib", "flags"):
        assert np.array_equal(back[f], ev[f]), f
    for f in ("t_start", "dm", "beam", "width", "peak", "snr"):
        assert np.array_equal(back["best"][f], ev["best"][f]), f
    t = C.c_void_p()
    for bad in ((None, 3, 5, 1), (st_path.encode(), 0, 5, 1), (st_path.encode(), 3, 0, 1), (st_path.encode(), 3, 5, 0), (b"/nonexistent/dir/st.bin", 3, 5, 1)):
        assert lib.bfh_stamp_sink_create(*bad, C.byref(t)) == BF_ERR_INVALID and not t.value, bad
    assert lib.bfh_stamp_sink_create(st_path.encode(), 3, 5, 2, C.byref(t)) == 0
    data = np.random.default_rng(2).standard_normal((2, 3, 5)).astype(np.float32)
    assert lib.bfh_stamp_sink_deliver(t, 2 ** 40 + 3, 63, 255, 16, 32, 9.25, data[0].ctypes.data, 3, 5) == 0
    assert lib.bfh_stamp_sink_deliver(t, 0, 0, 0, 1, 1, 4.0, data[1].ctypes.data, 5, 3) == -4                 # BF_ERR_STATE: not the header's shape
    assert lib.bfh_stamp_sink_deliver(t, 0, 0, 0, 1, 1, 4.0, None, 3, 5) == BF_ERR_INVALID
    assert lib.bfh_stamp_sink_deliver(t, 7, 1, 2, 1, 1, 4.0, data[1].ctypes.data, 3, 5) == 0
    assert lib.bfh_stamp_sink_destroy(t) == 0 and lib.bfh_stamp_sink_destroy(None) == 0
    hdr, stamps = host.read_stamp_file(st_path)
    assert (hdr["NFREQ_OUT"], hdr["NBINS"], hdr["FBIN"]) == ("3", "5", "2") and len(stamps) == 2
    assert [(s_["t0"], s_["dm"], s_["beam"], s_["tbin"], s_["width"], s_["snr"]) for s_ in stamps] == [(2 ** 40 + 3, 63, 255, 16, 32, 9.25), (7, 1, 2, 1, 1, 4.0)]
    assert np.array_equal(stamps[0]["data"].view(np.uint32), data[0].view(np.uint32)) and np.array_equal(stamps[1]["data"].view(np.uint32), data[1].view(np.uint32))
