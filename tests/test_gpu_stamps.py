"""GPU tests (-m gpu) of the stamps cut from the DM stage's ring (include/dsabf.h: bf_dm_stream_create_history, bf_dm_stream_history,
bf_dm_stream_cut; docs/EVENTS.md section 2), through the C-ABI.  The reference is tests/support/stamp_oracle.py: explicit np.float32
sequential sums over a series it holds whole.  Whole sentinel-filled outputs are compared bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cond_oracle  # noqa: E402
import dm_side  # noqa: E402
import stamp_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
SIZES = [8, 3, 8, 1, 7, 8, 5, 8, 2, 6]     # ragged pushes of at most 8 rows
MAX_ROWS, DMAX, HISTORY = 8, 7, 24


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


def make_ladder(n_dm, n_f, dmax=DMAX):
    """Trial 0: no delay anywhere; the last trial: the steepest, delays 0 .. dmax across the band."""
    x = (np.arange(n_f) / max(n_f - 1.0, 1.0)) ** 2
    d = np.rint(dmax * np.arange(n_dm)[:, None] / (n_dm - 1.0) * x[None, :]).astype(np.int32)
    assert not d[0].any() and d[-1].max() == dmax
    return d


def make_series(seed, n_t, n_f, n_b):
    rng = np.random.default_rng(seed)
    return (rng.random((n_t, n_f, n_b), dtype=np.float32) * np.float32(1e3) + np.float32(10.0)).astype(np.float32)


def cuts_of(n_t):
    out, at, k = [], 0, 0
    while at < n_t:
        n = min(SIZES[k % len(SIZES)], n_t - at)
        out.append((at, n))
        at, k = at + n, k + 1
    return out


class Feeder:
    """Rows of a device-resident series into a DmStream: the zero-copy feed (reserve, copy on the push's stream, push) on even pushes,
    the copy feed on odd ones."""

    def __init__(self, torch, hip, dm, series):
        self.hip, self.dm, self.row_bytes = hip, dm, series.shape[1] * series.shape[2] * 4
        self.d_series = torch.from_numpy(series).cuda()
        self.n = 0

    def reserve(self, at, n, stream):
        dst = self.dm.reserve(n, stream.cuda_stream)
        src = self.d_series.data_ptr() + at * self.row_bytes
        assert self.hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(n * self.row_bytes), 3, C.c_void_p(stream.cuda_stream)) == 0
        return dst

    def push(self, at, n, stream, host=None, reserved=None):
        src = self.d_series.data_ptr() + at * self.row_bytes
        if reserved is None and self.n % 2 == 0:
            reserved = self.reserve(at, n, stream)
        self.n += 1
        return self.dm.push(reserved if reserved is not None else src, n, host, stream.cuda_stream)


class Cuts:
    """Cuts issued without waiting for anything, each into a sentinel-filled output of its own; compared at the end."""

    def __init__(self, torch, dm, series, delays):
        self.torch, self.dm, self.series, self.delays, self.pending, self.n_cut = torch, dm, series, delays, [], 0

    def cut(self, reqs, n_tau, tbin, fbin, stream, what=""):
        oldest, nxt, _ = self.dm.history()
        want, st_want = so.cut(self.series, self.delays, reqs, n_tau, tbin, fbin, oldest, nxt)
        d_out = self.torch.from_numpy(np.full(want.shape, so.SENTINEL, np.uint32).view(np.int32)).cuda()
        st = self.dm.cut(reqs, n_tau, tbin, fbin, d_out, stream.cuda_stream)
        assert list(st) == list(st_want), (what, reqs, list(st), list(st_want), (oldest, nxt))
        self.pending.append((d_out, want, (what, reqs, n_tau, tbin, fbin, oldest, nxt)))
        self.n_cut += int((st == 0).sum())
        return st

    def compare(self):
        self.torch.cuda.synchronize()
        for d_out, want, what in self.pending:
            got = d_out.cpu().numpy().view(np.uint32)
            bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            assert bad.size == 0, (what, bad.size, np.unravel_index(bad[0], want.shape))
        self.pending = []


def edge_requests(delays, oldest, nxt, cap, n_tau, tbin, beams):
    """The zero-delay and the steepest trial; a window that begins exactly at oldest_row, one that ends exactly at next_row, each moved by
    one row (status 1 and 2), and one across the ring's seam.  Returns (requests, the seam was crossed)."""
    steep, b = len(delays) - 1, list(beams)
    reqs, seam = [], False
    for k, dm in enumerate((steep, 0)):
        sp = so.span(delays, dm, n_tau, tbin)
        reqs.append((oldest, dm, b[k % len(b)]))
        if oldest > 0:
            reqs.append((oldest - 1, dm, b[(k + 1) % len(b)]))
        if nxt >= sp:
            reqs.append((nxt - sp, dm, b[(k + 2) % len(b)]))
            reqs.append((nxt - sp + 1, dm, b[k % len(b)]))
        t0 = nxt // cap * cap - 3
        if t0 >= max(oldest, 1) and t0 + sp <= nxt and sp > 3:
            reqs.append((t0, dm, b[(k + 1) % len(b)]))
            seam = True
    return reqs, seam


# (n_tau, tbin, fbin) of the cuts in the wrapping ring: windows of at most cap_rows - 3 max_rows rows
WRAP_SHAPES = [(1, 1, 1), (7, 1, 1), (7, 2, 2), (7, 5, 64), (5, 3, 2), (7, 1, 64), (1, 5, 1), (16, 2, 1)]


def test_the_wrapping_ring_to_the_bit(torch, bfmod, hip):
    """64 channels x 256 beams: a row is 64 KiB (cap_rows is read from the stage: it depends on the device's granule).  Ragged pushes
    of at most 8 rows alternate over two streams and the two feeds until the ring has wrapped three times; after every third push a
    cut goes out on a third stream, with nothing waited for in between.  One cut has 33 requests (two launches), one has one, one none."""
    from dsabeamformer_amd import api

    n_f, n_b, n_dm = 64, 256, 4
    delays = make_ladder(n_dm, n_f)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    dm = api.DmStream(bf, delays, n_f, MAX_ROWS, history_rows=HISTORY)
    oldest, nxt, cap = dm.history()
    assert (oldest, nxt) == (0, 0) and cap >= DMAX + 3 * MAX_ROWS + HISTORY
    print("cap_rows", cap)
    n_t = 3 * cap + 40
    series = make_series(1, n_t, n_f, n_b)
    feed, cuts = Feeder(torch, hip, dm, series), Cuts(torch, dm, series, delays)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    s_cut = torch.cuda.Stream()
    torch.cuda.synchronize()
    seams = n_old = n_new = n_reserved = 0
    for k, (at, n) in enumerate(cuts_of(n_t)):
        st = streams[k % 2]
        if k % 7 == 5 and at >= cap:
            # a reservation outstanding: its producer is already overwriting the oldest rows
            before = dm.history()
            dst = feed.reserve(at, n, st)
            now = dm.history()
            assert now == (before[0] + n, before[1], cap) and before[0] == at - cap
            got = cuts.cut([(before[0], 0, 131), (before[0] + n - 1, 0, 0), (now[0], 0, 255)], 3, 2, 2, s_cut, "reserved")
            assert list(got) == [1, 1, 0]
            n_reserved += 1
            feed.push(at, n, st, reserved=dst)
        else:
            feed.push(at, n, st)
        oldest, nxt, _ = dm.history()
        assert (oldest, nxt) == (max(0, at + n - cap), at + n)
        if k % 3 != 2:
            continue
        n_tau, tbin, fbin = WRAP_SHAPES[(k // 3) % len(WRAP_SHAPES)]
        reqs, seam = edge_requests(delays, oldest, nxt, cap, n_tau, tbin, (0, 131, 255))
        if k // 3 == 9:
            reqs = (reqs * 33)[:33]
        if k // 3 == 10:
            reqs = reqs[:1]
        if k // 3 == 11:
            reqs = []
        got = cuts.cut(reqs, n_tau, tbin, fbin, s_cut, "push %d" % k)
        seams += seam
        n_old += int((got == 1).sum())
        n_new += int((got == 2).sum())
    assert dm.history()[1] == n_t and n_t // cap >= 3                  # the ring has wrapped at least three times
    cuts.compare()
    print("stamps cut", cuts.n_cut, "too old", n_old, "not yet", n_new, "across the seam", seams, "under a reservation", n_reserved)
    assert cuts.n_cut > 60 and n_old > 10 and n_new > 10 and seams >= 3 and n_reserved >= 3
    dm.close()
    bf.close()


# (n_f, n_b, cuts (n_tau, tbin, fbin)): a history that holds the whole series -- no wrap; every n_tau, tbin and fbin
SMALL = [(3, 4, [(1, 1, 1), (7, 5, 3), (64, 2, 1), (65, 3, 3), (130, 1, 1), (130, 2, 3)]),
         (8, 8, [(1, 1, 8), (7, 5, 2), (64, 2, 8), (65, 3, 1), (130, 1, 2), (130, 2, 1), (64, 1, 1)])]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "f%d-b%d" % (c[0], c[1]))
def test_small_rows(torch, bfmod, hip, case):
    """3 channels x 4 beams, 8 x 8: lanes beyond n_tau, one lane, more than a wave of output times, a workgroup with idle frequency groups."""
    from dsabeamformer_amd import api

    n_f, n_b, shapes = case
    n_dm, n_t = 3, 300
    delays = make_ladder(n_dm, n_f)
    series = make_series(10 * n_f + n_b, n_t, n_f, n_b)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    dm = api.DmStream(bf, delays, n_f, MAX_ROWS, history_rows=n_t)
    cap = dm.history()[2]
    assert cap > n_t
    feed, cuts = Feeder(torch, hip, dm, series), Cuts(torch, dm, series, delays)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    s_cut = torch.cuda.Stream()
    torch.cuda.synchronize()
    beams = (0, n_b // 2 + 1, n_b - 1)
    all_cuts = cuts_of(n_t)
    for k, (at, n) in enumerate(all_cuts):
        feed.push(at, n, streams[k % 2])
        if k % 9 == 8 or k == len(all_cuts) - 1:
            for n_tau, tbin, fbin in shapes:
                reqs, _ = edge_requests(delays, 0, at + n, cap, n_tau, tbin, beams)
                reqs += [(at // 2, d, b) for d in range(n_dm) for b in beams]
                cuts.cut(reqs, n_tau, tbin, fbin, s_cut, "push %d" % k)
    assert dm.history() == (0, n_t, cap)
    cuts.compare()
    print("stamps cut", cuts.n_cut)
    assert cuts.n_cut > 100
    dm.close()
    bf.close()


def test_behind_a_conditioner_the_stamp_shows_what_the_search_saw(torch, bfmod, hip):
    """Stamps equal the stamp oracle over cond_oracle's rows -- not over the raw rows (asserted: the two differ)."""
    from dsabeamformer_amd import api

    n_t, n_f, n_b, n_dm = 120, 24, 64, 5
    delays = make_ladder(n_dm, n_f)
    series = make_series(3, n_t, n_f, n_b) * (1.0 + 3.0 * np.random.default_rng(4).random(n_f)).astype(np.float32)[None, :, None]
    static = np.zeros(n_f, np.uint8)
    static[2] = 1
    kw = dict(baseline_pushes=3, zero_dm=True, auto_threshold=0.0)
    oracle = cond_oracle.Conditioner(n_f, n_b, mask=static, **kw)
    cooked = np.ascontiguousarray(np.concatenate([oracle.push(series[a:a + n]) for a, n in cuts_of(n_t)]), np.float32)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    dm = api.DmStream(bf, delays, n_f, MAX_ROWS, history_rows=n_t)       # (the whole series stays readable)
    cond = api.Conditioner(bf, n_f, MAX_ROWS, mask=static, **kw)
    dm.attach_conditioner(cond)
    cap = dm.history()[2]
    assert cap > n_t
    feed, cuts = Feeder(torch, hip, dm, series), Cuts(torch, dm, cooked, delays)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    s_cut = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k, (at, n) in enumerate(cuts_of(n_t)):
        feed.push(at, n, streams[k % 2])
        if k % 4 == 3:
            reqs, _ = edge_requests(delays, 0, at + n, cap, 9, 2, (0, 33, 63))
            cuts.cut(reqs, 9, 2, 2, s_cut, "push %d" % k)             # the newest rows: conditioned by the push just queued
    reqs = [(10, d, b) for d in (0, n_dm - 1) for b in (0, 33, 63)]
    assert not cuts.cut(reqs, 40, 2, 1, s_cut).any()
    raw, _ = so.cut(series, delays, reqs, 40, 2, 1, 0, n_t)
    assert not np.array_equal(raw, cuts.pending[-1][1])
    cuts.compare()
    assert cuts.n_cut > 20
    cond.close()
    dm.close()
    bf.close()


def test_a_producer_queued_behind_a_cut_does_not_overwrite_what_it_reads(torch, bfmod, hip, orc):
    """One queue is kept busy for tens of milliseconds with matrix products and a cut of the whole readable range is queued behind them.
    On another queue, enough reserve / write / push rounds follow at once to overwrite every row of the ring.  The cut still equals the
    oracle, and the chunks of those pushes still equal dedisperse_dm over the series."""
    from dsabeamformer_amd import api

    n_f, n_b, n_dm = 64, 256, 4
    delays = make_ladder(n_dm, n_f)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    dm = api.DmStream(bf, delays, n_f, MAX_ROWS, history_rows=HISTORY)
    cap = dm.history()[2]
    n_first = (cap + 16) // MAX_ROWS * MAX_ROWS                          # the ring is full and has wrapped
    n_after = (cap + MAX_ROWS - 1) // MAX_ROWS + 1                       # pushes of 8 rows that overwrite all of it
    n_t = n_first + n_after * MAX_ROWS
    series = make_series(2, n_t, n_f, n_b)
    want_chunks = orc.dedisperse_dm(series, delays, n_t - DMAX)
    feed, cuts = Feeder(torch, hip, dm, series), Cuts(torch, dm, series, delays)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.randn((8192, 8192), device="cuda")
    hosts = [torch.full((n_dm * MAX_ROWS * n_b,), float("nan"), dtype=torch.float32).pin_memory() for _ in range(n_first // MAX_ROWS + n_after)]
    emitted = []
    for k in range(n_first // MAX_ROWS):
        emitted.append(feed.push(k * MAX_ROWS, MAX_ROWS, s2, hosts[k]))
    torch.cuda.synchronize()
    oldest, nxt, _ = dm.history()
    assert (oldest, nxt) == (n_first - cap, n_first)
    with torch.cuda.stream(s1):
        for _ in range(4):
            torch.mm(big, big)
    tbin = 2
    n_tau = (nxt - oldest - DMAX) // tbin
    reqs = [(oldest, n_dm - 1, 0), (oldest, 0, 131), (nxt - so.span(delays, 0, n_tau, tbin), 0, 255), (oldest + (nxt - oldest - DMAX) % tbin, n_dm - 1, 255)]
    got = cuts.cut(reqs, n_tau, tbin, 1, s1, "behind the busy queue")     # runs when s1 gets to it
    assert list(got) == [0, 0, 0, 0]
    for k in range(n_first // MAX_ROWS, n_first // MAX_ROWS + n_after):  # at once, on the idle queue
        emitted.append(feed.push(k * MAX_ROWS, MAX_ROWS, s2, hosts[k]))
    assert dm.history()[0] >= nxt                                        # every row the cut reads has a new owner
    cuts.compare()
    for k, (first_t, n_out) in enumerate(emitted):
        assert (first_t, n_out) == (max(0, k * MAX_ROWS - DMAX), MAX_ROWS - (DMAX if k == 0 else 0))
        chunk = hosts[k][:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b)
        assert np.array_equal(bits(chunk), bits(want_chunks[:, first_t:first_t + n_out])), k
    dm.close()
    bf.close()


def test_no_change_when_off_and_every_refusal(torch, bfmod, hip, orc):
    """The same pushes through bf_dm_stream_create and bf_dm_stream_create_history(..., 0): bit-equal chunks, the same cap_rows.  The linear
    buffer keeps no history: creation succeeds, a cut answers BF_ERR_STATE.  So does a stage whose handle went first.  Every BF_ERR_INVALID."""
    from dsabeamformer_amd import _lib, api

    lib = _lib.load()
    n_f, n_b, n_dm, n_t = 24, 64, 5, 90
    delays = make_ladder(n_dm, n_f)
    series = make_series(7, n_t, n_f, n_b)
    want = orc.dedisperse_dm(series, delays, n_t - DMAX)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    st = torch.cuda.Stream()
    host = torch.full((n_dm * MAX_ROWS * n_b,), float("nan"), dtype=torch.float32).pin_memory()
    caps = []
    for how in ("create", "history 0"):
        dm = api.DmStream(bf, delays, n_f, MAX_ROWS)
        if how == "history 0":
            dm.close()
            assert lib.bf_dm_stream_create_history(bf._h, delays.ctypes.data, n_dm, n_f, MAX_ROWS, 0, C.byref(dm._s)) == 0
        caps.append(dm.history()[2])
        feed, parts = Feeder(torch, hip, dm, series), []
        for at, n in cuts_of(n_t):
            first_t, n_out = feed.push(at, n, st, host)
            st.synchronize()
            parts.append(host[:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b).copy())
        assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(want)), how
        if how == "create":
            dm.close()
    assert caps[0] == caps[1]
    # every BF_ERR_INVALID: nothing is launched, the output stays as it was
    d_out = torch.from_numpy(np.full((2, n_f, 4), so.SENTINEL, np.uint32).view(np.int32)).cuda()
    status = np.full(2, -7, np.int32)
    reqs = np.zeros(2, api.stamp_request_dtype())
    reqs["t0"], reqs["dm"], reqs["beam"] = 70, 1, 3                      # (readable in the smallest ring: rows 59 .. 89)

    def cut(r=reqs, n_req=2, n_tau=4, tbin=1, fbin=1, out=d_out.data_ptr(), stat=status.ctypes.data, s=None):
        return lib.bf_dm_stream_cut(dm._s if s is None else s, r.ctypes.data if r is not None else None, n_req, n_tau, tbin, fbin, out, stat, st.cuda_stream)

    for bad in (dict(n_tau=0), dict(tbin=0), dict(fbin=0), dict(fbin=5), dict(fbin=48), dict(n_req=-1), dict(r=None), dict(out=None), dict(stat=None),
                dict(n_tau=-3), dict(tbin=-1)):
        assert cut(**bad) == BF_ERR_INVALID, bad
    for field, value in (("dm", -1), ("dm", n_dm), ("beam", -1), ("beam", n_b)):
        r = reqs.copy()
        r[field][1] = value
        assert cut(r=r) == BF_ERR_INVALID and field.encode() in lib.bf_last_error().replace(b"trial", b"dm"), (field, value)
    s = C.c_void_p()
    assert lib.bf_dm_stream_create_history(bf._h, delays.ctypes.data, n_dm, n_f, MAX_ROWS, -1, C.byref(s)) == BF_ERR_INVALID and not s.value
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy().view(np.uint32) == so.SENTINEL) and np.all(status == -7)
    assert cut() == 0 and list(status) == [0, 0]                         # ... and the same call, valid
    assert cut(n_req=0, r=None, out=None, stat=None) == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[0], bits(so.stamp(series, delays, 70, 1, 3, 4, 1, 1))) and np.array_equal(got[0], got[1])
    dm.close()
    # the linear buffer keeps no history
    bf.set_switch("dm_ring", 0)
    lin = api.DmStream(bf, delays, n_f, MAX_ROWS, history_rows=HISTORY)
    bf.set_switch("dm_ring", 1)
    Feeder(torch, hip, lin, series).push(0, MAX_ROWS, st)
    oldest, nxt, _ = lin.history()
    assert oldest == nxt == MAX_ROWS
    assert cut(s=lin._s) == BF_ERR_STATE and b"linear" in lib.bf_last_error()
    # a stage whose handle was destroyed first
    ring = api.DmStream(bf, delays, n_f, MAX_ROWS, history_rows=HISTORY)
    Feeder(torch, hip, ring, series).push(0, MAX_ROWS, st)
    torch.cuda.synchronize()
    bf.close()
    u = C.c_uint64()
    assert cut(s=ring._s) == BF_ERR_STATE and cut(s=lin._s) == BF_ERR_STATE
    assert lib.bf_dm_stream_history(ring._s, C.byref(u), C.byref(u), C.byref(u)) == BF_ERR_STATE
    ring.close()
    lin.close()


def test_beam_cli_events_and_stamps_end_to_end(tmp_path):
    """`beam -j 33 -M 250 -N 8 -S 4 -B 6 -i 255 -w det.bin -W dm.bin -C cands.txt --events ev.txt --stamps st.bin` (no conditioner): 25
    burn-in reads + 8 analysed blocks.  ev.txt equals the event oracle over cands.txt (snr to 1e-9, as the candidates' own test); the
    log reports stamps_missed 0; events whose window passes the last row of the run (2048 rows: a width-32 stamp spans 1024) cannot be
    cut and are reported as such, their number recomputed from the requests; the set of stamps is the one the selection rule picks from the events of every deliver (recomputed,
    stamps_dropped included); every stamp is bit-equal to the stamp oracle over the rows of det.bin."""
    import subprocess

    from dsabeamformer_amd import build

    names = ("det.bin", "dm.bin", "cands.txt", "ev.txt", "st.bin")
    det_file, dm_file, cand_file, ev_file, st_file = (str(tmp_path / n) for n in names)
    r = subprocess.run([build.BEAM, "-j", "33", "-M", "250", "-N", "8", "-S", "4", "-B", "6", "-i", "255", "-w", det_file, "-W", dm_file, "-C", cand_file,
                        "--events", ev_file, "--stamps", st_file], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    opts = dict(max_width=32, ib_beam=255)
    # (the comparisons themselves: tests/support/dm_side.py, shared with the trial-split runs of tests/test_gpu_trial_split.py)
    cands, want = dm_side.check_events(ev_file, cand_file, **opts)
    print("candidates", len(cands), "events", len(want))
    assert len(want) >= 1
    # the rows the ring held: det.bin (there is no conditioner), and the driver's ladder -- dm.bin is the oracle's over both
    series = dm_side.read_rows(det_file)
    _, _, delays = dm_side.beam_ladder(250.0, 8, series.shape[1], 0.131)
    _, data, chunks = dm_side.check_dm_file(dm_file, series, delays)
    # the events of every deliver (the builder replayed over the chunks of dm.bin), the selection rule, the closing line, every stamp
    stamps = dm_side.check_stamps(st_file, r.stdout, cands, chunks, len(want), series, delays, **opts)
    print("stamps", len(stamps))
    assert len(stamps) >= 1
