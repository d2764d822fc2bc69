"""GPU tests (-m gpu) of the voltage history and its dedispersed cuts (include/dsabf.h: bf_vhist_*; docs/VOLTAGE_CUTS.md), through the
C-ABI and api.VoltageHistory.  The reference is tests/support/vcut_oracle.py: the contract's formula as fancy indexing over a series it
holds whole.  Bytes are moved, so whole sentinel-filled outputs (guard bytes on both sides included) are compared bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import vcut_oracle as vo  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
CAP = 5
SIZES = [3, 1, 2, 3, 2, 1, 3, 2]            # ragged pushes of at most 3 units
GUARD = 16                                   # sentinel bytes in front of and behind every output


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _cfg(bfmod, n_ant, n_out, n_avg, n_freq, n_pol=2, **over):
    kw = dict(n_ant=n_ant, n_pol=n_pol, n_avg=n_avg, n_beams=32, n_freq=n_freq, n_out_per_gemm=n_out, n_gemms_per_block=4, n_blocks_on_gpu=2,
              n_streams=4)
    kw.update(over)
    return bfmod.debug_config(**kw)


def _units(rng, cfg, n_units):
    """uint8 [unit][freq][S][B]: the input layout [unit][freq][time][ant] with time = S * n_pol."""
    return rng.integers(0, 256, size=(n_units, cfg.n_freq, cfg.n_out_per_gemm * cfg.n_avg, cfg.n_pol * cfg.n_ant), dtype=np.uint8)


def delay_kinds(S):
    return [0, 1, S - 1, S, S + 1, 3 * S + 2]


def make_delays(S, n_freq):
    """Six rows; row d, channel f takes kind (d + 2 f) % 6, so every kind occurs in every column -- and the rows' largest delays differ, so
    that some of them fit a ring of CAP units at every n_units_out.  Two more rows: no delay at all, and S - 1 everywhere."""
    k = delay_kinds(S)
    rows = [[k[(d + 2 * f) % 6] for f in range(n_freq)] for d in range(6)] + [[0] * n_freq, [S - 1] * n_freq]
    if n_freq == 3:
        rows += [[0, 1, S - 1], [S, S + 1, 1], [S - 1, S, 0]]        # rows WITHOUT the largest kind: they fit at three output units too
    return np.array(rows, np.int32)


class Cuts:
    """Cuts issued without waiting for anything, each into a sentinel-filled output of its own (offset by `shift` bytes from a 256-byte
    aligned address); compared at the end, guard bytes included."""

    def __init__(self, torch, vh, units, delays):
        self.torch, self.vh, self.units, self.delays, self.pending, self.n_cut = torch, vh, units, delays, [], 0
        self.seen = set()      # (physical unit of the first source run is the ring's last, the run has a second source run)
        self.kinds = set()     # delays of the runs that were cut

    def cut(self, reqs, n_units_out, stream, shift=0, what=""):
        oldest, nxt, cap = self.vh.history()
        want, st_want = vo.cut(self.units, self.delays, reqs, n_units_out, oldest, nxt)
        n = want.size
        d_buf = self.torch.full((GUARD + n + GUARD,), vo.SENTINEL, dtype=self.torch.uint8, device="cuda")
        assert d_buf.data_ptr() % 256 == 0 and shift % 4 == 0 and shift < GUARD
        stream.wait_stream(self.torch.cuda.current_stream())                   # (the fill runs on torch's queue: ordered on the device)
        st = self.vh.cut(reqs, n_units_out, d_buf.data_ptr() + shift, stream.cuda_stream)
        assert list(st) == list(st_want), (what, reqs, list(st), list(st_want), (oldest, nxt))
        self.pending.append((d_buf, shift, want, (what, reqs, n_units_out, oldest, nxt)))
        self.n_cut += int((st == 0).sum())
        S = self.units.shape[2]
        for (t0, dm), s in zip(reqs, st):
            if s == 0:
                for u in range(n_units_out):
                    for d in self.delays[dm]:
                        s0 = t0 + u * S + int(d)
                        self.seen.add(((s0 // S) % cap == cap - 1, s0 % S != 0))
                        self.kinds.add(int(d))
        return st

    def compare(self):
        self.torch.cuda.synchronize()
        for d_buf, shift, want, what in self.pending:
            got = d_buf.cpu().numpy()
            full = np.full(got.shape, vo.SENTINEL, np.uint8)
            full[shift:shift + want.size] = want.reshape(-1)
            bad = np.flatnonzero(got != full)
            assert bad.size == 0, (what, bad.size, int(bad[0]) - shift, np.unravel_index(min(max(int(bad[0]) - shift, 0), want.size - 1), want.shape))
        self.pending = []


def edge_requests(delays, S, oldest, nxt, n_units_out):
    """Per row of the table: windows that begin on a unit boundary, one sample before and one after it -- the boundaries of the oldest unit
    and the one behind it, of the newest unit and the end of the series, and of the ring's last physical unit and its first (the seam);
    and windows that end exactly at the newest sample, one before and one behind.  Statuses 0, 1 and 2 all occur."""
    seam = nxt // CAP * CAP
    bounds = {u for u in (oldest, oldest + 1, nxt - 1, nxt, seam - 1, seam) if oldest <= u <= nxt}
    reqs = []
    for dm in range(len(delays)):
        sp = vo.span(delays, dm, n_units_out, S)
        t0s = {nxt * S - sp + k for k in (-1, 0, 1)}
        for unit in bounds:
            t0s |= {unit * S + k for k in (-1, 0, 1)}
        reqs += [(t0, dm) for t0 in sorted(t0s) if t0 >= 0]
    return reqs


# (n_ant, n_out_per_gemm, n_avg, n_freq, n_units_out).  B = 2 n_ant: 8 and 24 bytes (n_ant 4, 12) and 136 (68) take the 4-byte kernel, 16
# and 128 (8, 64) the 16-byte one -- and the 4-byte one again where the output is offset by 4 bytes.  S = n_out * n_avg: 1, 3, 24, 256.  Runs
# of S B bytes from 8 bytes (one lane of one workgroup) to 34816 (68 antennas, S 256: eight and a half pieces of 4096 bytes) and 32768
# (64 antennas, S 256: two pieces of 16384 bytes).
SHAPE_CASES = [(4, 1, 1, 1, 1), (12, 3, 1, 3, 3), (8, 3, 8, 3, 1), (64, 16, 16, 3, 3), (68, 8, 3, 1, 3), (64, 1, 1, 1, 1), (8, 16, 16, 1, 3),
               (4, 8, 3, 3, 3), (12, 16, 16, 3, 1), (68, 16, 16, 1, 1), (64, 3, 1, 3, 1), (8, 1, 1, 3, 3), (64, 8, 3, 1, 3)]


def test_the_cases_cover_the_contract():
    """(no device needed, but it belongs to the cases) every antenna count, S, n_freq and n_units_out the contract names; and at every
    S > 1 every kind of delay lies in a row that fits a ring of 5 units in some case."""
    for lst, idx in (((4, 8, 12, 64, 68), 0), ((1, 3), 3), ((1, 3), 4)):
        assert {c[idx] for c in SHAPE_CASES} == set(lst), idx
    assert {c[1] * c[2] for c in SHAPE_CASES} == {1, 3, 24, 256}
    for S in (3, 24, 256):
        kinds = set()
        for n_ant, n_out, n_avg, n_freq, n_units_out in SHAPE_CASES:
            if n_out * n_avg == S:
                kinds |= fitting_kinds(make_delays(S, n_freq), S, n_units_out)
        assert kinds == set(delay_kinds(S)), (S, kinds)


def fitting_kinds(delays, S, n_units_out):
    """The delays of the rows whose window fits the ring."""
    return {int(d) for dm in range(len(delays)) if vo.span(delays, dm, n_units_out, S) <= CAP * S for d in delays[dm]}


@pytest.mark.sweep_cap(len(SHAPE_CASES))                                       # (a fraction of a second each: all of them, always)
@pytest.mark.parametrize("case", SHAPE_CASES, ids=lambda c: "ant%d-S%dx%d-f%d-u%d" % c)
def test_every_shape_to_the_byte(torch, bfmod, case):
    """A ring of 5 units, ragged pushes of at most 3 units alternating on two queues until the ring has wrapped three times, cuts on a third
    queue after every push with nothing waited for on the host: unit boundaries (the oldest, the newest, the ring's seam), one sample before
    and after them, for every row of a delay table whose channels take every kind of delay; 0, 1 and 33 requests; outputs offset by 4 bytes."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(20261020)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    n_ant, n_out, n_avg, n_freq, n_units_out = case
    cfg = _cfg(bfmod, n_ant, n_out, n_avg, n_freq)
    S = n_out * n_avg
    delays = make_delays(S, n_freq)
    n_units = 3 * CAP + 3
    units = _units(rng, cfg, n_units)
    d_units = torch.from_numpy(units).cuda()
    unit_bytes = units[0].nbytes
    bf = bfmod.Beamformer(cfg)
    vh = api.VoltageHistory(bf, delays, CAP)
    assert vh.history() == (0, 0, CAP)
    cuts = Cuts(torch, vh, units, delays)
    at, k = 0, 0
    torch.cuda.synchronize()
    while at < n_units:
        n = min(SIZES[k % len(SIZES)], n_units - at)
        vh.push(d_units.data_ptr() + at * unit_bytes, n, (s1, s2)[k % 2].cuda_stream)
        at, k = at + n, k + 1
        oldest, nxt, cap = vh.history()
        assert (oldest, nxt, cap) == (max(0, at - CAP), at, CAP)
        reqs = edge_requests(delays, S, oldest, nxt, n_units_out)
        assert len(reqs) > 33                                                  # (more than one launch)
        cuts.cut(reqs, n_units_out, s3, shift=4 * (k % 2), what=(case, "after push", k))
    assert at == n_units and at // CAP >= 3
    oldest, nxt, _ = vh.history()
    fits = [(oldest * S, dm) for dm in range(len(delays)) if vo.span(delays, dm, n_units_out, S) <= CAP * S]
    assert fits, case
    cuts.cut([], n_units_out, s3, what=(case, "no request"))
    cuts.cut(fits[:1], n_units_out, s3, shift=4, what=(case, "one request"))
    cuts.cut([fits[i % len(fits)] if i % 3 else (oldest * S - 1, 0) for i in range(33)], n_units_out, s3, what=(case, "33 requests"))
    cuts.compare()
    assert cuts.n_cut > 33, (case, cuts.n_cut)
    # source runs in the ring's last physical unit and elsewhere, with and without a second source run behind them
    assert cuts.seen == {(a, b) for a in (False, True) for b in ((False, True) if S > 1 else (False,))}, (case, cuts.seen)
    assert cuts.kinds == fitting_kinds(delays, S, n_units_out), (case, cuts.kinds)
    print("vcut %s: %d windows cut" % (case, cuts.n_cut))
    vh.close()
    bf.close()


def test_status_edges(torch, bfmod):
    """A window that begins exactly at oldest_unit * S and one that ends exactly at next_unit * S are cut; each moved by one sample is
    refused with 1 and 2; one that is both too old and too new answers 1.  Refused requests leave their sentinels beside cut ones."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(5)
    cfg = _cfg(bfmod, 8, 3, 8, 3)
    S = 24
    delays = np.array([[0, 0, 0], [0, 5, S + 1]], np.int32)
    units = _units(rng, cfg, 7)
    bf = bfmod.Beamformer(cfg)
    vh = api.VoltageHistory(bf, delays, CAP)
    st = torch.cuda.Stream()
    d_units = torch.from_numpy(units).cuda()
    torch.cuda.synchronize()
    for at, n in ((0, 3), (3, 3), (6, 1)):
        vh.push(d_units.data_ptr() + at * units[0].nbytes, n, st.cuda_stream)
    assert vh.history() == (2, 7, CAP)
    cuts = Cuts(torch, vh, units, delays)
    for dm in (0, 1):
        sp = vo.span(delays, dm, 2, S)
        reqs = [(2 * S, dm), (2 * S - 1, dm), (7 * S - sp, dm), (7 * S - sp + 1, dm), (2 * S + 1, dm), (0, dm), (7 * S, dm), (2 ** 63, dm)]
        got = cuts.cut(reqs, 2, st, what=("edges", dm))
        assert list(got) == [0, 1, 0, 2, 0, 1, 2, 2]
    # a window longer than the ring: too old AND not pushed yet answers 1; from the oldest sample on it answers 2
    assert list(cuts.cut([(2 * S - 1, 0), (2 * S, 0), (2 * S, 1)], 6, st, what="both")) == [1, 2, 2]
    # exactly the whole ring
    assert list(cuts.cut([(2 * S, 0), (2 * S, 1)], 5, st, what="whole ring")) == [0, 2]
    cuts.compare()
    vh.close()
    bf.close()


def test_a_cut_is_ordered_against_later_pushes(torch, bfmod):
    """One queue is kept busy for tens of milliseconds with matrix products and a cut of the whole ring is queued behind them.  On another
    queue enough pushes follow at once to overwrite every unit of the ring.  The cut still equals the oracle, and so does a later cut
    (on a third queue) of the new units."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(6)
    cfg = _cfg(bfmod, 64, 16, 16, 3)
    S = 256
    delays = np.array([[0, 0, 0], [S + 1, 7, 0]], np.int32)
    units = _units(rng, cfg, 2 * CAP + 2 + CAP)
    bf = bfmod.Beamformer(cfg)
    vh = api.VoltageHistory(bf, delays, CAP)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    d_units = torch.from_numpy(units).cuda()
    big = torch.randn((8192, 8192), device="cuda")
    unit_bytes = units[0].nbytes
    n_first = 2 * CAP + 2
    for at in range(0, n_first, 2):
        vh.push(d_units.data_ptr() + at * unit_bytes, 2, s2.cuda_stream)
    torch.cuda.synchronize()
    oldest, nxt, _ = vh.history()
    assert (oldest, nxt) == (n_first - CAP, n_first)
    cuts = Cuts(torch, vh, units, delays)
    with torch.cuda.stream(s1):
        for _ in range(4):
            torch.mm(big, big)
    got = cuts.cut([(oldest * S, 0), (oldest * S, 1), (oldest * S + S - 2, 1)], 3, s1, what="behind the busy queue")   # runs when s1 gets to it
    assert list(got) == [0, 0, 0]
    for k, at in enumerate(range(n_first, n_first + CAP, 1)):                   # at once, alternating between two idle queues
        vh.push(d_units.data_ptr() + at * unit_bytes, 1, (s2, s3)[k % 2].cuda_stream)
    oldest2, nxt2, _ = vh.history()
    assert oldest2 >= nxt                                                      # every unit the first cut reads has a new owner
    got = cuts.cut([(oldest2 * S, 0), (oldest2 * S, 1), (oldest2 * S + S - 2, 1)], 3, s3, what="the new units")
    assert list(got) == [0, 0, 0]
    cuts.compare()
    vh.close()
    bf.close()


def test_existing_stages_run_on_a_cut(torch, bfmod):
    """A pulse-like scene dispersed across 3 channels at 64 antennas and two polarisations: bf_stokes_device(n_int = 1) on the cut equals
    stokes_oracle over the oracle's cut, and bf_beamform_device on the cut equals the same call on an upload of the oracle's cut."""
    import stokes_oracle as so

    from dsabeamformer_amd import api

    rng = np.random.default_rng(8)
    cfg = _cfg(bfmod, 64, 8, 2, 3)
    S, n_units = 16, 6
    delays = np.array([[0, 0, 0], [0, 9, 21]], np.int32)                      # the pulse arrives later in the later channels
    units = rng.integers(0, 256, size=(n_units, 3, S, 128), dtype=np.uint8) & 0x11          # faint noise: nibbles 0 / 1
    pulse_at = 2 * S + 3                                                     # sample of the pulse at channel 0; 4 samples wide
    series = vo.series_of(units)
    for f in range(3):
        series[pulse_at + delays[1][f]:pulse_at + delays[1][f] + 4, f] = rng.integers(0, 256, size=(4, 128), dtype=np.uint8)
    units = np.ascontiguousarray(series.reshape(n_units, S, 3, 128).transpose(0, 2, 1, 3))
    w = rng.integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8)
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(w)
    vh = api.VoltageHistory(bf, delays, n_units)
    st = torch.cuda.Stream()
    d_units = torch.from_numpy(units).cuda()
    torch.cuda.synchronize()
    vh.push(d_units, n_units, st.cuda_stream)
    t0, n_out_units = pulse_at - S - 3, 2                                     # the dedispersed pulse lies inside the second output unit
    want_cut, st_want = vo.cut(units, delays, [(t0, 1)], n_out_units, 0, n_units)
    assert list(st_want) == [0]
    on_pulse = want_cut[0, 1, :, 6:10]                                       # aligned in every channel after the cut
    assert (on_pulse & 0xEE).any(axis=(1, 2)).all() and not (want_cut[0, 0] & 0xEE).any()
    d_cut = torch.full((want_cut.size,), vo.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert list(vh.cut([(t0, 1)], n_out_units, d_cut, st.cuda_stream)) == [0]
    st.synchronize()
    assert np.array_equal(d_cut.cpu().numpy(), want_cut.reshape(-1))
    # the Stokes stage on the cut
    beams = [31, 0, 7]
    stage = api.StokesBeams(bf, 1)
    stage.set_weights(w, beams)
    packed = want_cut[0].reshape(n_out_units, 3, S * 2, 64)
    want = so.stokes(packed, w, beams, 1, so.geometry(cfg))
    d_out = torch.zeros((want.size,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stage.compute(d_cut, n_out_units, d_out, st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy().reshape(want.shape), want)
    # the beamformer itself: the cut against an upload of the oracle's cut
    n_floats = n_out_units * cfg.n_out_per_gemm * cfg.n_freq * cfg.n_beams
    a = torch.zeros((n_floats,), dtype=torch.float32, device="cuda")
    b = torch.zeros((n_floats,), dtype=torch.float32, device="cuda")
    d_want = torch.from_numpy(want_cut.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    bf.beamform(d_cut, n_out_units, a, st.cuda_stream)
    bf.beamform(d_want, n_out_units, b, st.cuda_stream)
    st.synchronize()
    ga, gb = a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
    assert np.array_equal(ga, gb) and ga.any()
    stage.close()
    vh.close()
    bf.close()


def test_push_block_and_the_host_cut(torch, bfmod):
    """bf_submit_block, bf_enqueue_block and bf_vhist_push_block on the same queue for two blocks on alternating slots, the second block in
    two launches: the history holds the units in the order pushed, and bf_vhist_cut_host into pinned memory equals the oracle, refused
    requests untouched."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(9)
    cfg = _cfg(bfmod, 12, 8, 2, 3)                                              # S = 16, B = 24: 4-byte path; 4 units per block
    S, n_u = 16, cfg.n_gemms_per_block
    blocks = np.stack([_units(rng, cfg, n_u) for _ in range(2)])
    w = rng.integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8)
    delays = np.array([[0, 0, 0], [1, S, S + 1]], np.int32)
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(w)
    vh = api.VoltageHistory(bf, delays, 7)
    pin = torch.from_numpy(blocks).pin_memory()
    for slot in (0, 1):
        bf.submit_block(slot, pin[slot], blocks[slot].nbytes)
    bf.sync(-1)
    for slot, first, n in [(0, 0, n_u), (1, 0, 1), (1, 1, n_u - 1)]:
        bf.enqueue_block(slot, slot, first, n, None)
        vh.push_block(slot, slot, first, n)
    assert vh.history() == (1, 8, 7)
    for bad in ((4, 0, 0, 1), (0, 2, 0, 1), (0, 0, n_u, 1), (0, 0, 1, n_u)):
        with pytest.raises(bfmod.DsabfError) as e:
            vh.push_block(*bad)
        assert e.value.code == BF_ERR_INVALID
    units = blocks.reshape(2 * n_u, *blocks.shape[2:])
    reqs = [(S, 0), (S - 1, 1), (S + 5, 1), (8 * S - 2 * S, 0), (8 * S - 2 * S, 1), (3 * S + 1, 1)]
    want, st_want = vo.cut(units, delays, reqs, 2, 1, 8)
    assert list(st_want) == [0, 1, 0, 0, 2, 0]
    host = torch.full((want.size,), vo.SENTINEL, dtype=torch.uint8).pin_memory()
    got = vh.cut_host(reqs, 2, host)
    assert list(got) == list(st_want)
    assert np.array_equal(host.numpy(), want.reshape(-1))
    assert list(vh.cut_host(reqs[:1], 3, host)) == [0]                          # a larger cut: the stage's buffer grows
    assert np.array_equal(host.numpy()[:3 * units[0].nbytes], vo.window(units, delays, S, 0, 3).reshape(-1))
    vh.close()
    bf.close()


def _window_of_run(ring, first_block, cfg, delays_samples, t0, n_units_out):
    """The oracle's window over the series a `beam -j` run analyses, without holding that series: unit u of it is unit u % n_gemms_per_block
    of junk block (first_block + u / n_gemms_per_block) % 4.  Channel by channel: the units its samples touch, joined, then sliced."""
    n_u, S, B = cfg.n_gemms_per_block, cfg.n_out_per_gemm * cfg.n_avg, cfg.n_pol * cfg.n_ant
    out = np.empty((n_units_out, cfg.n_freq, S, B), np.uint8)
    for f in range(cfg.n_freq):
        s0 = t0 + int(delays_samples[f])
        first, j0 = s0 // S, s0 % S
        seg = np.concatenate([ring[(first_block + u // n_u) % 4][u % n_u][f] for u in range(first, first + n_units_out + (1 if j0 else 0))])
        out[:, f] = seg[j0:j0 + n_units_out * S].reshape(n_units_out, S, B)
    return out


def test_push_block_and_the_observation_loop(bfmod, tmp_path):
    """`beam -j 33 -M 250 -N 8 -S 4 -B 6 -i 255 -w det.bin -W dm.bin -C cands.txt --events ev.txt --voltages v.bin --voltage-units 2`: 25
    burn-in reads + 8 analysed blocks.  Every record of v.bin equals the oracle's cut of the junk source's blocks (regenerated with
    host.junk_bytes) at the DM stage's row delays times n_avg; the set of records is the selection rule recomputed from the events of
    every deliver (at most 4 per feed, by snr), vcuts_dropped and the requests beyond the end of the run included; vcuts_missed is 0; at
    least one record is written; and the -w stream beside it is byte-identical to the same run without --voltages."""
    import subprocess

    import evt_oracle as eo

    from dsabeamformer_amd import api, build, host

    names = ("det.bin", "dm.bin", "cands.txt", "ev.txt", "v.bin", "det0.bin", "dm0.bin", "cands0.txt", "ev0.txt")
    det_file, dm_file, cand_file, ev_file, v_file, det0, dm0, cand0, ev0 = (str(tmp_path / n) for n in names)
    base = [build.BEAM, "-j", "33", "-M", "250", "-N", "8", "-S", "4", "-B", "6", "-i", "255"]
    r = subprocess.run(base + ["-w", det_file, "-W", dm_file, "-C", cand_file, "--events", ev_file, "--voltages", v_file, "--voltage-units", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    r0 = subprocess.run(base + ["-w", det0, "-W", dm0, "-C", cand0, "--events", ev0], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and "Voltage cuts" not in r0.stdout, r0.stdout[-3000:] + r0.stderr
    for a, b in ((det_file, det0), (dm_file, dm0), (cand_file, cand0), (ev_file, ev0)):
        assert open(a, "rb").read() == open(b, "rb").read(), a
    os.remove(det0)
    cfg = bfmod.production_config()
    S, n_u = cfg.n_out_per_gemm * cfg.n_avg, cfg.n_gemms_per_block
    # the events of every deliver: the builder replayed over the chunks of dm.bin (a candidate is reported with the END of its boxcar)
    opts = dict(max_width=32, ib_beam=255)
    tab = np.loadtxt(cand_file, ndmin=2)
    cands = eo.candidates([(int(v[0]), int(v[1]), int(v[2]), int(v[3]), v[4], v[5]) for v in tab])
    _, _, chunks = host.read_dm_file(dm_file)
    t_end = cands["t_start"].astype(np.int64) + cands["width"] - 1
    picked, dropped = [], 0
    with api.EventBuilder(**opts) as eb:
        feeds = [eb.feed(cands[(t_end >= first_t) & (t_end < first_t + n_t)], first_t + n_t) for first_t, n_t in chunks] + [eb.flush()]
    for ev in feeds:
        pick = sorted([e for e in ev if not e["flags"]], key=lambda e: -float(e["best"]["snr"]))     # (stable: ties stay in event order)
        dropped += max(0, len(pick) - 4)
        picked += pick[:4]
    # the driver's ladder, in samples
    dms = host.dm_trials(dm_max=250.0)
    dms = np.array([dms[int(i * (len(dms) - 1) / 7)] for i in range(8)])
    freq = np.array([host.channel_frequency(0, ch) for ch in range(cfg.n_freq)], np.float32)
    delays = host.dm_delays(dms, freq, float(freq[0]), 0.131).astype(np.int64) * cfg.n_avg
    total = 8 * n_u * S

    def request(e):
        b = e["best"]
        return max(0, (int(b["t_start"]) + int(b["width"]) // 2) * cfg.n_avg - 2 * S // 2), int(b["dm"]), int(b["beam"]), int(b["width"])

    beyond = [e for e in picked if request(e)[0] + 2 * S + int(delays[request(e)[1]].max()) > total]
    picked = [e for e in picked if request(e)[0] + 2 * S + int(delays[request(e)[1]].max()) <= total]
    line = "Voltage cuts: %d cuts of 2 gemm-units, vcuts_dropped %d, vcuts_missed 0, beyond the end of the run %d" % (len(picked), dropped, len(beyond))
    assert line in r.stdout, (line, r.stdout[-1500:])
    hdr, cuts = host.read_voltage_file(v_file)
    print("voltage cuts", len(cuts), "dropped", dropped, "beyond the end", len(beyond))
    assert len(cuts) == len(picked) >= 1
    assert [hdr[k] for k in ("NANT", "NFREQ", "NPOL", "NAVG", "NOUT", "UNITS", "FIRST_CHANNEL")] == ["64", "256", "2", "16", "8", "2", "0"]
    assert sorted((c["t0"], c["dm"], c["beam"], c["width"]) for c in cuts) == sorted(request(e) for e in picked)
    n_time = cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg
    ring = host.junk_bytes(cfg.n_ant * cfg.n_freq * n_time * n_u, 4, 0xD5A, cfg).reshape(4, n_u, cfg.n_freq, S, cfg.n_pol * cfg.n_ant)
    for c in cuts:
        want = _window_of_run(ring, 25, cfg, delays[c["dm"]], c["t0"], 2)
        assert np.array_equal(c["data"], want), (c["t0"], c["dm"], c["beam"])


def test_refusals_and_lifetime(torch, bfmod):
    """Every BF_ERR_INVALID of the contract, with nothing launched: output and status stay as they were.  n_units > cap_units.  A stage whose
    handle was destroyed first answers BF_ERR_STATE and can still be destroyed."""
    from dsabeamformer_amd import _lib, api

    lib = _lib.load()
    rng = np.random.default_rng(10)
    cfg = _cfg(bfmod, 8, 3, 8, 3)
    S, n_dm = 24, 2
    delays = np.array([[0, 0, 0], [0, 5, S + 1]], np.int32)
    units = _units(rng, cfg, 5)
    bf = bfmod.Beamformer(cfg)
    st = torch.cuda.Stream()
    d_units = torch.from_numpy(units).cuda()
    torch.cuda.synchronize()
    v = C.c_void_p()

    def create(h=bf._h, d=delays.ctypes.data, n=n_dm, hist=CAP, out=C.byref(v)):
        return lib.bf_vhist_create(h, d, n, hist, out)

    neg = delays.copy()
    neg[1, 2] = -1
    for bad in (dict(h=None), dict(d=None), dict(n=0), dict(n=-1), dict(hist=0), dict(hist=-2), dict(out=None), dict(d=neg.ctypes.data)):
        assert create(**bad) == BF_ERR_INVALID and not v.value, bad
    assert b"negative" in lib.bf_last_error()
    vh = api.VoltageHistory(bf, delays, CAP)
    push = lambda p=d_units.data_ptr(), n=2, s=None: lib.bf_vhist_push(vh._c if s is None else s, p, n, st.cuda_stream)   # noqa: E731
    for bad in (dict(p=None), dict(p=d_units.data_ptr() + 2), dict(n=0), dict(n=-1), dict(n=CAP + 1)):
        assert push(**bad) == BF_ERR_INVALID, bad
    assert vh.history() == (0, 0, CAP)
    assert push(n=5) == 0
    n_bytes = 2 * 2 * units[0].nbytes
    d_out = torch.full((n_bytes + 16,), vo.SENTINEL, dtype=torch.uint8, device="cuda")
    status = np.full(2, -7, np.int32)
    reqs = np.zeros(2, api.vcut_request_dtype())
    reqs["t0"], reqs["dm"] = S + 1, 1

    def cut(r=reqs, n_req=2, n_units_out=2, out=d_out.data_ptr(), stat=status.ctypes.data, s=None):
        return lib.bf_vhist_cut(vh._c if s is None else s, r.ctypes.data if r is not None else None, n_req, n_units_out, out, stat, st.cuda_stream)

    for bad in (dict(n_units_out=0), dict(n_units_out=-3), dict(n_req=-1), dict(r=None), dict(out=None), dict(stat=None), dict(out=d_out.data_ptr() + 2),
                dict(out=d_out.data_ptr() + 1), dict(n_units_out=65536 // 3 + 1)):
        assert cut(**bad) == BF_ERR_INVALID, bad
    for value in (-1, n_dm):
        r = reqs.copy()
        r["dm"][1] = value
        assert cut(r=r) == BF_ERR_INVALID and b"trial" in lib.bf_last_error(), value
    host = np.zeros(n_bytes, np.uint8)
    for bad in (dict(n_units_out=0), dict(n_req=-1), dict(r=None), dict(out=None), dict(stat=None)):
        kw = dict(dict(r=reqs, n_req=2, n_units_out=2, out=host.ctypes.data, stat=status.ctypes.data), **bad)
        assert lib.bf_vhist_cut_host(vh._c, kw["r"].ctypes.data if kw["r"] is not None else None, kw["n_req"], kw["n_units_out"], kw["out"], kw["stat"]) \
            == BF_ERR_INVALID, bad
    u = C.c_uint64()
    assert lib.bf_vhist_history(vh._c, None, C.byref(u), C.byref(u)) == BF_ERR_INVALID
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == vo.SENTINEL) and np.all(status == -7) and not host.any()
    assert cut() == 0 and list(status) == [0, 0]                               # ... and the same call, valid
    assert cut(n_req=0, r=None, out=None, stat=None) == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    one = vo.window(units, delays, S + 1, 1, 2).reshape(-1)
    assert np.array_equal(got[:n_bytes], np.concatenate([one, one])) and np.all(got[n_bytes:] == vo.SENTINEL)
    # a stage whose handle was destroyed first
    bf.close()
    assert cut() == BF_ERR_STATE and push() == BF_ERR_STATE
    assert lib.bf_vhist_history(vh._c, C.byref(u), C.byref(u), C.byref(u)) == BF_ERR_STATE
    assert lib.bf_vhist_push_block(vh._c, 0, 0, 0, 1) == BF_ERR_STATE
    assert lib.bf_vhist_cut_host(vh._c, reqs.ctypes.data, 2, 2, host.ctypes.data, status.ctypes.data) == BF_ERR_STATE
    assert lib.bf_vhist_destroy(vh._c) == 0
    vh._c = C.c_void_p()
