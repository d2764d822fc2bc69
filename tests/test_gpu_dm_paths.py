"""GPU tests (-m gpu) of the shared-window DM kernel (csrc/bf_dm_wide.hip), one path of it per case.

dedisperse_dm_wide_kernel and dedisperse_dm_kernel give the same bits by design, and a group the first does not take -- or a launch
that fails a launcher gate -- silently runs the second: a bit-exact result alone does not show that the kernel under test ran.  Every
case here therefore asserts, besides the oracle's bits, WHICH trial groups the shared-window kernel took (bf_get_counter
"dm_wide_mask" / "dm_wide_groups") against what tests/support/dm_paths.py predicts from the delays.  The cases are built there, and
tests/test_dm_paths_cpu.py checks without a GPU that each reaches the path it is named after.  Every call goes through the C-ABI."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))

import dm_paths  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                                                              # floats of NaN on each side of every output


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


_want = {}


def expected(orc, case, n_t_out):
    """The oracle's result, computed once per (case, output length) and never written to."""
    key = (case.name, n_t_out)
    if key not in _want:
        w = orc.dedisperse_dm(case.series(), case.delays, n_t_out)
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def handle_for(bfmod, case):
    if case.handle_n_freq:                                              # more channels than the fused kernel's contract: set afterwards
        cfg = bfmod.debug_config(n_beams=case.n_b, n_ant=64, n_freq=case.handle_n_freq, n_avg=1, n_out_per_gemm=8)
        cfg.n_freq = case.n_f
    else:
        cfg = bfmod.debug_config(n_beams=case.n_b, n_freq=case.n_f)
    return bfmod.Beamformer(cfg)


def guarded(torch, n_floats, offset=0):
    """(allocation, view): n_floats floats that start `offset` floats behind a 16-byte boundary of a NaN-filled allocation, with at
    least GUARD floats of it on each side."""
    big = torch.full((GUARD + offset + n_floats + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    view = big[GUARD + offset:GUARD + offset + n_floats]
    assert big.data_ptr() % 16 == 0 and (view.data_ptr() - 4 * offset) % 16 == 0
    return big, view


def launch(torch, bf, case, d_series, d_delays, n_t_out, stream, out_offset=0):
    """One bf_dedisperse_dm_device into a guarded output.  Returns (allocation, offset of the output in it, floats)."""
    n = case.n_dm * n_t_out * case.n_b
    big, view = guarded(torch, n, out_offset)
    bf.dedisperse_dm(d_series, case.n_t, d_delays, case.n_dm, n_t_out, view, stream)
    return big, GUARD + out_offset, n


def check(big, lo, n, want, what):
    host = big.cpu().numpy()
    got = host[lo:lo + n].reshape(want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d of %d values differ from the oracle; first at (trial, time, beam) %s: got %r, want %r; trials %s" % (
            what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], np.unique(bad[:, 0])[:12].tolist()))
    assert np.isnan(host[:lo]).all() and np.isnan(host[lo + n:]).all(), "%s: wrote outside its output" % what


def run_case(torch, bf, orc, case, d_series=None, expect_mask=None, out_offset=0, n_t_outs=None):
    """The case three ways: the shared-window kernel on (the groups dm_paths predicts are the groups it took), off (it took none),
    and on again with the switch put back (the same groups).  Every result is the oracle's bits, and nothing is written outside the
    output."""
    if d_series is None:
        d_series = torch.from_numpy(case.series()).cuda()
    d_delays = torch.from_numpy(case.delays).cuda()
    mask = case.mask if expect_mask is None else expect_mask
    s = torch.cuda.current_stream().cuda_stream
    try:
        for n_t_out in n_t_outs or case.n_t_outs:
            want = expected(orc, case, n_t_out)
            bf.set_switch("dm_wide", 1)
            shared = launch(torch, bf, case, d_series, d_delays, n_t_out, s, out_offset)
            took = bf.counter("dm_wide_mask"), bf.counter("dm_wide_groups")
            bf.set_switch("dm_wide", 0)
            thread = launch(torch, bf, case, d_series, d_delays, n_t_out, s, out_offset)
            took_off = bf.counter("dm_wide_mask"), bf.counter("dm_wide_groups")
            bf.set_switch("dm_wide", 1)
            again = launch(torch, bf, case, d_series, d_delays, n_t_out, s, out_offset)
            took_again = bf.counter("dm_wide_mask"), bf.counter("dm_wide_groups")
            torch.cuda.synchronize()
            print("%s n_t_out %d: shared-window kernel took mask %s (%d groups), predicted %s" % (case, n_t_out, bin(took[0]), took[1], bin(mask)))
            check(*shared, want, "%s, n_t_out %d, dm_wide 1" % (case, n_t_out))
            check(*thread, want, "%s, n_t_out %d, dm_wide 0" % (case, n_t_out))
            assert took == (mask, bin(mask).count("1")), "%s, n_t_out %d: the shared-window kernel took groups %s, dm_paths predicts %s" % (
                case, n_t_out, bin(took[0]), bin(mask))
            assert took_off == (0, 0)
            check(*again, want, "%s, n_t_out %d, dm_wide back at 1" % (case, n_t_out))
            assert took_again == took
    finally:
        bf.set_switch("dm_wide", 1)


def run_on_own_handle(torch, bfmod, orc, case):
    bf = handle_for(bfmod, case)
    try:
        run_case(torch, bf, orc, case)
    finally:
        bf.close()


# ---- 1. pair distance: one straight-line asm body per distance 0 .. 3, DW_BODY_OWN for the rest (B before A too) ------------------
def test_pair_distances(torch, bfmod, orc):
    """All six distance classes, changing from channel to channel within a wave."""
    run_on_own_handle(torch, bfmod, orc, dm_paths.pair_distances())


@pytest.mark.parametrize("d", dm_paths.PAIR_CONSTANT_D)
def test_pair_constant_d(torch, bfmod, orc, d):
    """Every pair at distance d at every channel: a failure names the body."""
    run_on_own_handle(torch, bfmod, orc, dm_paths.pair_constant_d(d))


# ---- 2. DMA pieces per wave and the count wait_dma_but leaves in flight; 3. the fit boundary ---------------------------------------
def test_piece_counts(torch, bfmod, orc):
    """0 .. 4 pieces per wave, odd window heights, heights that change from window to window, one shared delay; a group one row over
    the cap at one channel between groups that are taken."""
    run_on_own_handle(torch, bfmod, orc, dm_paths.piece_counts())


@pytest.mark.parametrize("n_f", dm_paths.CAP_CHANNELS)
def test_cap_by_channels(torch, bfmod, orc, n_f):
    """The cap shrinks with the channel count: at rows_cap(n_f) a group is taken (the ring's three buffers full), one row over it is
    not; 1024 channels are supported, 1025 are not."""
    run_on_own_handle(torch, bfmod, orc, dm_paths.cap_by_channels(n_f))


# ---- 4. staging path: buffer-addressed ("inside") or per lane ----------------------------------------------------------------------
@pytest.mark.parametrize("n_b", dm_paths.EDGE_BEAMS)
def test_edges(torch, bfmod, orc, n_b):
    """Windows before row 0, across the last row, wholly past it; beam tiles of 4, 124, 128 + 4 and 2 x 128 beams."""
    run_on_own_handle(torch, bfmod, orc, dm_paths.edges(n_b))


# ---- 5. ring prologue and tails, the look-ahead reads behind the last channel; 6. trial counts -------------------------------------
@pytest.mark.parametrize("n_f", dm_paths.FEW_CHANNELS)
def test_few_channels(torch, bfmod, orc, n_f):
    run_on_own_handle(torch, bfmod, orc, dm_paths.few_channels(n_f))


def test_channels_multiple_of_64(torch, bfmod, orc):
    """No padding behind the tables: the reads of tab[f + 3] and offsAB[f + 1] behind the last channel land in window 0."""
    run_on_own_handle(torch, bfmod, orc, dm_paths.channels_multiple_of_64())


@pytest.mark.parametrize("n_dm", dm_paths.TRIAL_COUNTS)
def test_trial_counts(torch, bfmod, orc, n_dm):
    run_on_own_handle(torch, bfmod, orc, dm_paths.trial_counts(n_dm))


# ---- 7. launcher gates, and the flags of one call seen by the next -----------------------------------------------------------------
def test_gates(torch, bfmod, orc):
    """A series or an output that is only 4-byte aligned runs the per-thread-window kernel alone: mask 0 (not the flags the aligned
    call before it left in the same scratch), the oracle's bits, nothing outside the output.  An aligned call afterwards is taken again."""
    case = dm_paths.pair_distances()
    series = case.series()
    bf = handle_for(bfmod, case)
    try:
        aligned = torch.from_numpy(series).cuda()
        room = torch.zeros(series.size + 8, dtype=torch.float32, device="cuda")
        shifted = room[1:1 + series.size]
        shifted.copy_(aligned.reshape(-1))
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        run_case(torch, bf, orc, case, aligned)
        run_case(torch, bf, orc, case, shifted, expect_mask=0)
        run_case(torch, bf, orc, case, aligned, expect_mask=0, out_offset=1)
        run_case(torch, bf, orc, case, aligned)
    finally:
        bf.close()


def test_flags_between_calls(torch, bfmod, orc):
    """A stream's flag scratch is zeroed once and rewritten per launch for that launch's groups only.  Calls on one stream that flip a
    group's verdict or shrink the trial count -- no synchronisation between them but the counters' own -- each report their own groups
    and give their own bits; then two ladders that differ in group 1 alternate on two streams, each with its own scratch."""
    cases = dm_paths.flag_ladders()
    assert [c.mask for c in cases] == [0b101, 0b111, 0, 0b11]
    bf = handle_for(bfmod, cases[0])
    d_series = torch.from_numpy(cases[0].series()).cuda()
    d_delays = [torch.from_numpy(c.delays).cuda() for c in cases]
    n_t_out = cases[0].n_t_outs[0]                                      # complete sums of the longest ladder: every case lists it
    assert all(n_t_out in c.n_t_outs for c in cases)
    want = [expected(orc, c, n_t_out) for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(streams[0]):                             # (the NaN fills run on the stream of the launch behind them)
            outs = []
            for _ in range(2):                                          # eight launches, each followed by its counter reads and nothing else
                for i, c in enumerate(cases):
                    outs.append((i, launch(torch, bf, c, d_series, d_delays[i], n_t_out, streams[0].cuda_stream)))
                    assert (bf.counter("dm_wide_mask"), bf.counter("dm_wide_groups")) == (c.mask, bin(c.mask).count("1")), (c, c.mask)
            for i, out in outs:                                         # the bits afterwards: every output has its own allocation
                check(*out, want[i], "%s on one stream" % cases[i])
            del outs
        for turn in range(4):
            outs = []
            for k in (0, 1):                                            # stream k runs ladder (turn + k) % 2: group 1 flips on both, every turn
                i = (turn + k) % 2
                with torch.cuda.stream(streams[k]):
                    outs.append((i, launch(torch, bf, cases[i], d_series, d_delays[i], n_t_out, streams[k].cuda_stream)))
            i_last = outs[-1][0]
            assert bf.counter("dm_wide_mask") == cases[i_last].mask, turn   # the most recent launch: stream 1's
            torch.cuda.synchronize()
            for i, out in outs:
                check(*out, want[i], "%s, turn %d on two streams" % (cases[i], turn))
    finally:
        torch.cuda.synchronize()
        bf.close()


def test_stream_stage(torch, bfmod, orc):
    """bf_dm_stream over a ladder whose middle group is too coarse: after every push that emits rows the counters report groups
    {0, 2}; with the switch off, none; before the first chunk and once the stage is closed there is nothing to report."""
    from dsabeamformer_amd import api

    case, max_rows = dm_paths.stream_mixed_groups()
    assert case.fits.tolist() == [True, False, True]
    D = int(case.delays.max())
    want = expected(orc, case, case.n_t - D)
    bf = handle_for(bfmod, case)
    d_series = torch.from_numpy(case.series()).cuda()
    row_bytes = case.n_f * case.n_b * 4
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        for wide in (1, 0):
            bf.set_switch("dm_wide", wide)
            dm = api.DmStream(bf, case.delays, case.n_f, max_rows)
            assert bf.counter("dm_ring_stages") == 1
            cap_rows = dm.history()[2]                                  # the twice-mapped ring: the series runs past its seam by several pushes
            print("stream_stage: the ring holds %d rows, the series has %d" % (cap_rows, case.n_t))
            assert D + 3 * max_rows <= cap_rows <= case.n_t - 3 * max_rows, (cap_rows, case.n_t)
            host = torch.full((case.n_dm * max_rows * case.n_b,), float("nan"), dtype=torch.float32).pin_memory()
            parts, pushed, emitted, k = [], 0, False, 0
            sizes = [max_rows, 7, max_rows, 1, 19, max_rows, max_rows - 1, 3]
            while pushed < case.n_t:
                n = min(sizes[k % len(sizes)], case.n_t - pushed)
                k += 1
                first, n_out = dm.push(d_series.data_ptr() + pushed * row_bytes, n, host, st.cuda_stream)
                pushed += n
                emitted = emitted or n_out > 0
                took = bf.counter("dm_wide_mask"), bf.counter("dm_wide_groups")
                assert took == ((0b101, 2) if wide and emitted else (0, 0)), (wide, pushed, n_out, took)
                st.synchronize()
                if n_out:
                    parts.append(host[:case.n_dm * n_out * case.n_b].numpy().reshape(case.n_dm, n_out, case.n_b).copy())
            assert pushed == case.n_t and emitted
            assert np.array_equal(np.concatenate(parts, axis=1), want), wide
            dm.close()
            assert (bf.counter("dm_wide_mask"), bf.counter("dm_wide_groups")) == (0, 0)   # the scratch went with the stage
    finally:
        bf.set_switch("dm_wide", 1)
        bf.close()
