"""GPU tests (-m gpu) of the pulsar folder (include/dsabf.h: bf_psr_*, bf_dm_stream_attach_folder; docs/PULSAR_FOLDING.md), through the
C-ABI.  The reference is tests/support/psr_oracle.py, a numpy restatement of the contract; profiles and hits are compared with it bit
for bit (.view(np.uint64): a -0.0 cannot hide).

The input makes the ORDER of a cell's adds matter: x = N(0, 1) * 2^e with e uniform in -40 .. 40.  Tame powers fold to the same bits in
any order, and a kernel that summed with atomics or in a tree would pass on them; every parity case first asserts, on the CPU, that the
oracle's own result for its input changes when the rows are folded in reverse."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cond_oracle  # noqa: E402
import dm_side  # noqa: E402
import psr_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
SIZES = [1, 7, 33, 64]
ONE = 1 << 64


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def wide(rng, shape):
    return (rng.standard_normal(shape) * 2.0 ** rng.integers(-40, 41, shape)).astype(np.float32)


def cuts_of(n_rows, sizes):
    cuts, at, k = [], 0, 0
    while at < n_rows:
        n = min(sizes[k % len(sizes)], n_rows - at)
        cuts.append((at, n))
        at, k = at + n, k + 1
    return cuts


def order_matters(x, models, delays, n_bins, first_row=0):
    """The oracle's fold of x, after asserting that folding the rows in reverse changes its bits: a condition on the input."""
    want = psr_oracle.fold(x, models, delays, n_bins, first_row)
    back = psr_oracle.fold(x, models, delays, n_bins, first_row, reverse=True)
    assert np.array_equal(back[1], want[1]) and not np.array_equal(bits(back[0]), bits(want[0]))
    return want


def models_for(n_psr, n_bins, n_rows, which):
    """The four kinds of model the shapes need, as (phase0, dphase, ddphase, epoch_row):
    fast:  0.37 turns per row -- more than one bin per row from 5 bins on (bins are skipped), ddphase > 0;
    slow:  about 30 rows per bin (long register runs), ddphase < 0, the epoch in the middle of the series (negative n);
    still: dphase = ddphase = 0 -- every row of a channel lands in one bin;
    creep: three rows per bin at a constant step, from half a turn, the epoch at row 7 -- at 4096 bins the 203 rows of a channel stay in 68 bins.
    One pulsar is `which`; two are slow + creep, three fast + slow + still, four all of them."""
    pool = {"fast": (int(0.1 * ONE), int(0.37 * ONE), 3 << 40, 0),
            "slow": (int(0.9 * ONE), ONE // (30 * n_bins), -(5 << 36), n_rows // 2),
            "still": (int(0.77 * ONE), 0, 0, -12),
            "creep": (ONE // 2, ONE // (3 * n_bins), 0, 7)}
    return [pool[k] for k in {1: (which,), 2: ("slow", "creep"), 3: ("fast", "slow", "still"), 4: ("fast", "slow", "still", "creep")}[n_psr]]


def delays_for(rng, n_psr, n_f, n_rows):
    d = rng.integers(0, 25, (n_psr, n_f)).astype(np.int32)
    d[-1, n_f // 2] = n_rows + 50          # one delay larger than the whole series
    return d


def push_all(torch, folder, d_x, row_bytes, cuts, streams):
    """The rows of d_x through `folder` in the given cuts, alternating over the streams, no host synchronisation in between."""
    for k, (at, n) in enumerate(cuts):
        folder.push(d_x.data_ptr() + at * row_bytes, n, streams[k % len(streams)].cuda_stream)


# every value of every axis: n_beams 4 60 64 68 256 260 516, n_freq_total 1 3 40, n_bins 2 5 64 1024 4096, n_psr 1 2 3 4 -- every
# compiled psr_fold_kernel<NPSR> -- (and every kind of model alone).  260 beams: a second beam block (blockIdx.y = 1) with 4 live
# lanes; 516: three blocks; 4096 bins: the contract's maximum.
SHAPES = [(4, 1, 2, 1, "fast"), (60, 3, 5, 3, None), (64, 40, 64, 1, "slow"), (68, 3, 1024, 3, None), (256, 40, 64, 3, None),
          (256, 1, 1024, 1, "still"), (68, 40, 5, 1, "fast"), (64, 3, 2, 3, None), (60, 1, 64, 1, "slow"), (4, 40, 1024, 3, None),
          (260, 3, 5, 2, None), (516, 1, 64, 4, None), (4, 3, 4096, 4, None), (64, 1, 2, 2, None)]


@pytest.mark.sweep_cap(len(SHAPES))
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "b%d-f%d-bins%d-psr%d%s" % (c[0], c[1], c[2], c[3], "-" + c[4] if c[4] else ""))
def test_every_shape_to_the_bit(torch, bfmod, case):
    from dsabeamformer_amd import api

    n_b, n_f, n_bins, n_psr, which = case
    n_rows = 203
    rng = np.random.default_rng(n_b * 1000 + n_f * 10 + n_psr)
    x = wide(rng, (n_rows, n_f, n_b))
    models = models_for(n_psr, n_bins, n_rows, which)
    delays = delays_for(rng, n_psr, n_f, n_rows)
    want_prof, want_hits = order_matters(x, models, delays, n_bins)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    folder = api.PulsarFolder(bf, n_f, 64, n_bins, models, delays)
    push_all(torch, folder, d_x, n_f * n_b * 4, cuts_of(n_rows, SIZES), streams)
    folder.dump()
    prof, hits, first_row, got_rows = folder.collect()
    assert (first_row, got_rows) == (0, n_rows)
    assert np.array_equal(hits, want_hits) and int(hits.sum()) == n_rows * n_f * n_psr
    assert np.array_equal(bits(prof), bits(want_prof))
    folder.close()
    bf.close()


def test_the_cut_into_pushes_does_not_matter(torch, bfmod):
    from dsabeamformer_amd import api

    n_b, n_f, n_bins, n_rows = 68, 3, 5, 203
    rng = np.random.default_rng(77)
    x = wide(rng, (n_rows, n_f, n_b))
    models = models_for(3, n_bins, n_rows, None)
    delays = delays_for(rng, 3, n_f, n_rows)
    want_prof, want_hits = order_matters(x, models, delays, n_bins)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    for sizes in ([n_rows], [1], [33, 1, 64, 7, 2, 64]):
        folder = api.PulsarFolder(bf, n_f, n_rows, n_bins, models, delays)
        push_all(torch, folder, d_x, n_f * n_b * 4, cuts_of(n_rows, sizes), streams)
        folder.dump()
        prof, hits, _, _ = folder.collect()
        assert np.array_equal(hits, want_hits) and np.array_equal(bits(prof), bits(want_prof)), sizes
        folder.close()
    bf.close()


def test_dump_in_mid_stream(torch, bfmod):
    from dsabeamformer_amd import api

    n_b, n_f, n_bins, n_rows, split = 60, 3, 64, 180, 77
    rng = np.random.default_rng(31)
    x = wide(rng, (n_rows, n_f, n_b))
    models = models_for(3, n_bins, n_rows, None)
    delays = delays_for(rng, 3, n_f, n_rows)
    want = [order_matters(x[:split], models, delays, n_bins, 0), order_matters(x[split:], models, delays, n_bins, split)]
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    row_bytes = n_f * n_b * 4
    folder = api.PulsarFolder(bf, n_f, 64, n_bins, models, delays, max_in_flight=2)
    with pytest.raises(bfmod.DsabfError) as e:
        folder.collect()
    assert e.value.code == BF_ERR_STATE and str(e.value) == "libdsabf error -4: bf_psr_collect: no dump is pending"
    cuts = cuts_of(split, SIZES)
    push_all(torch, folder, d_x, row_bytes, cuts, streams)
    folder.dump(streams[1].cuda_stream)
    cuts2 = [(split + at, n) for at, n in cuts_of(n_rows - split, [64, 5])]
    push_all(torch, folder, d_x, row_bytes, cuts2, streams[::-1])
    folder.dump(streams[0].cuda_stream)
    assert folder.pending == 2
    with pytest.raises(bfmod.DsabfError) as e:
        folder.dump()
    assert e.value.code == BF_ERR_STATE
    assert str(e.value) == "libdsabf error -4: bf_psr_dump: 2 dumps are uncollected (max_in_flight): bf_psr_collect first"
    for (want_prof, want_hits), first, n in zip(want, (0, split), (split, n_rows - split)):
        prof, hits, first_row, got_rows = folder.collect()
        assert (first_row, got_rows) == (first, n)
        assert np.array_equal(hits, want_hits) and np.array_equal(bits(prof), bits(want_prof))
    assert folder.pending == 0
    with pytest.raises(bfmod.DsabfError) as e:
        folder.collect()
    assert e.value.code == BF_ERR_STATE and str(e.value) == "libdsabf error -4: bf_psr_collect: no dump is pending"
    folder.dump()                                       # an integration of no rows: zeros
    prof, hits, first_row, got_rows = folder.collect()
    assert (first_row, got_rows) == (n_rows, 0) and not hits.any() and not bits(prof).any()
    folder.close()
    bf.close()


def test_a_refused_dump_queues_and_zeroes_nothing(torch, bfmod):
    """max_in_flight 1 at the smallest shape of SHAPES (one pulsar, 2 bins, 1 channel, 4 beams): push, dump, and a second dump while the
    first is uncollected is refused with the whole message; after the collect, the next rows pushed on ANOTHER queue, dumped and
    collected are the oracle's fold of exactly those rows -- the refused dump copied nothing, zeroed nothing and did not move first_row."""
    from dsabeamformer_amd import api

    n_b, n_f, n_bins, n_rows, split = 4, 1, 2, 120, 71
    rng = np.random.default_rng(53)
    x = wide(rng, (n_rows, n_f, n_b))
    models = models_for(1, n_bins, n_rows, "fast")
    delays = np.zeros((1, n_f), np.int32)
    want = [order_matters(x[:split], models, delays, n_bins, 0), order_matters(x[split:], models, delays, n_bins, split)]
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    row_bytes = n_f * n_b * 4
    folder = api.PulsarFolder(bf, n_f, 64, n_bins, models, delays, max_in_flight=1)
    push_all(torch, folder, d_x, row_bytes, cuts_of(split, [64, 7]), streams[:1])
    folder.dump()
    with pytest.raises(bfmod.DsabfError) as e:
        folder.dump()
    assert e.value.code == BF_ERR_STATE and folder.pending == 1
    assert str(e.value) == "libdsabf error -4: bf_psr_dump: 1 dumps are uncollected (max_in_flight): bf_psr_collect first"
    prof, hits, first_row, got_rows = folder.collect()
    assert (first_row, got_rows) == (0, split)
    assert np.array_equal(hits, want[0][1]) and np.array_equal(bits(prof), bits(want[0][0]))
    push_all(torch, folder, d_x, row_bytes, [(split + at, n) for at, n in cuts_of(n_rows - split, [33, 16])], streams[1:])
    folder.dump()
    prof, hits, first_row, got_rows = folder.collect()
    assert (first_row, got_rows) == (split, n_rows - split) and int(hits.sum()) == (n_rows - split) * n_f
    assert np.array_equal(hits, want[1][1]) and np.array_equal(bits(prof), bits(want[1][0]))
    assert folder.pending == 0
    folder.close()
    bf.close()


def test_attached_to_a_dm_stage(torch, bfmod):
    """Behind a bf_dm_stream: the chunks with a folder attached are the chunks without one, bit for bit; the folder's profile is the
    oracle's on the rows as the DM stage saw them -- raw (the wide-range input: the order of the adds matters, asserted), and, with a
    Conditioner attached, cond_oracle's output.  In that leg the order cannot matter: conditioned rows are fp32 of unit variance, and
    150 of them sum without a rounding in fp64 whatever the input (values below 2^-29 of the sum would be needed); what the leg shows is
    WHICH rows were folded -- the profile is the oracle's on the conditioned rows and is not the one of the raw rows."""
    from dsabeamformer_amd import api

    n_b, n_f, n_dm, max_rows, n_rows, n_bins = 68, 8, 5, 32, 150, 16
    rng = np.random.default_rng(12)
    delays_dm = np.rint(9.0 * np.arange(n_dm)[:, None] / (n_dm - 1.0) * ((np.arange(n_f) / (n_f - 1.0)) ** 2)[None, :]).astype(np.int32)
    D = int(delays_dm.max())
    models = models_for(3, n_bins, n_rows, None)
    delays = delays_for(rng, 3, n_f, n_rows)
    raw = wide(rng, (n_rows, n_f, n_b))
    gain = (1.0 + 3.0 * rng.random(n_f)).astype(np.float32)
    powers = ((rng.random((n_rows, n_f, n_b), dtype=np.float32) * np.float32(1e3) + np.float32(10.0)) * gain[None, :, None]).astype(np.float32)
    cuts = cuts_of(n_rows, [32, 1, 7, 32, 3, 19])
    kw = dict(baseline_pushes=3, zero_dm=True, auto_threshold=0.0)
    co = cond_oracle.Conditioner(n_f, n_b, **kw)
    cooked = np.concatenate([co.push(powers[a:a + n]) for a, n in cuts])
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def run(series, fold, cond):
        d_series = torch.from_numpy(series).cuda()
        torch.cuda.synchronize()
        dm = api.DmStream(bf, delays_dm, n_f, max_rows)
        folder = api.PulsarFolder(bf, n_f, max_rows, n_bins, models, delays) if fold else None
        c = api.Conditioner(bf, n_f, max_rows, **kw) if cond else None
        if c is not None:
            dm.attach_conditioner(c)
        if folder is not None:
            dm.attach_folder(folder)
        hosts = [torch.full((n_dm * max_rows * n_b,), float("nan"), dtype=torch.float32).pin_memory() for _ in cuts]
        outs = []
        for k, (at, n) in enumerate(cuts):
            outs.append(dm.push(d_series.data_ptr() + at * n_f * n_b * 4, n, hosts[k], streams[k % 2].cuda_stream)[1])
        torch.cuda.synchronize()
        chunks = np.concatenate([h[:n_dm * n * n_b].numpy().reshape(n_dm, n, n_b) for h, n in zip(hosts, outs) if n], axis=1)
        result = None
        if folder is not None:
            folder.dump()
            result = folder.collect()
            # detached, the DM stage goes on and the folder sees nothing more
            dm.attach_folder(None)
            dm.push(d_series.data_ptr(), 4, None, streams[0].cuda_stream)
            folder.dump()
            assert folder.collect()[3] == 0
            folder.close()
        if c is not None:
            c.close()
        dm.close()
        return chunks, result

    plain, _ = run(raw, False, False)
    assert plain.shape == (n_dm, n_rows - D, n_b)
    with_fold, (prof, hits, first_row, got_rows) = run(raw, True, False)
    assert np.array_equal(with_fold.view(np.uint32), plain.view(np.uint32))
    want_prof, want_hits = order_matters(raw, models, delays, n_bins)
    assert (first_row, got_rows) == (0, n_rows) and np.array_equal(hits, want_hits) and np.array_equal(bits(prof), bits(want_prof))
    # behind the conditioner: the fold sees conditioned rows
    cond_plain, _ = run(powers, False, True)
    cond_fold, (prof, hits, first_row, got_rows) = run(powers, True, True)
    assert np.array_equal(cond_fold.view(np.uint32), cond_plain.view(np.uint32))
    want_prof, want_hits = psr_oracle.fold(cooked, models, delays, n_bins)
    assert (first_row, got_rows) == (0, n_rows) and np.array_equal(hits, want_hits) and np.array_equal(bits(prof), bits(want_prof))
    assert not np.array_equal(bits(prof), bits(psr_oracle.fold(powers, models, delays, n_bins)[0]))     # conditioned rows, not raw ones
    # attaches that are refused
    dm = api.DmStream(bf, delays_dm, n_f, max_rows)
    other = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    for bad, msg in ((api.PulsarFolder(bf, n_f + 1, max_rows, n_bins, models, np.zeros((3, n_f + 1), np.int32)), "channels"),
                     (api.PulsarFolder(bf, n_f, max_rows - 1, n_bins, models, delays), "max_rows_per_push"),
                     (api.PulsarFolder(other, n_f, max_rows, n_bins, models, delays), "different handles")):
        with pytest.raises(bfmod.DsabfError, match=msg) as e:
            dm.attach_folder(bad)
        assert e.value.code == BF_ERR_INVALID
        bad.close()
    folder = api.PulsarFolder(bf, n_f, max_rows, n_bins, models, delays)
    dm.attach_folder(folder)
    dm2 = api.DmStream(bf, delays_dm, n_f, max_rows)
    with pytest.raises(bfmod.DsabfError, match="another DM stage") as e:
        dm2.attach_folder(folder)
    assert e.value.code == BF_ERR_STATE
    folder.close()                                      # destroying an attached folder detaches it: the DM stage goes on
    d_series = torch.from_numpy(raw).cuda()
    assert dm.push(d_series, max_rows, None, 0) == (0, max_rows - D)
    torch.cuda.synchronize()
    dm2.close()
    dm.close()
    other.close()
    bf.close()


def test_the_handle_goes_first(torch, bfmod):
    from dsabeamformer_amd import api

    n_b, n_f, n_bins, n_rows = 64, 3, 16, 64
    x = wide(np.random.default_rng(4), (n_rows, n_f, n_b))
    models = models_for(1, n_bins, n_rows, "slow")
    delays = np.zeros((1, n_f), np.int32)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    d_x = torch.from_numpy(x).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    folder = api.PulsarFolder(bf, n_f, n_rows, n_bins, models, delays)
    folder.push(d_x, n_rows, st.cuda_stream)
    folder.dump()
    bf.close()                                          # with the push and the dump in flight
    for call in (lambda: folder.push(d_x, 1, 0), folder.dump, folder.collect):
        with pytest.raises(bfmod.DsabfError, match="pulsar folder") as e:
            call()
        assert e.value.code == BF_ERR_STATE
    folder.close()
    torch.cuda.synchronize()


def test_a_pulsar_is_found(torch, bfmod):
    """A periodic pulse in ONE beam column of a noise stream, dispersed by the integer delays, folded at the true model and at one 1 % off
    in f0 (two pulsars of one folder: one read of the rows).  Orderings only: no S/N is fixed in advance."""
    from dsabeamformer_amd import api

    n_b, n_f, n_bins, n_rows, beam, target = 16, 8, 64, 4096, 11, 40
    row = 0.131072e-3
    f0 = 1.0 / (37.3 * row)
    rng = np.random.default_rng(1)
    true = psr_oracle.model_from_spin(f0, 0.0, 0.2, row, 0)
    off = psr_oracle.model_from_spin(f0 * 1.01, 0.0, 0.2, row, 0)
    d1 = np.rint(30.0 * (1.0 - np.arange(n_f) / (n_f - 1.0)) ** 2).astype(np.int32)
    delays = np.stack([d1, d1])
    x = rng.standard_normal((n_rows, n_f, n_b)).astype(np.float32)
    x[:, :, beam] += np.where(psr_oracle.bins(true, d1, 0, n_rows, n_bins) == target, np.float32(1.0), np.float32(0.0))
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    folder = api.PulsarFolder(bf, n_f, 512, n_bins, [true, off], delays)
    push_all(torch, folder, d_x, n_f * n_b * 4, cuts_of(n_rows, [512]), streams)
    folder.dump()
    prof, hits, _, _ = folder.collect()
    want_prof, want_hits = psr_oracle.fold(x, [true, off], delays, n_bins)
    assert np.array_equal(hits, want_hits) and np.array_equal(bits(prof), bits(want_prof))
    snr_true, peak_true = api.PulsarFolder.beam_snr(prof[0], hits[0])
    snr_off, _ = api.PulsarFolder.beam_snr(prof[1], hits[1])
    print("S/N of the injected beam: true model %.2f, 1 %% off %.2f; the best other beam %.2f" %
          (snr_true[beam], snr_off[beam], np.delete(snr_true, beam).max()))
    assert int(np.argmax(snr_true)) == beam and np.all(np.delete(snr_true, beam) < snr_true[beam])
    assert peak_true[beam] == target
    assert snr_off[beam] < snr_true[beam]
    folder.close()
    bf.close()


def test_refusals_launch_nothing(torch, bfmod):
    from dsabeamformer_amd import _lib, api

    lib = _lib.load()
    n_b, n_f, n_bins, max_rows = 8, 5, 4, 6
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    models = (_lib.BfPsrModel * 5)()
    delays = np.zeros((5, n_f), np.int32)

    def create(n_freq=n_f, rows=max_rows, bins_=n_bins, n_psr=1, in_flight=2, handle=bf._h, m=models, d=delays, out=True):
        p = C.c_void_p()
        rc = lib.bf_psr_create(handle, n_freq, rows, bins_, C.cast(m, C.c_void_p) if m is not None else None, d.ctypes.data if d is not None else None,
                               n_psr, in_flight, C.byref(p) if out else None)
        assert (rc == 0) == bool(p.value)
        return rc, p

    neg = delays.copy()
    neg[0, 2] = -1
    for kw in (dict(bins_=1), dict(bins_=4097), dict(n_psr=0), dict(n_psr=5), dict(n_freq=0), dict(rows=0), dict(in_flight=0), dict(handle=None),
               dict(m=None), dict(d=None), dict(out=False), dict(d=neg)):
        assert create(**kw)[0] == BF_ERR_INVALID, kw
    for kw in (dict(bins_=2), dict(bins_=4096, n_psr=4)):
        rc, p = create(**kw)
        assert rc == 0 and lib.bf_psr_destroy(p) == 0
    x = wide(np.random.default_rng(6), (max_rows + 1, n_f, n_b))
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    folder = api.PulsarFolder(bf, n_f, max_rows, n_bins, [(0, ONE // 7, 0, 0)], delays[:1])
    for args in ((folder._c, d_x.data_ptr(), 0), (folder._c, d_x.data_ptr(), max_rows + 1), (folder._c, d_x.data_ptr(), -2), (folder._c, None, 1),
                 (None, d_x.data_ptr(), 1)):
        assert lib.bf_psr_push(args[0], args[1], args[2], None) == BF_ERR_INVALID, args
    assert lib.bf_psr_collect(folder._c, None, None, None, None) == BF_ERR_INVALID
    # an epoch that puts |n| at 2^31: the whole push is refused, one row inside the range is not
    for epoch, delay, ok in ((-(1 << 31), 0, False), (1 << 31, 0, False), ((1 << 31) - 1, 0, True), ((1 << 31) - 3, 3, False), (-(1 << 31) + max_rows - 1, 0, False),
                             (-(1 << 31) + max_rows - 1, 1, True)):
        far = api.PulsarFolder(bf, n_f, max_rows, n_bins, [(0, ONE // 7, 0, epoch)], np.full((1, n_f), delay, np.int32))
        rc = lib.bf_psr_push(far._c, d_x.data_ptr(), max_rows, None)
        assert rc == (0 if ok else BF_ERR_INVALID), (epoch, delay)
        if not ok:
            assert b"re-anchor epoch_row" in lib.bf_last_error()
        far.dump()
        prof, hits, _, got_rows = far.collect()
        assert got_rows == (max_rows if ok else 0) and int(hits.sum()) == got_rows * n_f and (ok or not bits(prof).any())
        far.close()
    folder.dump()
    prof, hits, first_row, got_rows = folder.collect()
    assert (first_row, got_rows) == (0, 0) and not hits.any() and not bits(prof).any()
    folder.close()
    bf.close()


def test_beam_cli_fold(tmp_path):
    """`beam -j 29 -M 40 -N 4 -T 0.02 --fold 31.7:-0.4:0.3 --fold-dm 25 --fold 1200 --fold-bins 16 --fold-rows 512 --fold-out folds.bin -w raw.bin`,
    in a child process: 25 burn-in reads + 4 analysed blocks of the production geometry, 256 rows each.  The file parses with the oracle's
    reader and holds two dumps of 512 rows; the hits sum to the rows folded; and both dumps are the oracle's fold of the -w file's rows at
    the models and delays the driver derives (bf_psr_model_from_spin at the row time, dsabf::dm_delays at the run's channels)."""
    from dsabeamformer_amd import build, host

    n_an, tsamp, n_bins, dump_rows = 4, 0.02, 16, 512
    raw_file, fold_file = tmp_path / "raw.bin", tmp_path / "folds.bin"
    r = subprocess.run([build.BEAM, "-j", str(25 + n_an), "-M", "40", "-N", "4", "-T", str(tsamp), "--fold", "31.7:-0.4:0.3", "--fold-dm", "25", "--fold", "1200",
                        "--fold-bins", str(n_bins), "--fold-rows", str(dump_rows), "--fold-out", str(fold_file), "-w", str(raw_file)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert "Pulsar folder: 2 pulsars, 16 bins, 2 dumps" in r.stdout, r.stdout[-2000:]
    raw = dm_side.read_rows(raw_file)                                # [gemm][output][f][b]: rows in time order
    assert raw.shape[0] == 2 * dump_rows
    # (the comparison itself: tests/support/dm_side.py, shared with the trial-split runs of tests/test_gpu_trial_split.py)
    _, freq, _ = dm_side.beam_ladder(40.0, 4, raw.shape[1], tsamp)
    delays = host.dm_delays(np.array([25.0, 0.0]), freq, float(freq[0]), tsamp)
    assert delays.shape == (2, raw.shape[1]) and delays[0].max() > 0 and not delays[1].any()
    recs = dm_side.check_folds(fold_file, raw, freq, tsamp, [(31.7, -0.4, 0.3), (1200.0, 0.0, 0.0)], [25.0, 0.0], n_bins, dump_rows)
    assert [(q["first_row"], q["n_rows"]) for q in recs] == [(0, dump_rows), (dump_rows, dump_rows)]
