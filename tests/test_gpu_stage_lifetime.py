"""GPU tests (-m gpu) of what the four stage objects of a handle share: their place on the handle, the order in which handle and
stages may be destroyed, and that a create / destroy cycle gives back what it took.  Public API only (dsabeamformer_amd.api): the
file says nothing about how the runtime keeps its stages, and every comparison of device output is np.array_equal."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import corr_oracle  # noqa: E402
import sk_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_STATE = -4
N_F, N_B, N_DM, ROWS, N_WIDTHS, COND_WINDOW, AUTO_THRESHOLD, CORR_IN_FLIGHT = 8, 64, 4, 16, 3, 2, 5.0, 2
# delays[k][f] = k (7 - f) / 4, rounded down: trial 0 is undispersed, the largest delay is 5
DELAYS = np.array([[k * (N_F - 1 - f) // 4 for f in range(N_F)] for k in range(N_DM)], np.int32)
D = int(DELAYS.max())
# Free device memory after cycle 2 minus free memory after cycle 4 of test_four_cycles_give_back_what_they_took, as the runtime
# with one hand-written release per stage kind measured it (bytes): the bar, with no margin on top.
CYCLE_DROP_BEFORE_THE_SHARED_BASE = 0


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _handle(bfmod):
    return bfmod.Beamformer(bfmod.production_config(n_freq=N_F, n_beams=N_B, n_gemms_per_block=1, n_blocks_on_gpu=1, n_streams=1))


def _stages(bf, kinds):
    """The stages named in `kinds`, created in that order: "dm", "corr", "sps", "cond"."""
    from dsabeamformer_amd import api

    make = {"dm": lambda: api.DmStream(bf, DELAYS, N_F, ROWS),
            "corr": lambda: api.Correlator(bf, CORR_IN_FLIGHT),
            "sps": lambda: api.SinglePulseSearch(bf, N_DM, N_WIDTHS, ROWS, min_samples=ROWS - D, threshold=-1e300),
            "cond": lambda: api.Conditioner(bf, N_F, ROWS, baseline_pushes=COND_WINDOW, auto_threshold=AUTO_THRESHOLD)}
    return [make[k]() for k in kinds]


def _rows(seed, n_pushes):
    return (np.random.default_rng(seed).random((n_pushes * ROWS, N_F, N_B), dtype=np.float32) * 1e3).astype(np.float32)


def _run(torch, dm, sps, cond, d_rows, n_pushes):
    """n_pushes pushes of ROWS rows on a side stream, the search collected after every push that emits: chunks, candidates, mask."""
    st = torch.cuda.Stream()
    host = torch.zeros(N_DM * ROWS * N_B, dtype=torch.float32).pin_memory()
    chunks, cands, at = [], [], 0
    for k in range(n_pushes):
        first, n_out = dm.push(d_rows.data_ptr() + k * ROWS * N_F * N_B * 4, ROWS, host, st.cuda_stream)
        assert first == at and n_out == (ROWS - D if k == 0 else ROWS)
        at += n_out
        cands.append(sps.collect())
        st.synchronize()
        chunks.append(host[:N_DM * n_out * N_B].numpy().reshape(N_DM, n_out, N_B).copy())
    return chunks, cands, cond.mask()


def test_stages_of_every_kind_share_one_handle(torch, bfmod):
    """Handle A gets DM1, a correlator, a search stage, a conditioner and DM2, in that order; DM1 and the correlator are destroyed
    (the first and an interior stage of those the handle keeps), the search and the conditioner attached to DM2.  Three pushes of
    seeded rows give, bit for bit, the chunks, the candidates and the mask of handle B, which only ever had one DM stage, one search
    stage and one conditioner.  The counter of ring stages on A follows DM2's creation, DM1's destruction and DM2's."""
    rows = _rows(11, 3)
    d_rows = torch.from_numpy(rows).cuda()
    a = _handle(bfmod)
    dm1, = _stages(a, ["dm"])
    ring = a.counter("dm_ring_stages")          # 1: the twice-mapped ring; 0: a device without virtual-memory management
    assert ring in (0, 1)
    corr, sps, cond, dm2 = _stages(a, ["corr", "sps", "cond", "dm"])
    assert a.counter("dm_ring_stages") == 2 * ring
    dm1.close()
    assert a.counter("dm_ring_stages") == ring
    corr.close()
    dm2.attach_search(sps)
    dm2.attach_conditioner(cond)
    got = _run(torch, dm2, sps, cond, d_rows, 3)
    dm2.close()
    assert a.counter("dm_ring_stages") == 0
    sps.close()
    cond.close()
    a.close()

    b = _handle(bfmod)
    dm, sps, cond = _stages(b, ["dm", "sps", "cond"])
    dm.attach_search(sps)
    dm.attach_conditioner(cond)
    want = _run(torch, dm, sps, cond, d_rows, 3)
    for s in (sps, cond, dm):
        s.close()
    b.close()

    assert sum(len(c) for c in want[1]) > 0 and sum(c.shape[1] for c in want[0]) == 3 * ROWS - D
    for k in range(3):
        assert np.array_equal(got[0][k], want[0][k]), k
        assert got[1][k].dtype == want[1][k].dtype and got[1][k].shape == want[1][k].shape
        for name in want[1][k].dtype.names:
            assert np.array_equal(got[1][k][name], want[1][k][name]), (k, name)
    assert np.array_equal(got[2], want[2])


def test_the_handle_goes_first_with_every_stage_attached_and_in_flight(torch, bfmod, orc):
    """All four kinds on one handle, search and conditioner attached to the DM stage, one push of each feed on a side stream and no
    synchronisation: the handle is destroyed.  Every call on every stage then answers BF_ERR_STATE, "... has been destroyed"; the
    stages are destroyed -- one attached stage before the DM stage it pointed at, one after -- and a new handle on the same device
    computes the oracle's chunk."""
    rows = _rows(12, 1)
    d_rows = torch.from_numpy(rows).cuda()
    bf = _handle(bfmod)
    d_packed = torch.from_numpy(np.random.default_rng(13).integers(0, 256, bf.bytes_per_gemm, dtype=np.uint8)).cuda()
    dm, corr, sps, cond = _stages(bf, ["dm", "corr", "sps", "cond"])
    dm.attach_search(sps)
    dm.attach_conditioner(cond)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert dm.push(d_rows, ROWS, None, st.cuda_stream) == (0, ROWS - D)
    corr.push(d_packed, 1, st.cuda_stream)
    corr.dump(st.cuda_stream)
    bf.close()
    calls = {"dm.push": lambda: dm.push(d_rows, ROWS), "dm.reserve": lambda: dm.reserve(ROWS), "dm.attach_search": lambda: dm.attach_search(sps),
             "dm.attach_conditioner": lambda: dm.attach_conditioner(cond), "dm.detach": lambda: dm.attach_search(None),
             "sps.push": lambda: sps.push(d_rows, ROWS, 0), "sps.collect": sps.collect,
             "cond.push": lambda: cond.push(d_rows, ROWS), "cond.set_mask": lambda: cond.set_mask(np.zeros(N_F, np.uint8)),
             "corr.push": lambda: corr.push(d_packed, 1), "corr.dump": corr.dump, "corr.collect": corr.collect}
    for name, call in calls.items():
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE and "has been destroyed" in str(e.value), (name, str(e.value))
    for s in (sps, dm, cond, corr):
        s.close()

    from dsabeamformer_amd import api

    bf = _handle(bfmod)
    dm = api.DmStream(bf, DELAYS, N_F, ROWS)
    host = torch.zeros(N_DM * ROWS * N_B, dtype=torch.float32).pin_memory()
    assert dm.push(d_rows, ROWS, host, st.cuda_stream) == (0, ROWS - D)
    st.synchronize()
    got = host[:N_DM * (ROWS - D) * N_B].numpy().reshape(N_DM, ROWS - D, N_B)
    assert np.array_equal(got, orc.dedisperse_dm(rows, DELAYS, ROWS - D))
    dm.close()
    bf.close()


def test_four_cycles_give_back_what_they_took(torch, bfmod):
    """Four times: a handle, the four kinds, attach, one push of each feed, synchronise, destroy the stages, destroy the handle.  Free
    device memory after cycle 4 is not below free memory after cycle 2 by more than CYCLE_DROP_BEFORE_THE_SHARED_BASE (cycle 1 pays
    for the first kernel loads and the ring's address arena)."""
    d_rows = torch.from_numpy(_rows(14, 1)).cuda()
    d_packed = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    free = []
    for _ in range(4):
        bf = _handle(bfmod)
        assert bf.bytes_per_gemm <= d_packed.numel()
        dm, corr, sps, cond = _stages(bf, ["dm", "corr", "sps", "cond"])
        dm.attach_search(sps)
        dm.attach_conditioner(cond)
        assert dm.push(d_rows, ROWS) == (0, ROWS - D)
        corr.push(d_packed, 1)
        torch.cuda.synchronize()
        for s in (dm, corr, sps, cond):
            s.close()
        bf.close()
        free.append(torch.cuda.mem_get_info()[0])
    print("free device memory after each cycle:", free, "drop from cycle 2 to cycle 4: %d bytes" % (free[1] - free[3]))
    assert free[1] - free[3] <= CYCLE_DROP_BEFORE_THE_SHARED_BASE, free


def test_a_correlator_and_a_moments_stage_on_one_handle_keep_their_own_state(torch, bfmod):
    """The correlator and the moments stage are one accumulator stage underneath: whatever that base kept per kind and not per
    instance -- an accumulator, a column count, the event chain, the dump counters -- would show here.  One of each on one handle, both
    with max_in_flight 1, two ring slots of different voltages: slot 0 into both on queue 0, a dump of the correlator alone, slot 1
    into both on queue 1, a dump of both.  Bit for bit the correlator's dumps are slot 0 alone and slot 1 alone, the moments' single
    dump is the sum of both with the summed column count; the correlator's full set refuses its second dump and leaves the moments
    stage with nothing pending."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(43)
    cfg = bfmod.debug_config(n_ant=100, n_pol=2, n_avg=2, n_beams=8, n_freq=3, n_out_per_gemm=8, n_gemms_per_block=4, n_blocks_on_gpu=2,
                             n_streams=4)                                        # tests/test_gpu_sk.py's push_block geometry
    n_u, cols = cfg.n_gemms_per_block, cfg.n_gemms_per_block * cfg.n_out_per_gemm * cfg.n_avg
    blocks = rng.integers(0, 256, size=(2, n_u, cfg.n_freq, cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg, cfg.n_ant), dtype=np.uint8)
    want_vis = [corr_oracle.visibilities(b, 2) for b in blocks]
    want_mom = sk_oracle.moments(blocks.reshape((2 * n_u,) + blocks.shape[2:]), 2)
    assert not np.array_equal(want_vis[0], want_vis[1])
    bf = bfmod.Beamformer(cfg)
    corr, sk = api.Correlator(bf, 1), api.SpectralKurtosis(bf, 1)
    pin = torch.from_numpy(blocks).pin_memory()
    for slot in (0, 1):
        bf.submit_block(slot, pin[slot], blocks[slot].nbytes)
    bf.sync(-1)
    for stage in (corr, sk):
        stage.push_block(0, 0, 0, n_u)
    corr.dump()
    for stage in (corr, sk):
        stage.push_block(1, 1, 0, n_u)
    with pytest.raises(bfmod.DsabfError) as e:
        corr.dump()
    assert e.value.code == BF_ERR_STATE, str(e.value)
    assert str(e.value) == "libdsabf error -4: bf_corr_dump: 1 dumps are uncollected (max_in_flight): bf_corr_collect first"
    assert corr.pending == 1 and sk.pending == 0
    vis, n_columns = corr.collect()                                              # makes room for the correlator's second dump
    assert n_columns == cols and np.array_equal(vis, want_vis[0])
    corr.dump()
    sk.dump()
    assert corr.pending == 1 and sk.pending == 1
    vis, n_columns = corr.collect()
    assert n_columns == cols and np.array_equal(vis, want_vis[1])
    mom, n_columns = sk.collect()
    assert n_columns == 2 * cols and np.array_equal(mom, want_mom)
    assert corr.pending == 0 and sk.pending == 0
    for s in (corr, sk):
        s.close()
    bf.close()
