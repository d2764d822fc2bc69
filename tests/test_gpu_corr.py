"""GPU tests (-m gpu) of the correlator (include/dsabf.h: bf_correlate_device, bf_corr_*; docs/CORRELATOR.md).  The reference is
tests/support/corr_oracle.py -- a nibble table and an int64 einsum -- and every comparison of visibilities is np.array_equal: the sums
are exact integers, so there is no tolerance to state.  The one floating-point comparison (the beams as the quadratic form of the
visibilities) uses the bound include/dsabf.h states for the detect.

Every test is ONE function that loops over its cases, as tests/test_gpu_incoherent.py does: the sweep cap of conftest.py thins
parametrised cases, and none of these may be left out."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

SUPPORT = os.path.join(ROOT, "tests", "support")
sys.path.insert(0, SUPPORT)
import corr_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _cfg(bfmod, n_ant, n_pol, n_avg, n_out, n_beams=8, n_freq=3, **over):
    kw = dict(n_ant=n_ant, n_pol=n_pol, n_avg=n_avg, n_beams=n_beams, n_freq=n_freq, n_out_per_gemm=n_out, n_gemms_per_block=4,
              n_blocks_on_gpu=2, n_streams=4)
    kw.update(over)
    return bfmod.debug_config(**kw)


def _random_packed(rng, cfg, n_units):
    return rng.integers(0, 256, size=(n_units, cfg.n_freq, cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg, cfg.n_ant), dtype=np.uint8)


def _vis_shape(cfg):
    return (cfg.n_freq, cfg.n_pol, corr_oracle.n_baselines(cfg.n_ant), 2)


def _sentinel(torch, cfg):
    return torch.full(_vis_shape(cfg), SENTINEL, dtype=torch.int64, device="cuda")


# columns per polarisation and unit -> (n_out_per_gemm, n_avg): both sides of one K step of the (r | m) form (32) and of a full 64
COLUMNS = {1: (1, 1), 3: (3, 1), 32: (2, 16), 33: (3, 11), 64: (4, 16), 65: (5, 13)}
# (n_ant, columns, n_pol, n_freq, n_units).  4 and 256 antennas -- the smallest and the largest -- meet every column count, both
# polarisation counts, both channel counts and both unit counts; the tile shapes in between one or two cases each.
TILE_CASES = [(4, 1, 1, 1, 1), (4, 3, 2, 3, 3), (4, 32, 1, 3, 1), (4, 33, 2, 1, 3), (4, 64, 2, 3, 1), (4, 65, 1, 1, 3),
              (16, 33, 2, 3, 1),                      # exactly one tile
              (20, 65, 2, 1, 3), (20, 3, 1, 3, 1),    # a ragged off-diagonal tile
              (64, 32, 2, 3, 3), (64, 65, 1, 1, 1),   # C3's antennas: one full super-tile
              (100, 33, 2, 3, 1), (100, 64, 1, 1, 3),  # C5's ragged seventh tile; a second super-tile row
              (132, 3, 2, 1, 3), (132, 65, 2, 3, 1),  # across 128: three super-tile rows, the last one tile deep
              (256, 1, 2, 3, 3), (256, 3, 1, 1, 1), (256, 32, 2, 1, 1), (256, 33, 1, 3, 3), (256, 64, 1, 3, 1), (256, 65, 2, 1, 3)]


def test_every_tile_shape_and_column_count_to_the_bit(torch, bfmod):
    """bf_correlate_device against the oracle on random bytes: antenna counts 4, 16, 20, 64, 100, 132, 256 (less than a tile, one
    tile, a ragged off-diagonal tile, C3, C5's ragged seventh tile, across 128, the maximum), 1, 3, 32, 33, 64, 65 columns per
    polarisation and unit, n_pol 1 and 2, 1 and 3 channels, 1 and 3 units.  The output is filled with a sentinel first and compared
    whole: a store outside the triangle, or one left out, shows.  No weights are set: the call needs none."""
    for lst, idx in (((4, 16, 20, 64, 100, 132, 256), 0), (tuple(COLUMNS), 1), ((1, 2), 2), ((1, 3), 3), ((1, 3), 4)):
        for n_ant in (4, 256) if idx else (None,):
            have = {c[idx] for c in TILE_CASES if n_ant is None or c[0] == n_ant}
            assert have == set(lst), (idx, n_ant, have)
    rng = np.random.default_rng(20261018)
    t0, n = time.perf_counter(), 0
    for n_ant, cols, n_pol, n_freq, n_units in TILE_CASES:
        n_out, n_avg = COLUMNS[cols]
        cfg = _cfg(bfmod, n_ant, n_pol, n_avg, n_out, n_freq=n_freq)
        assert cfg.n_out_per_gemm * cfg.n_avg == cols
        packed = _random_packed(rng, cfg, n_units)
        want = corr_oracle.visibilities(packed, n_pol)
        bf = bfmod.Beamformer(cfg)
        assert bf.corr_entries * 2 == want.size
        d_vis = _sentinel(torch, cfg)
        bf.correlate(torch.from_numpy(packed).cuda(), n_units, d_vis)
        torch.cuda.synchronize()
        got = d_vis.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, ((n_ant, cols, n_pol, n_freq, n_units), len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        bf.close()
        n += want.size
    print("corr_kernel: %d cases, %d int64 compared, %.1f s" % (len(TILE_CASES), n, time.perf_counter() - t0))


def test_every_pair_of_byte_codes(torch, bfmod):
    """4 antennas, one polarisation, 65536 columns: antenna 0 carries c % 256, antenna 1 c // 256, antenna 2 the constant 0x88
    (-8-8i), antenna 3 0x80 (-8): every product of two byte codes, the extremes included, to the bit."""
    cfg = _cfg(bfmod, 4, 1, 16, 64, n_freq=1)                                # 1024 columns per unit x 64 units
    c = np.arange(65536)
    packed = np.stack([c % 256, c // 256, np.full(65536, 0x88), np.full(65536, 0x80)], axis=-1).astype(np.uint8).reshape(64, 1, 1024, 4)
    want = corr_oracle.visibilities(packed, 1)
    r, m = corr_oracle.RE, corr_oracle.IM                                    # the closed form of two entries, as a check of the oracle's input
    assert want[0, 0, corr_oracle.bl(0, 0), 0] == 256 * int((r * r + m * m).sum())
    assert tuple(want[0, 0, corr_oracle.bl(1, 0)]) == (int(r.sum()) ** 2 + int(m.sum()) ** 2, 0) == (32768, 0)   # every pair of codes once
    assert tuple(want[0, 0, corr_oracle.bl(3, 2)]) == (64 * 65536, -64 * 65536)   # (-8) conj(-8 - 8i) = 64 - 64i, summed
    bf = bfmod.Beamformer(cfg)
    d_vis = _sentinel(torch, cfg)
    bf.correlate(torch.from_numpy(packed).cuda(), 64, d_vis)
    torch.cuda.synchronize()
    got = d_vis.cpu().numpy()
    assert np.array_equal(got, want), (got[0, 0].tolist(), want[0, 0].tolist())
    bf.close()


def test_accumulate_adds_and_store_overwrites(torch, bfmod):
    """Two calls with accumulate = 1 into a zeroed array equal the oracle over both inputs; accumulate = 0 ignores a sentinel-filled
    array; accumulate = 1 on the sentinel adds to it."""
    rng = np.random.default_rng(3)
    for n_ant, cols, n_pol in ((20, 33, 2), (132, 65, 1)):
        n_out, n_avg = COLUMNS[cols]
        cfg = _cfg(bfmod, n_ant, n_pol, n_avg, n_out)
        a, b = _random_packed(rng, cfg, 2), _random_packed(rng, cfg, 3)
        want_a, want_ab = corr_oracle.visibilities(a, n_pol), corr_oracle.visibilities(np.concatenate([a, b]), n_pol)
        bf = bfmod.Beamformer(cfg)
        d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        d_vis = torch.zeros(_vis_shape(cfg), dtype=torch.int64, device="cuda")
        bf.correlate(d_a, 2, d_vis, accumulate=True)
        bf.correlate(d_b, 3, d_vis, accumulate=True)
        torch.cuda.synchronize()
        assert np.array_equal(d_vis.cpu().numpy(), want_ab), n_ant
        d_s = _sentinel(torch, cfg)
        bf.correlate(d_a, 2, d_s, accumulate=False)
        torch.cuda.synchronize()
        assert np.array_equal(d_s.cpu().numpy(), want_a), n_ant
        d_s = _sentinel(torch, cfg)
        bf.correlate(d_a, 2, d_s, accumulate=True)
        torch.cuda.synchronize()
        assert np.array_equal(d_s.cpu().numpy(), want_a + SENTINEL), n_ant
        bf.close()


def test_the_exactness_bound(torch, bfmod):
    """4 antennas, N = 2^24 - 1 columns of 0x88 (64 MiB; 4095 columns x 4097 units): every entry's re is 128 N exactly -- one short of
    2^31 -- and im is 0.  A geometry and unit count with N = 2^24 is refused by bf_correlate_device and by bf_corr_push and nothing is
    launched (an untouched sentinel, an empty dump); 260 antennas are refused."""
    from dsabeamformer_amd import api

    small = dict(n_freq=1, n_gemms_per_block=1, n_blocks_on_gpu=1, n_streams=1)
    cfg = _cfg(bfmod, 4, 1, 1, 4095, **small)
    n_units = 4097
    N = n_units * 4095
    assert N == 2 ** 24 - 1 and 128 * N == 2 ** 31 - 128
    bf = bfmod.Beamformer(cfg)
    d_in = torch.full((n_units * 4095 * 4,), 0x88, dtype=torch.uint8, device="cuda")
    d_vis = _sentinel(torch, cfg)
    t0 = time.perf_counter()
    bf.correlate(d_in, n_units, d_vis)
    torch.cuda.synchronize()
    print("N = 2^24 - 1 columns in one workgroup: %.2f s" % (time.perf_counter() - t0))
    got = d_vis.cpu().numpy()
    assert np.all(got[..., 0] == 128 * N) and np.all(got[..., 1] == 0), got.reshape(-1, 2)[:4]
    bf.close()
    over = bfmod.Beamformer(_cfg(bfmod, 4, 1, 1, 4096, **small))             # 4096 x 4096 = 2^24 columns
    d_vis = _sentinel(torch, over.cfg)
    with pytest.raises(bfmod.DsabfError, match="2\\^24") as e:
        over.correlate(d_in, 4096, d_vis)
    assert e.value.code == BF_ERR_INVALID
    stage = api.Correlator(over, 2)
    with pytest.raises(bfmod.DsabfError, match="2\\^24") as e:
        stage.push(d_in, 4096)
    assert e.value.code == BF_ERR_INVALID
    stage.dump()
    vis, n_columns = stage.collect()
    torch.cuda.synchronize()
    assert n_columns == 0 and not vis.any() and torch.all(d_vis == SENTINEL).item()   # nothing was launched
    over.correlate(d_in, 4095, d_vis)                                        # one unit fewer: inside the bound
    torch.cuda.synchronize()
    assert torch.all(d_vis[..., 0] == 128 * 4095 * 4096).item()
    stage.close()
    over.close()
    wide = bfmod.Beamformer(_cfg(bfmod, 260, 2, 1, 2, **small))
    d_vis = torch.full((2 * 260 * 261,), SENTINEL, dtype=torch.int64, device="cuda")
    with pytest.raises(bfmod.DsabfError, match="256") as e:
        wide.correlate(d_in, 1, d_vis)
    assert e.value.code == BF_ERR_INVALID
    with pytest.raises(bfmod.DsabfError, match="256") as e:
        api.Correlator(wide, 2)
    assert e.value.code == BF_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(d_vis == SENTINEL).item()
    wide.close()


def test_pushes_on_two_queues_without_synchronisation(torch, bfmod):
    """A stage fed ragged unit counts alternately on two streams with no host synchronisation between the pushes, dumps in mid-run,
    max_in_flight 2: every collected record equals the oracle over exactly the pushes in front of its dump, with the right column
    count; a third uncollected dump is refused with BF_ERR_STATE, twice in the run (and queues nothing: the next record is complete; one integration is empty); the handle is
    destroyed before the stage."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(17)
    cfg = _cfg(bfmod, 64, 2, 11, 3, n_freq=24)                               # 33 columns per polarisation and unit
    cols = 33
    packed = _random_packed(rng, cfg, 40)
    per_unit = packed[0].size
    bf = bfmod.Beamformer(cfg)
    stage = api.Correlator(bf, 2)
    d_in = torch.from_numpy(packed).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    counts = [1, 7, 2, 5, None, 3, 9, 1, None, None, 4, 6, 2, None]         # None: a dump
    at, k, groups, first = 0, 0, [], 0
    with pytest.raises(bfmod.DsabfError) as e:
        stage.collect()
    assert e.value.code == BF_ERR_STATE and stage.pending == 0
    refused = 0
    for c in counts:
        if c is None:
            if stage.pending == 2:
                with pytest.raises(bfmod.DsabfError) as e:
                    stage.dump()
                assert e.value.code == BF_ERR_STATE and stage.pending == 2
                refused += 1
                vis, n_columns = stage.collect()                             # the oldest: make room, then dump
                lo, hi = groups.pop(0)
                assert n_columns == (hi - lo) * cols and np.array_equal(vis, corr_oracle.visibilities(packed[lo:hi], 2)), (lo, hi)
            stage.dump(streams[k % 2].cuda_stream)
            groups.append((first, at))
            first = at
            continue
        stage.push(d_in.data_ptr() + at * per_unit, c, streams[k % 2].cuda_stream)
        at, k = at + c, k + 1
    assert at == 40 and refused == 2 and stage.pending == 2
    for lo, hi in groups:
        vis, n_columns = stage.collect()
        assert n_columns == (hi - lo) * cols and np.array_equal(vis, corr_oracle.visibilities(packed[lo:hi], 2)), (lo, hi)
    assert stage.pending == 0
    bf.close()                                                               # the handle first: the stage answers BF_ERR_STATE and can be destroyed
    for call in (lambda: stage.push(d_in, 1), stage.dump, stage.collect):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE
    stage.close()


def test_the_beams_are_the_quadratic_form_of_the_visibilities(torch, bfmod):
    """One identity ties the new code to the old.  One gemm-unit, random int8 weights (imaginary parts in [-127, 127]), canonical
    detect: sum over o of out[o][f][b] from bf_beamform_device against
        E = alpha^2 * sum over p, a1, a2 of W[f][a1][b] conj(W[f][a2][b]) V[f][p][a1][a2],   alpha = float32(1 / 127),
    with E evaluated in exact integers from the GPU's visibilities.  Bound (include/dsabf.h): |out - E| <= (n_ipo + 4) 2^-24 E per
    output window, hence for the sum over o.  The left-hand side takes nothing from the correlator."""
    rng = np.random.default_rng(29)
    alpha = float(np.float32(1.0 / 127.0))
    for n_ant, n_beams in ((20, 8), (64, 16)):
        cfg = _cfg(bfmod, n_ant, 2, 4, 3, n_beams=n_beams, n_freq=3)
        n_ipo = cfg.n_pol * cfg.n_avg
        packed = _random_packed(rng, cfg, 1)
        w = rng.integers(-127, 128, size=(cfg.n_freq, n_ant, n_beams, 2), dtype=np.int8)
        bf = bfmod.Beamformer(cfg)
        bf.set_weights(w)
        d_in = torch.from_numpy(packed).cuda()
        d_out = torch.zeros((cfg.n_out_per_gemm, cfg.n_freq, n_beams), dtype=torch.float32, device="cuda")
        d_vis = _sentinel(torch, cfg)
        bf.beamform(d_in, 1, d_out)
        bf.correlate(d_in, 1, d_vis)
        torch.cuda.synchronize()
        lhs = d_out.cpu().numpy().astype(np.float64).sum(axis=0)             # [f][b]: exact sums of float32 values
        vis = d_vis.cpu().numpy()
        assert np.array_equal(vis, corr_oracle.visibilities(packed, 2))
        vr, vi = vis.sum(axis=1)[..., 0], vis.sum(axis=1)[..., 1]            # summed over p: [f][bl], int64
        a1, a2 = np.tril_indices(n_ant)
        off = a1 != a2
        wr, wi = w[..., 0].astype(np.int64), w[..., 1].astype(np.int64)      # [f][a][b]
        # W1 conj(W2) V + its Hermitian mirror = 2 re(W1 conj(W2) V) off the diagonal; |W|^2 V on it -- all int64, no rounding
        pr = wr[:, a1] * wr[:, a2] + wi[:, a1] * wi[:, a2]                   # re(W1 conj(W2)): [f][bl][b]
        pi = wi[:, a1] * wr[:, a2] - wr[:, a1] * wi[:, a2]                   # im
        term = pr * vr[..., None] - pi * vi[..., None]
        e_int = 2 * term[:, off].sum(axis=1) + term[:, ~off].sum(axis=1)     # [f][b]
        assert np.all(e_int > 0)
        e = alpha * alpha * e_int.astype(np.float64)
        err = np.abs(lhs - e) / e
        bound = (n_ipo + 4) * 2.0 ** -24
        print("%d antennas x %d beams: largest |sum_o out - E| / E = %.3g (bound %.3g)" % (n_ant, n_beams, err.max(), bound))
        assert np.all(err <= bound), (n_ant, err.max(), bound)
        bf.close()


# ---- the resident block and the driver ----------------------------------------------------------------------------------------------
N_ANALYSED = 2      # `-j 27`: the junk source counts the 25 burn-in reads (BURNIN), so 2 blocks are analysed


def _junk_ring(host, cfg):
    n_time = cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg
    return host.junk_bytes(cfg.n_ant * cfg.n_freq * n_time * cfg.n_gemms_per_block, 4, 0xD5A, cfg).reshape(
        4, cfg.n_gemms_per_block, cfg.n_freq, n_time, cfg.n_ant)


def _vis_of_the_run(host, cfg):
    """The oracle's visibilities of the blocks a `beam -j 27` run analyses, one per block (block i is junk block (25 + i) % 4).  The
    float64 route of the oracle (exact, and equal to the int64 einsum: tests/test_corr_cpu.py) over 128 MiB blocks; channels 0 and
    the last are held against the einsum here as well."""
    ring = _junk_ring(host, cfg)
    out = []
    for i in range(N_ANALYSED):
        blk = ring[(25 + i) % 4]
        v = corr_oracle.visibilities_f64(blk, cfg.n_pol)
        for f in (0, cfg.n_freq - 1):
            assert np.array_equal(v[f], corr_oracle.visibilities(blk[:, f:f + 1], cfg.n_pol)[0])
        out.append(v)
    return out


def _check_header(hdr, cfg, first_channel):
    assert hdr["CONTENT"] == "visibilities" and hdr["DTYPE"] == "int64" and int(hdr["HDR_SIZE"]) == 4096
    assert (int(hdr["NANT"]), int(hdr["NPOL"]), int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"])) == (cfg.n_ant, cfg.n_pol, cfg.n_freq, first_channel)
    assert hdr["LAYOUT"] == "freq,pol,baseline(lower triangle a1*(a1+1)/2+a2),reim"


def test_push_block_and_the_observation_loop(torch, bfmod, tmp_path):
    """bf_submit_block, bf_enqueue_block, bf_corr_push_block on the same queue for two blocks on alternating slots: the dump equals the
    oracle over the submitted bytes.  Then `beam -j 27 -a 1 -V vis.bin -L 1` (observation mode runs the production geometry whatever -a
    says, as for every other option of that mode): two records whose headers and entries equal the oracle over the junk source's
    blocks (regenerated with host.junk_bytes: bfh_junk_fill); -L 2 gives one record that is their sum; -L 3 none (an incomplete
    integration is dropped)."""
    from dsabeamformer_amd import api, build, host

    rng = np.random.default_rng(41)
    cfg = _cfg(bfmod, 100, 2, 2, 8)                                          # 16 columns per polarisation and unit, 4 units per block
    n_u = cfg.n_gemms_per_block
    blocks = np.stack([_random_packed(rng, cfg, n_u) for _ in range(2)])
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(rng.integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8))
    stage = api.Correlator(bf, 2)
    pin = torch.from_numpy(blocks).pin_memory()
    for slot in (0, 1):
        bf.submit_block(slot, pin[slot], blocks[slot].nbytes)
    bf.sync(-1)
    for slot in (0, 1):                                                      # the second block in two launches, as units_per_launch would
        for first, n in (((0, n_u),) if slot == 0 else ((0, 1), (1, n_u - 1))):
            bf.enqueue_block(slot, slot, first, n, None)
            stage.push_block(slot, slot, first, n)
    stage.dump()
    vis, n_columns = stage.collect()
    assert n_columns == 2 * n_u * 16 and np.array_equal(vis, corr_oracle.visibilities(blocks.reshape((2 * n_u,) + blocks.shape[2:]), 2))
    for bad in ((4, 0, 0, 1), (0, 2, 0, 1), (0, 0, n_u, 1), (0, 0, 1, n_u)):
        with pytest.raises(bfmod.DsabfError) as e:
            stage.push_block(*bad)
        assert e.value.code == BF_ERR_INVALID
    stage.close()
    bf.close()
    # ---- the driver
    pcfg = bfmod.production_config()
    want = _vis_of_the_run(host, pcfg)
    n_cols = pcfg.n_gemms_per_block * pcfg.n_out_per_gemm * pcfg.n_avg
    for blocks_per_dump, records in ((1, [(0, n_cols, want[0]), (1, n_cols, want[1])]), (2, [(0, 2 * n_cols, want[0] + want[1])]), (3, [])):
        path = tmp_path / ("vis%d.bin" % blocks_per_dump)
        r = subprocess.run([build.BEAM, "-j", str(25 + N_ANALYSED), "-a", "1", "-V", str(path), "-L", str(blocks_per_dump)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Correlator: %d dumps of %d blocks" % (len(records), blocks_per_dump) in r.stdout, r.stdout
        hdr, dumps = host.read_vis_file(str(path))
        _check_header(hdr, pcfg, 0)
        assert [(d[0], d[1]) for d in dumps] == [(rec[0], rec[1]) for rec in records], blocks_per_dump
        for d, rec in zip(dumps, records):
            assert np.array_equal(d[2], rec[2]), (blocks_per_dump, d[0])


def test_two_loopback_ranks_write_their_own_channels(bfmod, tmp_path):
    """`beam -j 27 -R 2 -r k -V vis.bin` as two shard processes (the stand-in RCCL library and launch pattern of
    tests/test_gpu_incoherent.py): vis.bin.0 and vis.bin.1 carry FIRST_CHANNEL 0 and n_freq, and each equals the oracle over its
    rank's input -- every shard reads the junk bytes with ITS geometry (128 channels), so both see the same bytes."""
    from test_gpu_multirank import FAKE  # noqa: F401  (built by that module's fixture; build here if it has not run)

    from dsabeamformer_amd import build, host

    src = os.path.join(SUPPORT, "fake_rccl.cpp")
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(src):
        obj = os.path.join(SUPPORT, "fake_rccl.o")
        subprocess.check_call([build.HIPCC, "-O2", "-std=c++17", "-fPIC", "-c", src, "-o", obj])
        cxx = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
        subprocess.check_call([cxx if os.path.exists(cxx) else "g++", "-shared", "-fPIC", "-o", FAKE, obj, "-lpthread", "-lrt"])
    vis = tmp_path / "vis.bin"
    cmd = lambda rk: [build.BEAM, "-j", str(25 + N_ANALYSED), "-D", "0", "-R", "2", "-r", str(rk), "-I", str(tmp_path / "id"),  # noqa: E731
                      "-V", str(vis), "-L", "2"]
    procs = [subprocess.Popen(cmd(rk), env=dict(os.environ, DSABF_RCCL_LIB=FAKE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for rk in (0, 1)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("Correlator: 1 dumps of 2 blocks" in o for o in outs), "\n".join(outs)
    assert not os.path.exists(vis)
    shard = bfmod.production_config(n_freq=128)
    want = sum(_vis_of_the_run(host, shard))
    n_cols = N_ANALYSED * shard.n_gemms_per_block * shard.n_out_per_gemm * shard.n_avg
    for rk in (0, 1):
        hdr, dumps = host.read_vis_file(str(vis) + ".%d" % rk)
        _check_header(hdr, shard, rk * 128)
        assert [(d[0], d[1]) for d in dumps] == [(0, n_cols)]
        assert np.array_equal(dumps[0][2], want), rk
