"""GPU tests (-m gpu) of the voltage moments and the spectral-kurtosis flags (include/dsabf.h: bf_sk_device, bf_sk_*;
docs/SPECTRAL_KURTOSIS.md).  The reference is tests/support/sk_oracle.py -- a 256-entry table and an int64 reshape-sum -- and every
comparison of moments is np.array_equal on whole sentinel-filled outputs: the sums are exact integers, so there is no tolerance to
state.  The gains of the last test are compared to the bit with tests/support/cal_oracle.py.

Every test is ONE function that loops over its cases, as tests/test_gpu_corr.py does: the sweep cap of conftest.py thins
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
import cal_oracle  # noqa: E402
import corr_oracle  # noqa: E402
import sk_oracle  # noqa: E402

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


def _shape(cfg):
    return (cfg.n_freq, cfg.n_pol, cfg.n_ant, 2)


def _sentinel(torch, cfg):
    return torch.full(_shape(cfg), SENTINEL, dtype=torch.int64, device="cuda")


# columns per polarisation and unit -> (n_out_per_gemm, n_avg); 1024 is the large case's
COLUMNS = {1: (1, 1), 3: (3, 1), 32: (2, 16), 33: (3, 11), 1024: (64, 16)}
# (n_ant, columns, n_pol, n_freq, n_units).  4 and 256 antennas meet every column count, both polarisation counts, both channel
# counts and both unit counts; the other antenna counts one or two cases each.  16-byte words where n_ant % 16 == 0 (16, 64, 256,
# 2048), 4-byte words otherwise; n_ant * time % 16 is non-zero in (4, 1, 1, ..), (4, 3, 2, ..), (20, 3, 1, ..), (68, 33, 1, ..),
# (100, 33, 1, ..), (132, 3, 1, ..) and (260, 1, 1, ..).  More than 1024 antennas x polarisations: several antenna chunks (2048).
SPAN_CASES = [(4, 1, 1, 1, 1), (4, 3, 2, 3, 3), (4, 32, 1, 3, 1), (4, 33, 2, 1, 3),
              (16, 33, 2, 3, 1), (20, 3, 1, 3, 1), (20, 32, 2, 1, 3),
              (64, 32, 2, 3, 3), (64, 1, 1, 1, 1), (68, 33, 1, 1, 3), (100, 33, 1, 3, 1), (100, 32, 2, 1, 3),
              (132, 3, 1, 1, 3), (132, 33, 2, 3, 1),
              (256, 1, 2, 3, 3), (256, 3, 1, 1, 1), (256, 32, 2, 1, 1), (256, 33, 1, 3, 3),
              (260, 1, 1, 3, 1), (260, 32, 2, 1, 3), (2048, 3, 2, 1, 3), (2048, 33, 1, 3, 1)]
# The large case: 64 antennas, 2 polarisations, 3 channels, 48 units of 1024 columns (18 MiB).  A workgroup's row-block is 64 columns:
# 3 * 48 * 32 = 4608 row-blocks, more than four per workgroup of the largest launch (4 workgroups per CU on 256 CUs), so the
# workgroups walk ranges that are cut by the cap, not by the input, and some of them cross from one channel to the next.
LARGE_CASE = (64, 1024, 2, 3, 48)


def test_every_span_shape_and_column_count_to_the_bit(torch, bfmod):
    """bf_sk_device against the oracle on random bytes: antenna counts 4 ... 2048 (both load widths, ragged lane rows, several antenna
    chunks), 1, 3, 32, 33 columns per polarisation and unit, n_pol 1 and 2, 1 and 3 channels, 1 and 3 units, and one large case.  The
    output is filled with a sentinel first and compared whole.  No weights are set: the call needs none."""
    for lst, idx in (((4, 16, 20, 64, 68, 100, 132, 256, 260, 2048), 0), ((1, 3, 32, 33), 1), ((1, 2), 2), ((1, 3), 3), ((1, 3), 4)):
        for n_ant in (4, 256) if idx else (None,):
            have = {c[idx] for c in SPAN_CASES if n_ant is None or c[0] == n_ant}
            assert have == set(lst), (idx, n_ant, have)
    assert {c[0] * COLUMNS[c[1]][0] * COLUMNS[c[1]][1] * c[2] % 16 == 0 for c in SPAN_CASES} == {True, False}
    rng = np.random.default_rng(20261019)
    t0, n = time.perf_counter(), 0
    for n_ant, cols, n_pol, n_freq, n_units in SPAN_CASES + [LARGE_CASE]:
        n_out, n_avg = COLUMNS[cols]
        cfg = _cfg(bfmod, n_ant, n_pol, n_avg, n_out, n_freq=n_freq)
        assert cfg.n_out_per_gemm * cfg.n_avg == cols
        packed = _random_packed(rng, cfg, n_units)
        want = sk_oracle.moments(packed, n_pol)
        bf = bfmod.Beamformer(cfg)
        assert bf.sk_entries * 2 == want.size
        d_mom = _sentinel(torch, cfg)
        bf.voltage_moments(torch.from_numpy(packed).cuda(), n_units, d_mom)
        torch.cuda.synchronize()
        got = d_mom.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, ((n_ant, cols, n_pol, n_freq, n_units), len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        bf.close()
        n += want.size
    print("moments_kernel: %d cases, %d int64 compared, %.1f s" % (len(SPAN_CASES) + 1, n, time.perf_counter() - t0))


def test_every_byte_code_in_every_lane_position(torch, bfmod):
    """64 antennas x 256 columns, one polarisation: antenna a sees code (c + a) % 256 at column c, so every code lands in every byte
    lane of a 16-byte word (and of a 4-byte one: the same bytes at 68 antennas, where the words are 4 bytes)."""
    for n_ant in (64, 68):
        cfg = _cfg(bfmod, n_ant, 1, 16, 16, n_freq=1)                            # 256 columns in one unit
        c, a = np.meshgrid(np.arange(256), np.arange(n_ant), indexing="ij")
        packed = ((c + a) % 256).astype(np.uint8).reshape(1, 1, 256, n_ant)
        want = sk_oracle.moments(packed, 1)
        assert np.all(want[0, 0, :, 0] == int(sk_oracle.P.sum())) and np.all(want[0, 0, :, 1] == int(sk_oracle.P2.sum()))
        bf = bfmod.Beamformer(cfg)
        d_mom = _sentinel(torch, cfg)
        bf.voltage_moments(torch.from_numpy(packed).cuda(), 1, d_mom)
        torch.cuda.synchronize()
        got = d_mom.cpu().numpy()
        assert np.array_equal(got, want), (n_ant, got[0, 0, :4].tolist(), want[0, 0, :4].tolist())
        bf.close()


def test_accumulate_adds_and_store_overwrites(torch, bfmod):
    """Two calls with accumulate = 1 into a zeroed array equal the oracle over both inputs; accumulate = 0 ignores a sentinel-filled
    array; accumulate = 1 on the sentinel adds to it."""
    rng = np.random.default_rng(3)
    for n_ant, cols, n_pol in ((20, 33, 2), (256, 32, 1)):
        n_out, n_avg = COLUMNS[cols]
        cfg = _cfg(bfmod, n_ant, n_pol, n_avg, n_out)
        a, b = _random_packed(rng, cfg, 2), _random_packed(rng, cfg, 3)
        want_a, want_ab = sk_oracle.moments(a, n_pol), sk_oracle.moments(np.concatenate([a, b]), n_pol)
        bf = bfmod.Beamformer(cfg)
        d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        d_mom = torch.zeros(_shape(cfg), dtype=torch.int64, device="cuda")
        bf.voltage_moments(d_a, 2, d_mom, accumulate=True)
        bf.voltage_moments(d_b, 3, d_mom, accumulate=True)
        torch.cuda.synchronize()
        assert np.array_equal(d_mom.cpu().numpy(), want_ab), n_ant
        d_s = _sentinel(torch, cfg)
        bf.voltage_moments(d_a, 2, d_s, accumulate=False)
        torch.cuda.synchronize()
        assert np.array_equal(d_s.cpu().numpy(), want_a), n_ant
        d_s = _sentinel(torch, cfg)
        bf.voltage_moments(d_a, 2, d_s, accumulate=True)
        torch.cuda.synchronize()
        assert np.array_equal(d_s.cpu().numpy(), want_a + SENTINEL), n_ant
        bf.close()


def test_the_exactness_bound(torch, bfmod):
    """4 antennas, N = 2^24 - 1 columns of 0x88 (64 MiB; 4095 columns x 4097 units), n_pol = 1: M1 = 128 N and M2 = 16384 N exactly.
    N = 2^24 is refused by bf_sk_device and by bf_sk_push and nothing is launched (an untouched sentinel, an empty dump)."""
    from dsabeamformer_amd import api

    small = dict(n_freq=1, n_gemms_per_block=1, n_blocks_on_gpu=1, n_streams=1)
    cfg = _cfg(bfmod, 4, 1, 1, 4095, **small)
    n_units = 4097
    N = n_units * 4095
    assert N == 2 ** 24 - 1
    bf = bfmod.Beamformer(cfg)
    d_in = torch.full((n_units * 4095 * 4,), 0x88, dtype=torch.uint8, device="cuda")
    d_mom = _sentinel(torch, cfg)
    t0 = time.perf_counter()
    bf.voltage_moments(d_in, n_units, d_mom)
    torch.cuda.synchronize()
    print("N = 2^24 - 1 columns: %.2f s" % (time.perf_counter() - t0))
    got = d_mom.cpu().numpy()
    assert np.all(got[..., 0] == 128 * N) and np.all(got[..., 1] == 16384 * N), got.reshape(-1, 2)[:4]
    bf.close()
    over = bfmod.Beamformer(_cfg(bfmod, 4, 1, 1, 4096, **small))                 # 4096 x 4096 = 2^24 columns
    d_mom = _sentinel(torch, over.cfg)
    with pytest.raises(bfmod.DsabfError, match="2\\^24") as e:
        over.voltage_moments(d_in, 4096, d_mom)
    assert e.value.code == BF_ERR_INVALID
    stage = api.SpectralKurtosis(over, 2)
    with pytest.raises(bfmod.DsabfError, match="2\\^24") as e:
        stage.push(d_in, 4096)
    assert e.value.code == BF_ERR_INVALID
    stage.dump()
    mom, n_columns = stage.collect()
    torch.cuda.synchronize()
    assert n_columns == 0 and not mom.any() and torch.all(d_mom == SENTINEL).item()   # nothing was launched
    over.voltage_moments(d_in, 4095, d_mom)                                      # one unit fewer: inside the bound
    torch.cuda.synchronize()
    assert torch.all(d_mom[..., 0] == 128 * 4095 * 4096).item() and torch.all(d_mom[..., 1] == 16384 * 4095 * 4096).item()
    stage.close()
    over.close()


def test_m1_is_the_correlators_diagonal(torch, bfmod):
    """At 64 and 132 antennas M1 == re(V[a][a]) from bf_correlate_device on the same device buffer: two independent kernels (MFMA with
    time as the K axis; per-byte dots) agree on the same exact integers."""
    rng = np.random.default_rng(5)
    for n_ant in (64, 132):
        cfg = _cfg(bfmod, n_ant, 2, 11, 3)
        packed = _random_packed(rng, cfg, 3)
        bf = bfmod.Beamformer(cfg)
        d_in = torch.from_numpy(packed).cuda()
        d_mom = _sentinel(torch, cfg)
        d_vis = torch.full((cfg.n_freq, cfg.n_pol, corr_oracle.n_baselines(n_ant), 2), SENTINEL, dtype=torch.int64, device="cuda")
        bf.voltage_moments(d_in, 3, d_mom)
        bf.correlate(d_in, 3, d_vis)
        torch.cuda.synchronize()
        mom, vis = d_mom.cpu().numpy(), d_vis.cpu().numpy()
        diag = [corr_oracle.bl(a, a) for a in range(n_ant)]
        assert np.array_equal(mom[..., 0], vis[:, :, diag, 0]) and not vis[:, :, diag, 1].any(), n_ant
        assert np.array_equal(mom, sk_oracle.moments(packed, 2))
        bf.close()


def test_pushes_on_two_queues_without_synchronisation(torch, bfmod):
    """A stage fed ragged unit counts alternately on two streams with no host synchronisation between the pushes, dumps in mid-run,
    max_in_flight 2: every collected record equals the oracle over exactly the pushes in front of its dump, with the right column
    count; a third uncollected dump is refused with BF_ERR_STATE (and queues nothing: the next record is complete); the handle is
    destroyed before the stage."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(17)
    cfg = _cfg(bfmod, 64, 2, 11, 3, n_freq=24)                                   # 33 columns per polarisation and unit
    cols = 33
    packed = _random_packed(rng, cfg, 40)
    per_unit = packed[0].size
    bf = bfmod.Beamformer(cfg)
    stage = api.SpectralKurtosis(bf, 2)
    d_in = torch.from_numpy(packed).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    counts = [1, 7, 2, 5, None, 3, 9, 1, None, None, 4, 6, 2, None]             # None: a dump
    at, k, groups, first = 0, 0, [], 0
    with pytest.raises(bfmod.DsabfError) as e:
        stage.collect()
    assert e.value.code == BF_ERR_STATE and stage.pending == 0
    assert str(e.value) == "libdsabf error -4: bf_sk_collect: no dump is pending"
    refused = 0
    for c in counts:
        if c is None:
            if stage.pending == 2:
                with pytest.raises(bfmod.DsabfError) as e:
                    stage.dump()
                assert e.value.code == BF_ERR_STATE and stage.pending == 2
                assert str(e.value) == "libdsabf error -4: bf_sk_dump: 2 dumps are uncollected (max_in_flight): bf_sk_collect first"
                refused += 1
                mom, n_columns = stage.collect()                                 # the oldest: make room, then dump
                lo, hi = groups.pop(0)
                assert n_columns == (hi - lo) * cols and np.array_equal(mom, sk_oracle.moments(packed[lo:hi], 2)), (lo, hi)
            stage.dump(streams[k % 2].cuda_stream)
            groups.append((first, at))
            first = at
            continue
        stage.push(d_in.data_ptr() + at * per_unit, c, streams[k % 2].cuda_stream)
        at, k = at + c, k + 1
    assert at == 40 and refused == 2 and stage.pending == 2
    for lo, hi in groups:
        mom, n_columns = stage.collect()
        want = sk_oracle.moments(packed[lo:hi], 2) if hi > lo else np.zeros(_shape(cfg), np.int64)
        assert n_columns == (hi - lo) * cols and np.array_equal(mom, want), (lo, hi)
    assert stage.pending == 0
    bf.close()                                                                   # the handle first: the stage answers BF_ERR_STATE and can be destroyed
    for call in (lambda: stage.push(d_in, 1), stage.dump, stage.collect):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE
    stage.close()


# ---- the resident block and the driver ----------------------------------------------------------------------------------------------
N_ANALYSED = 2      # `-j 27`: the junk source counts the 25 burn-in reads (BURNIN), so 2 blocks are analysed
_RUN_MOMENTS = {}   # n_freq of the geometry -> the oracle's moments of the analysed blocks (computed once, shared by two tests)


def _moments_of_the_run(host, cfg):
    """The oracle's moments of the blocks a `beam -j 27` run analyses, one per block (block i is junk block (25 + i) % 4, regenerated with
    host.junk_bytes as tests/test_gpu_corr.py does for -V), unit by unit to keep the table look-ups small."""
    if cfg.n_freq not in _RUN_MOMENTS:
        n_time = cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg
        ring = host.junk_bytes(cfg.n_ant * cfg.n_freq * n_time * cfg.n_gemms_per_block, 4, 0xD5A, cfg).reshape(
            4, cfg.n_gemms_per_block, cfg.n_freq, n_time, cfg.n_ant)
        _RUN_MOMENTS[cfg.n_freq] = [sum(sk_oracle.moments(ring[(25 + i) % 4][u:u + 1], cfg.n_pol) for u in range(cfg.n_gemms_per_block))
                                    for i in range(N_ANALYSED)]
    return _RUN_MOMENTS[cfg.n_freq]


def _check_header(hdr, cfg, first_channel):
    assert hdr["CONTENT"] == "voltage_moments" and hdr["DTYPE"] == "int64" and int(hdr["HDR_SIZE"]) == 4096
    assert (int(hdr["NANT"]), int(hdr["NPOL"]), int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"])) == (cfg.n_ant, cfg.n_pol, cfg.n_freq, first_channel)
    assert hdr["LAYOUT"] == "freq,pol,ant,m1m2"


def test_push_block_and_the_observation_loop(torch, bfmod, tmp_path):
    """bf_submit_block, bf_enqueue_block, bf_sk_push_block on the same queue for two blocks on alternating slots: the dump equals the
    oracle over the submitted bytes.  Then `beam -j 27 -a 1 -Y m.bin -J 1`: two records whose headers and entries equal the oracle over
    the junk source's blocks; -J 2 gives one record that is their sum; -J 3 none (an incomplete integration is dropped)."""
    from dsabeamformer_amd import api, build, host

    rng = np.random.default_rng(41)
    cfg = _cfg(bfmod, 100, 2, 2, 8)                                              # 16 columns per polarisation and unit, 4 units per block
    n_u = cfg.n_gemms_per_block
    blocks = np.stack([_random_packed(rng, cfg, n_u) for _ in range(2)])
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(rng.integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8))
    stage = api.SpectralKurtosis(bf, 2)
    pin = torch.from_numpy(blocks).pin_memory()
    for slot in (0, 1):
        bf.submit_block(slot, pin[slot], blocks[slot].nbytes)
    bf.sync(-1)
    for slot in (0, 1):                                                          # the second block in two launches, as units_per_launch would
        for first, n in (((0, n_u),) if slot == 0 else ((0, 1), (1, n_u - 1))):
            bf.enqueue_block(slot, slot, first, n, None)
            stage.push_block(slot, slot, first, n)
    stage.dump()
    mom, n_columns = stage.collect()
    assert n_columns == 2 * n_u * 16 and np.array_equal(mom, sk_oracle.moments(blocks.reshape((2 * n_u,) + blocks.shape[2:]), 2))
    for bad in ((4, 0, 0, 1), (0, 2, 0, 1), (0, 0, n_u, 1), (0, 0, 1, n_u)):
        with pytest.raises(bfmod.DsabfError) as e:
            stage.push_block(*bad)
        assert e.value.code == BF_ERR_INVALID
    stage.close()
    bf.close()
    # ---- the driver
    pcfg = bfmod.production_config()
    want = _moments_of_the_run(host, pcfg)
    n_cols = pcfg.n_gemms_per_block * pcfg.n_out_per_gemm * pcfg.n_avg
    for blocks_per_dump, records in ((1, [(0, n_cols, want[0]), (1, n_cols, want[1])]), (2, [(0, 2 * n_cols, want[0] + want[1])]), (3, [])):
        path = tmp_path / ("m%d.bin" % blocks_per_dump)
        r = subprocess.run([build.BEAM, "-j", str(25 + N_ANALYSED), "-a", "1", "-Y", str(path), "-J", str(blocks_per_dump)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Voltage moments: %d dumps of %d blocks" % (len(records), blocks_per_dump) in r.stdout, r.stdout
        hdr, dumps = host.read_moments_file(str(path))
        _check_header(hdr, pcfg, 0)
        assert [(d[0], d[1]) for d in dumps] == [(rec[0], rec[1]) for rec in records], blocks_per_dump
        for d, rec in zip(dumps, records):
            assert np.array_equal(d[2], rec[2]), (blocks_per_dump, d[0])


def _write_vis_file(path, cfg, first_channel, records):
    """A file of visibilities in the format `beam -V` writes (docs/CORRELATOR.md), for `beam -E`."""
    text = ("HDR_VERSION 1.0\nHDR_SIZE 4096\nINSTRUMENT DSA\nCONTENT visibilities\nDTYPE int64\nENDIAN little\n"
            "LAYOUT freq,pol,baseline(lower triangle a1*(a1+1)/2+a2),reim\nRECORD_HEADER_BYTES 16\nNANT %d\nNPOL %d\nNFREQ %d\nFIRST_CHANNEL %d\n"
            % (cfg.n_ant, cfg.n_pol, cfg.n_freq, first_channel)).encode()
    with open(path, "wb") as fp:
        fp.write(text.ljust(4096, b"\0"))
        for first_block, n_columns, vis in records:
            fp.write(np.array([first_block, n_columns], "<u8").tobytes() + np.ascontiguousarray(vis, "<i8").tobytes())


def _indices(path):
    return [int(x) for x in open(path).read().splitlines() if x.strip() and not x.startswith("#")]


def test_from_voltages_to_flagged_gains(torch, bfmod, tmp_path):
    """The loop the stage closes, at 16 antennas: the scene (sk_oracle.scene) with a common point-source term on every antenna, so that
    the visibilities have a solution.  voltage_moments -> sk_select on the GPU's moments flags exactly {5, 9, 12}; bf_solve_gains_device
    with those flags returns gains of exactly (0, 0) for the three and every gain bit-equal to cal_oracle with the same flags;
    bf_calibrate_weights_device gives them zero weights.  Then the same through the driver's files: the GPU's moments and visibilities
    in the formats `beam -Y` and `beam -V` write (the junk source of `beam -j` cannot carry a scene), `beam -e -O` -> `beam -E -G -f`:
    the flag file lists the three antennas and the gains file is bit-equal to the in-process gains."""
    from dsabeamformer_amd import api, build, host

    n_ant, n_pol, n_freq, n_units = 16, 2, 3, 4
    one = sk_oracle.scene(20261019, n_freq=n_freq, n_pol=n_pol, n_ant=n_ant, n_cols=4096, common=1.0)   # [1][freq][8192][ant]
    T = one.shape[2] // n_units
    packed = np.ascontiguousarray(one[0].reshape(n_freq, n_units, T, n_ant).transpose(1, 0, 2, 3))      # 4 units of 1024 columns per polarisation
    cfg = _cfg(bfmod, n_ant, n_pol, 16, 64, n_freq=n_freq)
    assert cfg.n_out_per_gemm * cfg.n_avg * n_pol == T
    M = 4096
    want_mom = sk_oracle.moments(packed, n_pol)
    assert np.array_equal(want_mom, sk_oracle.moments(one, n_pol))
    o_sk, o_cell, o_ant, o_chan = sk_oracle.select(want_mom, M)
    assert tuple(np.flatnonzero(o_ant)) == sk_oracle.SCENE_BAD and not o_chan.any()    # the oracle alone, before anything of the library's
    bf = bfmod.Beamformer(cfg)
    d_in = torch.from_numpy(packed).cuda()
    d_mom = _sentinel(torch, cfg)
    bf.voltage_moments(d_in, n_units, d_mom)
    torch.cuda.synchronize()
    mom = d_mom.cpu().numpy()
    assert np.array_equal(mom, want_mom)
    sk, cell, ant, chan = api.sk_select(mom, M)
    assert np.array_equal(sk.view(np.uint64), o_sk.view(np.uint64)) and np.array_equal(cell, o_cell)
    assert tuple(np.flatnonzero(ant)) == sk_oracle.SCENE_BAD and not chan.any()
    # ---- flags -> gains -> weights
    d_vis = torch.full((n_freq, n_pol, corr_oracle.n_baselines(n_ant), 2), SENTINEL, dtype=torch.int64, device="cuda")
    d_g = torch.full((n_pol, n_freq, n_ant, 2), float("nan"), dtype=torch.float64, device="cuda")
    d_i = torch.full((n_pol, n_freq, 2), -1, dtype=torch.int32, device="cuda")
    d_flags = torch.from_numpy(ant).cuda()
    bf.correlate(d_in, n_units, d_vis)
    bf.solve_gains(d_vis, d_g, d_i, flags=d_flags)
    torch.cuda.synchronize()
    vis, gains, info = d_vis.cpu().numpy(), d_g.cpu().numpy(), d_i.cpu().numpy()
    assert np.array_equal(vis, corr_oracle.visibilities(packed, n_pol))
    want_g, want_i = cal_oracle.solve(vis, n_ant, flags=ant)
    assert np.array_equal(info, want_i) and np.array_equal(gains.view(np.uint64), np.ascontiguousarray(want_g).view(np.uint64))
    bad = list(sk_oracle.SCENE_BAD)
    good = [a for a in range(n_ant) if a not in bad]
    assert not gains[:, :, bad].any() and np.all(np.hypot(gains[:, :, good, 0], gains[:, :, good, 1]) > 0)
    rng = np.random.default_rng(9)
    w = rng.integers(-127, 128, size=(n_freq, n_ant, cfg.n_beams, 2), dtype=np.int8)
    d_w = torch.full(w.shape, 0x7F, dtype=torch.int8, device="cuda")
    bf.calibrate_weights(torch.from_numpy(w).cuda(), d_g[0], d_w, flags=d_flags)
    torch.cuda.synchronize()
    got_w = d_w.cpu().numpy()
    assert np.array_equal(got_w, cal_oracle.calibrate_weights(w, gains[0], ant)) and not got_w[:, bad].any() and got_w[:, good].any()
    bf.close()
    # ---- the same through the driver's files
    mom_file, vis_file, ant_file, chan_file, gains_file = (str(tmp_path / n) for n in ("m.bin", "vis.bin", "ant.txt", "chan.txt", "gains.bin"))
    sk_oracle.write_moments_file(mom_file, 0, [(0, M // 2, mom // 2), (1, M // 2, mom - mom // 2)])   # two records: beam -e sums them
    _write_vis_file(vis_file, cfg, 0, [(0, M, vis)])
    r = subprocess.run([build.BEAM, "-e", mom_file, "-O", ant_file, "-q", chan_file], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _indices(ant_file) == bad and _indices(chan_file) == []
    r = subprocess.run([build.BEAM, "-E", vis_file, "-G", gains_file, "-f", ant_file], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hdr, records = host.read_gains_file(gains_file)
    assert len(records) == 1 and records[0][:2] == (0, M)
    assert np.array_equal(np.ascontiguousarray(records[0][2]).view(np.uint64), gains.view(np.uint64)) and np.array_equal(records[0][3], info)
    r = subprocess.run([build.BEAM, "-E", vis_file, "-G", gains_file], capture_output=True, text=True, timeout=300)   # without -f: other gains
    assert r.returncode == 0, r.stdout + r.stderr
    assert host.read_gains_file(gains_file)[1][0][2][:, :, 5].any()


def test_beam_applies_gains_with_antenna_flags(bfmod, tmp_path):
    """`beam ... -A gains.bin -f antflags.txt` in the DEBUG run: the flags reach bf_calibrate_weights_device, where a flagged antenna and a
    zero-gain antenna both get zero weights -- so the table equals, byte for byte, the one of a gains file whose gains are zero at the
    flagged antennas, and differs from the one without -f."""
    from dsabeamformer_amd import build, host

    dbg = bfmod.debug_config()
    rng = np.random.default_rng(31)
    amp = rng.uniform(0.5, 1.5, size=(1, dbg.n_freq, dbg.n_ant))
    g = amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape))
    layer = np.stack([g.real, g.imag], axis=-1)
    zeroed = layer.copy()
    zeroed[:, :, list(sk_oracle.SCENE_BAD)] = 0.0
    info = np.ones((1, dbg.n_freq, 2), np.int32)
    full_path, zero_path, flags_path = (str(tmp_path / n) for n in ("gains.bin", "zeroed.bin", "ant.txt"))
    host.write_gains_file(full_path, n_ant=dbg.n_ant, n_pol=1, n_freq=dbg.n_freq, first_channel=0, records=[(0, 1, layer, info)])
    host.write_gains_file(zero_path, n_ant=dbg.n_ant, n_pol=1, n_freq=dbg.n_freq, first_channel=0, records=[(0, 1, zeroed, info)])
    open(flags_path, "w").write("# antennas\n" + "".join("%d\n" % a for a in sk_oracle.SCENE_BAD))
    cfgdir = os.path.join(ROOT, "tests", "golden", "config")
    files = ["-p", os.path.join(cfgdir, "linear_positions.txt"), "-d", os.path.join(cfgdir, "linear_directions.txt"),
             "-s", os.path.join(cfgdir, "linear_source_directions_1024.txt")]
    tables = {}
    for name, extra in (("flagged", ["-A", full_path, "-f", flags_path]), ("zeroed", ["-A", zero_path]), ("all", ["-A", full_path])):
        out = str(tmp_path / (name + ".py"))
        r = subprocess.run([build.BEAM] + files + extra + ["-o", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Calibrated the weights" in r.stdout and os.path.getsize(out) > 0, r.stdout + r.stderr
        tables[name] = open(out).read()
    assert tables["flagged"] == tables["zeroed"] and tables["flagged"] != tables["all"]


def test_two_loopback_ranks_write_their_own_channels(bfmod, tmp_path):
    """`beam -j 27 -R 2 -r k -Y m.bin` as two shard processes (the stand-in RCCL library and launch pattern of the correlator's test):
    m.bin.0 and m.bin.1 carry FIRST_CHANNEL 0 and 128, and each equals the oracle over its rank's input -- every shard reads the junk
    bytes with ITS geometry (128 channels), so both see the same bytes."""
    from test_gpu_multirank import FAKE  # noqa: F401  (built by that module's fixture; build here if it has not run)

    from dsabeamformer_amd import build, host

    src = os.path.join(SUPPORT, "fake_rccl.cpp")
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(src):
        obj = os.path.join(SUPPORT, "fake_rccl.o")
        subprocess.check_call([build.HIPCC, "-O2", "-std=c++17", "-fPIC", "-c", src, "-o", obj])
        cxx = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
        subprocess.check_call([cxx if os.path.exists(cxx) else "g++", "-shared", "-fPIC", "-o", FAKE, obj, "-lpthread", "-lrt"])
    mfile = tmp_path / "m.bin"
    cmd = lambda rk: [build.BEAM, "-j", str(25 + N_ANALYSED), "-D", "0", "-R", "2", "-r", str(rk), "-I", str(tmp_path / "id"),  # noqa: E731
                      "-Y", str(mfile), "-J", "2"]
    procs = [subprocess.Popen(cmd(rk), env=dict(os.environ, DSABF_RCCL_LIB=FAKE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for rk in (0, 1)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("Voltage moments: 1 dumps of 2 blocks" in o for o in outs), "\n".join(outs)
    assert not os.path.exists(mfile)
    shard = bfmod.production_config(n_freq=128)
    want = sum(_moments_of_the_run(host, shard))
    n_cols = N_ANALYSED * shard.n_gemms_per_block * shard.n_out_per_gemm * shard.n_avg
    for rk in (0, 1):
        hdr, dumps = host.read_moments_file(str(mfile) + ".%d" % rk)
        _check_header(hdr, shard, rk * 128)
        assert [(d[0], d[1]) for d in dumps] == [(0, n_cols)]
        assert np.array_equal(dumps[0][2], want), rk
