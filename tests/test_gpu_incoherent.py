"""GPU tests (-m gpu) of the incoherent beam (include/dsabf.h: bf_incoherent_device, bf_set_incoherent_beam; docs/INCOHERENT_BEAM.md).
The reference is tests/support/ib_oracle.py -- a table lookup and an integer sum -- and every comparison is np.array_equal: the
sums are exact integers below 2^24, so there is no tolerance to state.

Every test is ONE function that loops over its cases, as tests/test_gpu_sps_shapes.py does: the sweep cap of conftest.py thins
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
import ib_oracle  # noqa: E402
import sps_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID = -1
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _cfg(bfmod, n_ant, n_pol, n_avg, n_beams=8, n_freq=3, n_out=2, **over):
    kw = dict(n_ant=n_ant, n_pol=n_pol, n_avg=n_avg, n_beams=n_beams, n_freq=n_freq, n_out_per_gemm=n_out, n_gemms_per_block=4,
              n_blocks_on_gpu=2, n_streams=4)
    kw.update(over)
    return bfmod.debug_config(**kw)


def _random_packed(rng, cfg, n_units):
    n_ipo = cfg.n_pol * cfg.n_avg
    p = rng.integers(0, 256, size=(n_units, cfg.n_freq, cfg.n_out_per_gemm * n_ipo, cfg.n_ant), dtype=np.uint8)
    return p, n_ipo


# (n_ant, n_pol, n_avg): span bytes -> load width and lanes per output of incoherent_kernel (csrc/ib/bf_incoherent.hip)
ISSUE_SHAPES = [(4, 1, 1),        # 4 B: 4-byte words, one lane per span
                (64, 2, 1),       # 128 B, the DEBUG span: 16-byte words, 4 lanes
                (132, 2, 1),      # 264 B, 8- but not 16-aligned: 4-byte words, 16 lanes
                (100, 2, 3),      # 600 B: 4-byte words, 16 lanes, a ragged last trip
                (100, 2, 16),     # 3200 B = 200 16-byte words: ragged against every power-of-two lane group
                (64, 2, 16),      # 2048 B, C3: 16-byte words, 16 lanes
                (260, 2, 16)]     # 8320 B, the generic-kernel antenna class: 16-byte words, 64 lanes
# the classes the list above does not reach, and both sides of every threshold of incoherent_lanes (8, 32, 512 words)
EXTRA_SHAPES = [(4, 2, 2),        # 16 B: ONE 16-byte word, one lane per span
                (28, 2, 2),       # 112 B = 7 words of 16: the largest one-lane span
                (28, 1, 1),       # 28 B = 7 words of 4: one lane;  (4-byte words)
                (20, 2, 1),       # 40 B = 10 words of 4: 4 lanes
                (124, 2, 2),      # 496 B = 31 words of 16: the largest 4-lane span
                (128, 2, 2),      # 512 B = 32 words: the smallest 16-lane span
                (292, 1, 7),      # 2044 B = 511 words of 4: the largest 16-lane span
                (516, 1, 5)]      # 2580 B = 645 words of 4: 64 lanes with 4-byte words


def _check_shape(torch, bfmod, rng, shape, n_units, n_out=2):
    n_ant, n_pol, n_avg = shape
    n_beams = 8
    cfg = _cfg(bfmod, n_ant, n_pol, n_avg, n_beams=n_beams, n_out=n_out)
    packed, n_ipo = _random_packed(rng, cfg, n_units)
    assert packed.size >= 256
    packed.reshape(-1)[:256] = rng.permutation(256).astype(np.uint8)      # every byte code, from the first span on
    want = ib_oracle.incoherent(packed, cfg.n_out_per_gemm, n_ipo)       # [unit][o][f]
    bf = bfmod.Beamformer(cfg)                                             # (no weights: the incoherent beam needs none)
    d_in = torch.from_numpy(packed).cuda()
    d_out = torch.full(want.shape, float(SENTINEL), dtype=torch.float32, device="cuda")
    bf.incoherent(d_in, n_units, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want), (shape, np.argwhere(got != want)[:4], got.reshape(-1)[:4], want.reshape(-1)[:4])
    for b in (0, 5, n_beams - 1):                                          # the in-stream column: offset 5 is no multiple of 4
        d_det = torch.full(want.shape + (n_beams,), float(SENTINEL), dtype=torch.float32, device="cuda")
        bf.incoherent(d_in, n_units, d_det.data_ptr() + 4 * b, stride=n_beams)
        torch.cuda.synchronize()
        det = d_det.cpu().numpy()
        assert np.array_equal(det[..., b], want), (shape, b)
        assert np.all(np.delete(det, b, axis=-1) == SENTINEL), (shape, b)
    bf.close()
    return want.size


def test_every_byte_code_and_span_shape_to_the_bit(torch, bfmod):
    """bf_incoherent_device, compact (stride 1) and as a column of a sentinel-filled detected array (stride n_beams, at beam 0, 5
    and the last), on the issue's seven span shapes and on the eight that reach the remaining lane / load-width classes and both
    sides of every class threshold; random bytes with all 256 codes planted from the first span on.  Two units, three channels, two
    outputs each -- spans below 128 bytes with 32 units (the 4-byte span with three outputs each), so that the input holds 256 bytes
    at all and the one-lane class fills more than one workgroup.  Last: more spans than a launch has lane groups (8 workgroups per
    CU x 4 groups of 64 lanes), so that the groups stride on to a second span."""
    rng = np.random.default_rng(20261018)
    t0, n = time.perf_counter(), 0
    for shape in ISSUE_SHAPES + EXTRA_SHAPES:
        small = shape[0] * shape[1] * shape[2] < 128
        n += _check_shape(torch, bfmod, rng, shape, n_units=32 if small else 2, n_out=3 if shape == (4, 1, 1) else 2)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_units = (n_cus * 8 * 4) // 6 + 3                                     # x 3 channels x 2 outputs: a few spans past one per group
    n += _check_shape(torch, bfmod, rng, (516, 1, 5), n_units=n_units)
    print("incoherent_kernel: %d shapes, %d outputs compared, %.1f s" % (len(ISSUE_SHAPES + EXTRA_SHAPES) + 1, n, time.perf_counter() - t0))


def test_the_exactness_bound(torch, bfmod):
    """2048 antennas x 2 polarisations x n_avg 32, one channel, one output: 128 * n_ant * n_ipo = 2^24 exactly, the largest sum the
    feature is defined for (bf_create accepts the geometry).  Every byte 0x88 (re = im = -8) gives 16777216.0; one byte zeroed
    16777088.0 -- a sum whose x256 partials pass 2^31 if they are not shifted out before the lanes are added.  n_avg 33: both
    exports answer BF_ERR_INVALID."""
    cfg = _cfg(bfmod, 2048, 2, 32, n_beams=4, n_freq=1, n_out=1, n_gemms_per_block=1, n_blocks_on_gpu=1, n_streams=1)
    assert 128 * cfg.n_ant * cfg.n_pol * cfg.n_avg == 2 ** 24
    packed = np.full((3, 1, 64, 2048), 0x88, np.uint8)
    packed[1, 0, 17, 1033] = 0
    packed[2, 0, 63, 2047] = 0x08                                          # (im alone: 64 less)
    bf = bfmod.Beamformer(cfg)
    d_out = torch.zeros(3, dtype=torch.float32, device="cuda")
    bf.incoherent(torch.from_numpy(packed).cuda(), 3, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    print("at the bound:", got.tolist())
    assert got.tolist() == [16777216.0, 16777088.0, 16777152.0]
    assert np.array_equal(got, ib_oracle.incoherent(packed, 1, 64).reshape(-1))
    bf.set_incoherent_beam(3)                                              # inside the bound: accepted
    bf.set_incoherent_beam(-1)
    for bad in (4, -2):
        with pytest.raises(bfmod.DsabfError) as e:
            bf.set_incoherent_beam(bad)
        assert e.value.code == BF_ERR_INVALID
    bf.close()
    over = bfmod.Beamformer(_cfg(bfmod, 2048, 2, 33, n_beams=4, n_freq=1, n_out=1, n_gemms_per_block=1, n_blocks_on_gpu=1, n_streams=1))
    d_in = torch.zeros(66 * 2048, dtype=torch.uint8, device="cuda")
    with pytest.raises(bfmod.DsabfError, match="2\\^24") as e:
        over.incoherent(d_in, 1, d_out)
    assert e.value.code == BF_ERR_INVALID
    with pytest.raises(bfmod.DsabfError, match="2\\^24") as e:
        over.set_incoherent_beam(0)
    assert e.value.code == BF_ERR_INVALID
    over.set_incoherent_beam(-1)                                           # switching it off is always possible
    over.close()


# ---- the column in the stream ---------------------------------------------------------------------------------------------------
STREAM_GEOMS = [dict(n_ant=64, n_pol=2, n_avg=16, n_beams=32), dict(n_ant=260, n_pol=2, n_avg=1, n_beams=8)]
PATHS = ("device", "block", "block_to", "units", "units_literal")


class _Stream:
    """A handle with weights, N_SLOTS blocks of random bytes in its ring (and the first one as a device array), pinned host buffers."""

    def __init__(self, torch, bfmod, geom, seed):
        self.torch = torch
        self.cfg = cfg = _cfg(bfmod, **geom)
        rng = np.random.default_rng(seed)
        self.n_u, self.n_slots = cfg.n_gemms_per_block, cfg.n_blocks_on_gpu
        self.blocks = np.stack([_random_packed(rng, cfg, self.n_u)[0] for _ in range(self.n_slots)])
        self.n_ipo = cfg.n_pol * cfg.n_avg
        self.shape = (self.n_u, cfg.n_out_per_gemm, cfg.n_freq, cfg.n_beams)
        self.want = np.stack([ib_oracle.incoherent(b, cfg.n_out_per_gemm, self.n_ipo) for b in self.blocks])   # [slot][unit][o][f]
        self.bf = bf = bfmod.Beamformer(cfg)
        bf.set_weights(rng.integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8))
        self.pin_in = torch.from_numpy(self.blocks).pin_memory()
        for slot in range(self.n_slots):
            bf.submit_block(slot, self.pin_in[slot], self.blocks[slot].nbytes)
        bf.sync(-1)
        self.d_packed = torch.from_numpy(self.blocks[0]).cuda()
        self.per = bf.floats_per_detect

    def host(self):
        return self.torch.full(self.shape, float(SENTINEL), dtype=self.torch.float32).pin_memory()

    def run(self, path, slot=0):
        """One block through `path`.  Returns (what the device holds or None, the host copies), both [unit][o][f][b]."""
        torch, bf, n_u, per = self.torch, self.bf, self.n_u, self.per
        host, dev = self.host(), None
        if path == "device":
            assert slot == 0
            d_out = torch.full(self.shape, float(SENTINEL), dtype=torch.float32, device="cuda")
            bf.beamform(self.d_packed, n_u, d_out)
            torch.cuda.synchronize()
            return d_out.cpu().numpy(), None
        if path == "block":
            bf.enqueue_block(1, slot, 0, n_u, [host[u] for u in range(n_u)])
            back = self.host()
            bf.enqueue_d2h(1, bf.block_output_device(1), back, n_u * per)
            bf.sync(1)
            dev = back.numpy().copy()
        elif path == "block_to":
            d_dst = torch.full(self.shape, float(SENTINEL), dtype=torch.float32, device="cuda")
            bf.enqueue_block_to(2, slot, 0, n_u, d_dst, [host[u] for u in range(n_u)])
            bf.sync(2)
            dev = d_dst.cpu().numpy()
        else:
            bf.set_switch("coalesce", 0 if path == "units_literal" else 1)
            for u in range(n_u):
                bf.enqueue_gemm_unit(u % self.cfg.n_streams, slot, u, host[u])
            bf.sync(-1)
            bf.set_switch("coalesce", 1)
        return dev, host.numpy().copy()

    def check_on(self, got, off, b, slot, where):
        assert np.array_equal(got[..., b], self.want[slot]), where
        assert np.array_equal(np.delete(got, b, axis=-1), np.delete(off, b, axis=-1)), where
        assert not np.array_equal(got[..., b], off[..., b]), where


def test_the_column_on_all_launch_paths(torch, bfmod):
    """bf_set_incoherent_beam(b), b = 0, 5 and the last beam, on bf_beamform_device, bf_enqueue_block, bf_enqueue_block_to and
    bf_enqueue_gemm_unit (coalesced, and with the "coalesce" switch off): column b equals the oracle, every other column the same
    call with the column off, and the host copies carry what the device holds.  After -1 the output is the off run's everywhere.
    Units queued when the setting changes keep the setting they were enqueued under."""
    t0 = time.perf_counter()
    for gi, geom in enumerate(STREAM_GEOMS):
        s = _Stream(torch, bfmod, geom, 100 + gi)
        bf, n_beams = s.bf, geom["n_beams"]
        off = {}
        for path in PATHS:
            dev, host = s.run(path)
            off[path] = host if dev is None else dev
            if dev is not None and host is not None:
                assert np.array_equal(dev, host), path
        for path in PATHS[1:]:
            assert np.array_equal(off[path], off["device"]), path
        for b in (0, 5, n_beams - 1):
            bf.set_incoherent_beam(b)
            for path in PATHS:
                dev, host = s.run(path)
                for got in (dev, host):
                    if got is not None:
                        s.check_on(got, off["device"], b, 0, (geom, b, path))
        bf.set_incoherent_beam(-1)
        for path in PATHS:
            dev, host = s.run(path)
            for got in (dev, host):
                assert got is None or np.array_equal(got, off["device"]), (geom, path)
        # ---- units still only queued keep the old setting: off -> 5 -> off with two units queued at either change, on ring slot 1
        off1 = s.run("block_to", slot=1)[0]
        host, half = s.host(), s.n_u // 2
        for first, setting in ((0, 5), (half, -1)):
            for u in range(first, first + half):
                bf.enqueue_gemm_unit(u % s.cfg.n_streams, 1, u, host[u])
            assert bf.counter("queued_units") == half
            before = bf.counter("fused_launches")
            bf.set_incoherent_beam(setting)                   # launches what is queued, under the setting it was enqueued with
            assert bf.counter("queued_units") == 0 and bf.counter("fused_launches") == before + 1
        bf.sync(-1)
        got = host.numpy()
        assert np.array_equal(got[:half], off1[:half]), geom                                        # enqueued while off
        assert np.array_equal(got[half:, ..., 5], s.want[1][half:]), geom                           # enqueued while on
        assert np.array_equal(np.delete(got[half:], 5, axis=-1), np.delete(off1[half:], 5, axis=-1)), geom
        bf.close()
    print("the column on %d paths x %d geometries: %.1f s" % (len(PATHS), len(STREAM_GEOMS), time.perf_counter() - t0))


def test_the_dm0_row_carries_the_ascending_f_sum_of_the_column(torch, bfmod):
    """With the column on, entry b of every DM-0 row -- bf_enqueue_dedisperse behind a coalesced or a literal gemm-unit, and
    bf_enqueue_block_dedisperse behind a block launch -- is the ascending-f float32 sum of the oracle's values of output 0; the
    other entries are those of the same call with the column off."""
    b = 5
    for gi, geom in enumerate(STREAM_GEOMS):
        s = _Stream(torch, bfmod, geom, 200 + gi)
        bf, n_u, n_beams = s.bf, s.n_u, geom["n_beams"]
        want_b = ib_oracle.dm0_row(s.want[0][:, 0, :])                                               # [unit]
        assert want_b.dtype == np.float32 and np.all(want_b > 0)
        rows = {}
        for setting in (-1, b):
            bf.set_incoherent_beam(setting)
            for mode in ("units", "units_literal", "block"):
                r = torch.full((n_u, n_beams), float(SENTINEL), dtype=torch.float32).pin_memory()
                if mode == "block":
                    bf.enqueue_block(1, 0, 0, n_u, None)
                    bf.enqueue_block_dedisperse(1, 0, n_u, r)
                else:
                    bf.set_switch("coalesce", 0 if mode == "units_literal" else 1)
                    for u in range(n_u):
                        bf.enqueue_gemm_unit(u % s.cfg.n_streams, 0, u, None)
                        bf.enqueue_dedisperse(u % s.cfg.n_streams, r[u])
                bf.sync(-1)
                bf.set_switch("coalesce", 1)
                rows[(setting, mode)] = r.numpy().copy()
        for mode in ("units", "units_literal", "block"):
            on, off = rows[(b, mode)], rows[(-1, mode)]
            assert np.array_equal(off, rows[(-1, "block")]), (geom, mode)
            assert np.array_equal(on[:, b], want_b), (geom, mode, on[:, b], want_b)
            assert np.array_equal(np.delete(on, b, axis=1), np.delete(off, b, axis=1)), (geom, mode)
        bf.close()


def _pulse_delays(n_dm, n_f, d_max):
    """The fine, monotone ladder of tests/test_gpu_round5.py: delay[dm][f] grows with the trial and falls with f; trial 0 is DM 0."""
    d = (np.arange(n_dm)[:, None] * np.linspace(d_max / max(n_dm - 1, 1), 0.0, n_f)[None, :]).astype(np.int32)
    return np.ascontiguousarray(d)


def test_behind_the_dm_stage_and_the_search_a_burst_on_every_antenna_peaks_at_dm_0(torch, bfmod, orc):
    """The zero-copy feed of run_observation -- bf_dm_stream_reserve, bf_enqueue_block_to, bf_dm_stream_push -- with a search stage
    attached, four blocks of 8 gemm-units x 3 outputs (96 rows), four trials from DM 0 up, widths 1, 2, 4.  Every chunk is bit-equal
    to orc.dedisperse_dm of the numpy series: the column-off detected stream (the same launches with the column off) with column b
    replaced by the oracle's incoherent beam.  The search records are sps_oracle's on those chunks.  Four consecutive output rows
    carry 0x77 on every antenna and channel: beam b's best candidate is trial 0, width 4, starting on the first of them."""
    from dsabeamformer_amd import api

    b, n_dm, n_widths, thr, min_samples = 5, 4, 3, 5.0, 16
    cfg = _cfg(bfmod, 64, 2, 4, n_beams=8, n_freq=8, n_out=3, n_gemms_per_block=8, n_blocks_on_gpu=4)
    n_u, n_out, n_f, n_b, n_ipo = cfg.n_gemms_per_block, cfg.n_out_per_gemm, cfg.n_freq, cfg.n_beams, cfg.n_pol * cfg.n_avg
    rows_per_block, n_blocks = n_u * n_out, cfg.n_blocks_on_gpu
    T, t_burst = rows_per_block * n_blocks, 46                               # rows 46 .. 49 straddle blocks 1 | 2 (row 48)
    rng = np.random.default_rng(5)
    stream = rng.integers(0, 256, size=(n_blocks, n_u, n_f, n_out, n_ipo, cfg.n_ant), dtype=np.uint8)
    for r in range(t_burst, t_burst + 4):
        stream[r // rows_per_block, (r % rows_per_block) // n_out, :, r % n_out] = 0x77
    blocks = stream.reshape(n_blocks, n_u, n_f, n_out * n_ipo, cfg.n_ant)
    ib = np.concatenate([ib_oracle.incoherent(blk, n_out, n_ipo).reshape(rows_per_block, n_f) for blk in blocks])   # [T][f]
    delays = _pulse_delays(n_dm, n_f, 6)
    D = int(delays.max())
    assert np.all(delays[0] == 0) and D == 6
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(rng.integers(-127, 128, size=(n_f, cfg.n_ant, n_b, 2), dtype=np.int8))
    pin_in = torch.from_numpy(blocks).pin_memory()
    for slot in range(n_blocks):
        bf.submit_block(slot, pin_in[slot], blocks[slot].nbytes)
    bf.sync(-1)
    # the column-off detected stream, from the same launches
    d_off = torch.zeros((T, n_f, n_b), dtype=torch.float32, device="cuda")
    for blk in range(n_blocks):
        bf.enqueue_block_to(0, blk, 0, n_u, d_off.data_ptr() + 4 * blk * rows_per_block * n_f * n_b)
    bf.sync(0)
    series = d_off.cpu().numpy()
    assert not np.array_equal(series[:, :, b], ib)
    series[:, :, b] = ib
    want = orc.dedisperse_dm(series, delays, T - D)                          # [n_dm][T - D][n_b]
    search = sps_oracle.Search(want, n_widths, threshold=thr, min_samples=min_samples)
    # ---- the device, column on
    bf.set_incoherent_beam(b)
    dm = api.DmStream(bf, delays, n_f, rows_per_block)
    sps = api.SinglePulseSearch(bf, n_dm, n_widths, rows_per_block, threshold=thr, min_samples=min_samples)
    dm.attach_search(sps)
    host = torch.full((n_dm * rows_per_block * n_b,), float("nan"), dtype=torch.float32).pin_memory()
    parts, found, first_want = [], [], 0
    for blk in range(n_blocks):
        q = blk % 2
        st = bf.queue_stream(q)
        dst = dm.reserve(rows_per_block, st)
        bf.enqueue_block_to(q, blk, 0, n_u, dst)
        first_t, n_t = dm.push(dst, rows_per_block, host, st)
        assert (first_t, n_t) == (first_want, rows_per_block - (D if blk == 0 else 0))
        first_want += n_t
        bf.sync(q)
        parts.append(host[:n_dm * n_t * n_b].numpy().reshape(n_dm, n_t, n_b).copy())
        assert np.array_equal(parts[-1], want[:, first_t:first_t + n_t]), blk
        w = search.push(n_t)
        cands = sps.collect()
        rec = sps.last_records()
        assert np.array_equal(rec["value"], w["value"]) and np.array_equal(rec["t_end"], w["t_end"]), blk
        sps_oracle.assert_candidates_equal(cands, w["cands"], rtol=1e-9)
        found.append(cands)
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    found = np.concatenate(found)
    mine = found[found["beam"] == b]
    assert len(mine) > 0
    top = mine[int(mine["snr"].argmax())]
    print("beam %d's best candidate:" % b, top)
    assert (int(top["t_start"]), int(top["dm"]), int(top["width"])) == (t_burst, 0, 4) and np.count_nonzero(mine["snr"] == top["snr"]) == 1
    sps.close()
    dm.close()
    bf.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------------
N_ANALYSED = 2      # `-j 27`: the junk source counts the 25 burn-in reads (BURNIN), so 2 blocks are analysed (-j 2 alone: none)


def _junk_ring(host, cfg):
    n_time = cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg
    return host.junk_bytes(cfg.n_ant * cfg.n_freq * n_time * cfg.n_gemms_per_block, 4, 0xD5A, cfg).reshape(
        4, cfg.n_gemms_per_block, cfg.n_freq, n_time, cfg.n_ant)


def _column_of_the_run(host, cfg):
    """The oracle's incoherent beam of the blocks a `beam -j 27` run analyses: [gemm-unit][o][f] (block i is junk block (25 + i) % 4)."""
    ring = _junk_ring(host, cfg)
    return np.concatenate([ib_oracle.incoherent(ring[(25 + i) % 4], cfg.n_out_per_gemm, cfg.n_pol * cfg.n_avg) for i in range(N_ANALYSED)])


def test_beam_cli_i_replaces_one_column_of_the_detected_file(bfmod, tmp_path):
    """`beam -j 27 -a 1 -i 5 -w det.bin` against the same command without -i (observation mode runs the production geometry; the
    issue's `-j 2` would analyse nothing: the junk source counts the 25 burn-in reads): column 5 of every gemm-unit equals the
    oracle over the regenerated junk bytes (host.junk_bytes: bfh_junk_fill), every other column is byte-equal between the files."""
    from dsabeamformer_amd import build, host

    files = {}
    for name, extra in (("on", ["-i", "5"]), ("off", [])):
        path = tmp_path / (name + ".bin")
        r = subprocess.run([build.BEAM, "-j", str(25 + N_ANALYSED), "-a", "1"] + extra + ["-w", str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("Incoherent beam: in beam column 5" in r.stdout) == (name == "on")
        files[name] = host.read_detected_file(str(path))[1]
    cfg = bfmod.production_config()
    on, off = files["on"], files["off"]
    assert on.shape == off.shape == (N_ANALYSED * cfg.n_gemms_per_block, cfg.n_out_per_gemm, cfg.n_freq, cfg.n_beams)
    assert np.array_equal(on[..., 5], _column_of_the_run(host, cfg))
    assert np.array_equal(np.delete(on, 5, axis=-1).view(np.uint32), np.delete(off, 5, axis=-1).view(np.uint32))
    assert not np.array_equal(on[..., 5], off[..., 5])


def test_two_loopback_ranks_fill_their_slices_of_the_column(bfmod, tmp_path):
    """`beam -j 27 -R 2 -r k -i 5` as two shard processes (the stand-in RCCL library and launch pattern of
    tests/test_gpu_round5.py): on the gather root, column 5 over the whole band is the oracle's over both shards' inputs -- every
    shard reads the junk bytes with ITS geometry (128 channels) and fills its own channels of the column."""
    from test_gpu_multirank import FAKE  # noqa: F401  (built by that module's fixture; build here if it has not run)

    from dsabeamformer_amd import build, host

    src = os.path.join(SUPPORT, "fake_rccl.cpp")
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(src):
        obj = os.path.join(SUPPORT, "fake_rccl.o")
        subprocess.check_call([build.HIPCC, "-O2", "-std=c++17", "-fPIC", "-c", src, "-o", obj])
        cxx = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
        subprocess.check_call([cxx if os.path.exists(cxx) else "g++", "-shared", "-fPIC", "-o", FAKE, obj, "-lpthread", "-lrt"])
    det = tmp_path / "det.bin"
    cmd = lambda rk: [build.BEAM, "-j", str(25 + N_ANALYSED), "-D", "0", "-i", "5", "-R", "2", "-r", str(rk), "-I", str(tmp_path / "id")] + (  # noqa: E731
        ["-w", str(det)] if rk == 0 else [])
    procs = [subprocess.Popen(cmd(rk), env=dict(os.environ, DSABF_RCCL_LIB=FAKE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for rk in (0, 1)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("Incoherent beam: in beam column 5" in o for o in outs)
    shard = bfmod.production_config(n_freq=128)
    col = _column_of_the_run(host, shard)                                   # [unit][o][128]: the same bytes for either shard
    got = host.read_detected_file(str(det))[1]                              # [unit][o][256][256]
    assert got.shape == (N_ANALYSED * shard.n_gemms_per_block, shard.n_out_per_gemm, 256, 256)
    assert np.array_equal(got[..., 5], np.concatenate([col, col], axis=-1))
    assert np.isfinite(got).all() and not np.array_equal(got[..., 5], got[..., 4])
