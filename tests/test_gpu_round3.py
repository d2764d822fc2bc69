"""GPU tests (-m gpu) of the round-3 surface: the HIP path on the integers the reference's executed notebook itself used
(the tight pin of a2 / a3 / a8), calibrated (non-conjugate-symmetric) weights through the general kernel at production
size, events on a handle's device, the block-wide DM-0 collapse.  Every call goes through the C-ABI of libdsabf.so."""
import os
import sys

import numpy as np
import pytest

import bench
from conftest import NOTEBOOK_INTEGER_TOL, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))

import dm_paths  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _table_on_gpu(torch, bf, g, col, batch=128):
    """DEBUG geometry: beamform all sources (16 identical time columns each) and collapse frequency on the device."""
    n_src = col.shape[0]
    s = torch.cuda.current_stream().cuda_stream
    ded = torch.empty((n_src, g.n_beams), dtype=torch.float32, device="cuda")
    first = None
    for u0 in range(0, n_src, batch):
        packed = np.ascontiguousarray(np.broadcast_to(col[u0:u0 + batch, :, None, :], (batch, g.n_freq, g.n_time, g.n_ant)))
        d_in = torch.from_numpy(packed).cuda()
        d_out = torch.empty(batch * g.out_per_gemm, dtype=torch.float32, device="cuda")
        bf.beamform(d_in, batch, d_out, s)
        per_unit = d_out.view(batch, g.out_per_gemm)
        for u in range(batch):
            bf.dedisperse(per_unit[u], ded[u0 + u], s)          # output 0 of the gemm-unit, as the DEBUG flow does
        if first is None:
            torch.cuda.synchronize()
            first = d_out.cpu().numpy().reshape(batch, g.n_out_per_gemm, g.n_freq, g.n_beams)
    torch.cuda.synchronize()
    return ded.cpu().numpy(), first


@pytest.mark.parametrize("paired", [True, False])
def test_hip_path_on_the_notebooks_own_integers_agrees_to_fp32_rounding(torch, bfmod, orc, notebook_integers, paired, monkeypatch):
    """VERDICT r02 item 1 on the GPU.  expand -> int8 MFMA -> detect -> DM-0 collapse of libdsabf.so, fed with the A * 127 and
    the quantised signals the executed notebook used, against the notebook's double `out` (2D Beamformer.ipynb cell 8):
    every one of the 1024 x 256 entries within fp32 rounding (<= 261 * 2^-24 = 1.56e-5; measured 1.5e-6), and bit-identical
    to the oracle on the same integers.  Both kernels: the notebook's all-double weight set is conjugate-symmetric."""
    w, col, nb_out, _ = notebook_integers
    g = orc.DEBUG_GEOM
    if not paired:
        monkeypatch.setenv("DSABF_PAIRED", "0")
    bf = bfmod.Beamformer(bfmod.debug_config())
    bf.set_weights(w)
    assert ("PAIRED" in bf.kernel_info(128)["kernel"]) == paired
    table, first = _table_on_gpu(torch, bf, g, col)
    bf.close()
    ref = nb_out.T
    worst = float(np.abs(table.astype(np.float64) / ref - 1).max())
    assert worst <= NOTEBOOK_INTEGER_TOL, worst
    assert worst <= 4e-6, worst
    assert np.array_equal(table.argmax(1), nb_out.argmax(0))
    # the same bits as the oracle on the same integers (first 128 sources in full, then the whole collapsed table)
    packed = np.ascontiguousarray(np.broadcast_to(col[:128, :, None, :], (128, g.n_freq, g.n_time, g.n_ant)))
    want = orc.beamform(g, w, packed)
    assert np.array_equal(first, want)
    full = np.ascontiguousarray(np.broadcast_to(col[:, :, None, :], (1024, g.n_freq, g.n_time, g.n_ant)))
    want_all = orc.beamform(g, w, full)
    assert np.array_equal(table, np.stack([orc.dedisperse(g, want_all[u, 0]) for u in range(1024)]))


@pytest.mark.parametrize("contracted", [False, True])
def test_calibrated_weights_run_the_general_kernel_bit_exact_at_production_size(torch, bfmod, orc, contracted):
    """What a real array uploads: the steering fan times per-(frequency, antenna) complex gains (bench.calibrated_weights).
    The conjugate symmetry is gone, so bf_set_weights must select the GENERAL kernel -- the production number of the bench
    line -- and its output must be the oracle's, at BASELINE configs[2] size (64 ant x 256 freq x 256 beams, N_TIME 512),
    on sampled (unit, frequency) pairs bit for bit, in both detect readings."""
    from dsabeamformer_amd import host
    from dsabeamformer_amd._lib import BF_DETECT_CONTRACTED

    cfg = bfmod.production_config(n_avg=16, n_out_per_gemm=16, detect_mode=BF_DETECT_CONTRACTED if contracted else 0)
    fan = host.make_weights_default(n_beams=cfg.n_beams, n_ant=cfg.n_ant, n_freq_total=256, gpu=0)
    w = bench.calibrated_weights(fan, seed=7)
    assert (w[:, :, ::-1, 0] != w[..., 0]).any()                       # no longer W[B-1-b] = conj(W[b])
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(fan)
    assert "PAIRED" in bf.kernel_info(8)["kernel"]
    bf.set_weights(w)
    assert "PAIRED" not in bf.kernel_info(8)["kernel"]
    n_units, n_time = 8, 16 * 32
    rng = np.random.default_rng(77)
    packed = rng.integers(0, 256, size=(n_units, cfg.n_freq, n_time, cfg.n_ant), dtype=np.uint8)
    d_in = torch.from_numpy(packed).cuda()
    d_out = torch.full((n_units * 16 * cfg.n_freq * cfg.n_beams,), float("nan"), dtype=torch.float32, device="cuda")
    bf.beamform(d_in, n_units, d_out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().reshape(n_units, 16, cfg.n_freq, cfg.n_beams)
    bf.close()
    assert np.isfinite(got).all()
    g1 = orc.Geom(n_beams=cfg.n_beams, n_ant=cfg.n_ant, n_freq=1, n_avg=16, n_out_per_gemm=16)
    with orc.detect_contract(orc.CONTRACT_NVCC if contracted else orc.CONTRACT_NONE):
        for f in (0, 1, 37, 128, 255):
            want = orc.beamform(g1, np.ascontiguousarray(w[f:f + 1]), np.ascontiguousarray(packed[:, f:f + 1]))
            assert np.array_equal(got[:, :, f], want[:, :, 0]), f


def test_events_are_created_on_the_handles_device(torch, bfmod):
    """bf_event_create used the caller's current device.  bf_event_create_on(h, ...) creates the event
    under the handle's device; on a one-GPU box this exercises the entry point and the observation loop that now uses it
    (a second device, when present, is driven while device 0 stays current)."""
    from dsabeamformer_amd import api

    dev = torch.cuda.device_count() - 1
    cfg = bfmod.debug_config(n_beams=64, n_freq=8)
    torch.cuda.set_device(0)
    bf = bfmod.Beamformer(cfg, device=dev)
    ev = api.event_create(bf)
    w = np.random.default_rng(1).integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8)
    bf.set_weights(w)
    host_in = np.random.default_rng(2).integers(0, 256, size=bf.bytes_per_block, dtype=np.uint8)
    pinned = torch.from_numpy(host_in).pin_memory()
    bf.submit_block(0, pinned, bf.bytes_per_block, ev)       # records `ev` on the handle's transfer queue
    while api.event_query(ev) != 0:
        pass
    bf.timer_start()
    assert bf.timer_stop() >= 0.0
    api.event_destroy(ev)
    assert torch.cuda.current_device() == 0
    bf.close()


def test_block_dedisperse_equals_per_unit_dedisperse(torch, bfmod, orc):
    """bf_enqueue_block_dedisperse: the DM-0 collapse (a8) of every gemm-unit of a block in one launch -- the bits of
    bf_enqueue_dedisperse unit by unit, and the oracle's."""
    g = orc.Geom(n_beams=96, n_ant=64, n_freq=24, n_avg=1, n_out_per_gemm=8)
    cfg = bfmod.debug_config(n_beams=g.n_beams, n_freq=g.n_freq)
    cfg.n_gemms_per_block, cfg.n_blocks_on_gpu, cfg.n_streams = 8, 2, 4
    rng = np.random.default_rng(31)
    w = rng.integers(-127, 128, size=(g.n_freq, g.n_ant, g.n_beams, 2), dtype=np.int8)
    block = rng.integers(0, 256, size=(cfg.n_gemms_per_block, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(w)
    pinned = torch.from_numpy(block).pin_memory()
    bf.submit_block(1, pinned, block.nbytes)
    bf.sync(-1)
    rows = torch.zeros((cfg.n_gemms_per_block, g.n_beams), dtype=torch.float32).pin_memory()
    outs = torch.zeros((cfg.n_gemms_per_block, g.out_per_gemm), dtype=torch.float32).pin_memory()
    bf.enqueue_block(2, 1, 0, cfg.n_gemms_per_block, [outs[u] for u in range(cfg.n_gemms_per_block)])   # one coalesced copy
    bf.enqueue_block_dedisperse(2, 0, 5, rows)             # units 0..4
    bf.enqueue_block_dedisperse(2, 5, 3, rows[5:])         # units 5..7
    # the first block launch allocates EVERY queue's buffer (round 4), but a queue that has launched nothing still has nothing
    # to collapse: refused, as before
    with pytest.raises(bfmod.DsabfError, match="has not run on queue 3"):
        bf.enqueue_block_dedisperse(3, 0, 1, rows)
    bf.sync(-1)
    want = orc.beamform(g, w, block)
    assert np.array_equal(outs.numpy().reshape(want.shape), want)
    assert np.array_equal(rows.numpy(), np.stack([orc.dedisperse(g, want[u, 0]) for u in range(cfg.n_gemms_per_block)]))
    # per-unit path for comparison
    row1 = torch.zeros(g.n_beams, dtype=torch.float32).pin_memory()
    for u in (0, 7):
        bf.enqueue_gemm_unit(0, 1, u, None)
        bf.enqueue_dedisperse(0, row1)
        bf.sync(-1)
        assert np.array_equal(row1.numpy(), rows.numpy()[u])
    bf.close()


def test_debug_flow_block_and_reference_launch_patterns_write_the_same_table(bfmod, tmp_path):
    """run_debug_observation: one launch + one copy + one DM-0 launch per block (default) vs the reference's per gemm-unit
    pattern (src/beamformer.cu:454-519): the same [1024][256] table, the golden one, bit for bit."""
    from conftest import CFG, GOLDEN
    from dsabeamformer_amd import host

    kw = dict(gpu=0, positions=os.path.join(CFG, "linear_positions.txt"), directions=os.path.join(CFG, "linear_directions.txt"),
              sources=os.path.join(CFG, "linear_source_directions_1024.txt"))
    blk, ms_blk = host.run_debug_observation(bfmod.debug_config(), output=str(tmp_path / "a.py"), **kw)
    ref, ms_ref = host.run_debug_observation(bfmod.debug_config(), output=str(tmp_path / "b.py"), per_unit_launches=True, **kw)
    golden = np.load(os.path.join(GOLDEN, "linear_debug.npz"))["dedispersed"]
    assert np.array_equal(blk, golden) and np.array_equal(ref, golden)
    assert open(tmp_path / "a.py").read() == open(tmp_path / "b.py").read()
    print("DEBUG flow: block launches %.1f ms, reference pattern %.1f ms" % (ms_blk, ms_ref))


def test_pulse_dispersed_with_the_notebooks_own_delays_is_recovered(torch, bfmod, orc):
    """8f-4 end to end on what the reference's notebook produced: a pulse drawn with the 2048 per-channel delays that
    sandbox/Dispersion Theory.ipynb cell 5 used for DM 2000 (tests/golden/dispersion_notebook.npz, captured by executing the
    cell) into a [1000 sample][2048 channel] series, dedispersed over the last trials of the notebook's own ladder (cell 2)
    plus the cell's DM-2000 delays themselves: the DM-2000 trial collects all 2048 channels at the pulse's start sample,
    every ladder trial a step away collects fewer; the device result is the oracle's, bit for bit."""
    from conftest import GOLDEN
    from dsabeamformer_amd import host

    nb = np.load(os.path.join(GOLDEN, "dispersion_notebook.npz"))
    nb_delays = nb["delays_dm2000"].astype(np.int32)                      # channel i at 1.28 + 0.25/2048 i GHz
    n_t, n_f, n_b, start = 1000, 2048, 16, 100                             # the cell's max_time, Nchan, start_index
    freq = np.array([1.28 + (1.53 - 1.28) / 2048 * i for i in range(n_f)], np.float32)
    ladder = nb["dms"][-6:]                                                # ... 1990.6, 1993.1, 1995.6, 1998.0, 2000.5
    delays = np.concatenate([host.dm_delays(ladder, freq, 1.53, float(nb["tsamp_ms"][0])), nb_delays[None]]).astype(np.int32)
    series = np.zeros((n_t, n_f, n_b), np.float32)
    series[start + nb_delays, np.arange(n_f), :] = 1.0                     # what cell 5 draws (its += 2.0 without the noise)
    cfg = bfmod.debug_config(n_beams=n_b, n_freq=n_f)
    bf = bfmod.Beamformer(cfg)
    n_t_out = n_t - int(delays.max())
    d_out = torch.full((len(delays), n_t_out, n_b), float("nan"), dtype=torch.float32, device="cuda")
    bf.dedisperse_dm(torch.from_numpy(series).cuda(), n_t, torch.from_numpy(delays).cuda(), len(delays), n_t_out, d_out,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    bf.close()
    assert np.array_equal(got, orc.dedisperse_dm(series, delays, n_t_out))
    assert got[-1, start, 0] == n_f and got[-1].max() == n_f               # every channel lands on the start sample
    peaks = got[:-1].max(axis=(1, 2))
    assert (peaks < n_f).all() and peaks.argmax() >= len(ladder) - 2        # the closest ladder trials come closest
    assert np.array_equal(got[:-1].argmax(axis=1)[:, 0] >= start - 2, np.ones(len(ladder), bool))


@pytest.mark.parametrize("case", ["fine_64", "ragged_beams_trials", "mixed_groups", "negative_and_tail", "tiny"])
def test_shared_window_dm_kernel_bit_exact(torch, bfmod, orc, case, monkeypatch):
    """The round-3 DM-trial kernel (csrc/bf_dm_wide.hip: 32 trials x 16 times x 128 beams per workgroup, windows staged by
    LDS-DMA and shared by all trials) against the oracle and against the per-thread-window kernel alone (bf_set_switch "dm_wide" 0):
    the same bits.  Cases: a fine ladder (every group fits); beams that do not fill the last 128-beam tile with a trial count
    that does not fill the last pair / group; groups that fit next to groups that do not (the two kernels share one launch);
    delays that start negative (rows before the series read +0) with outputs running past its end; a tiny problem."""
    rng = np.random.default_rng(hash(case) % 1000)
    if case == "fine_64":
        n_t, n_f, n_b, n_dm = 300, 64, 256, 64
        delays = np.sort(rng.integers(0, 40, size=(n_dm, n_f)), axis=0)
        delays = np.sort(delays, axis=1)[:, ::-1].copy()
    elif case == "ragged_beams_trials":
        n_t, n_f, n_b, n_dm = 200, 48, 132, 37
        delays = (np.arange(n_dm)[:, None] * np.linspace(1.5, 0, n_f)[None, :]).astype(np.int64)
    elif case == "mixed_groups":
        n_t, n_f, n_b, n_dm = 400, 32, 64, 96      # group 0 fine, group 1 far too coarse, group 2 fine
        step = np.concatenate([np.full(32, 0.5), np.full(32, 9.0), np.full(32, 0.5)])
        delays = (np.cumsum(step)[:, None] * np.linspace(1.0, 0.1, n_f)[None, :]).astype(np.int64)
    elif case == "negative_and_tail":
        n_t, n_f, n_b, n_dm = 150, 40, 128, 33
        delays = (np.arange(n_dm)[:, None] * np.linspace(1.0, -0.5, n_f)[None, :]).astype(np.int64) - 7
    else:
        n_t, n_f, n_b, n_dm = 20, 4, 4, 3
        delays = np.array([[0, 0, 0, 0], [2, 1, 1, 0], [5, 3, 2, 0]])
    delays = np.ascontiguousarray(delays.astype(np.int32))
    # which kernel will run, predicted from the delays alone (tests/support/dm_paths.py) -- and it is what the cases above say
    fits = dm_paths.wide_fits(delays)
    assert fits.tolist() == {"fine_64": [True, True], "ragged_beams_trials": [True, True], "mixed_groups": [True, False, True],
                             "negative_and_tail": [True, True], "tiny": [True]}[case]
    series = (rng.random((n_t, n_f, n_b), dtype=np.float32) * 1e4).astype(np.float32)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    d_series, d_delays = torch.from_numpy(series).cuda(), torch.from_numpy(delays).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for n_t_out in sorted({max(1, n_t - int(delays.max())), n_t}):
        want = orc.dedisperse_dm(series, delays, n_t_out)
        got = {}
        for mode in ("shared", "thread"):
            bf.set_switch("dm_wide", 0 if mode == "thread" else 1)   # per handle (bf_set_switch): never the environment mid-process
            d_out = torch.full((n_dm, n_t_out, n_b), float("nan"), dtype=torch.float32, device="cuda")
            bf.dedisperse_dm(d_series, n_t, d_delays, n_dm, n_t_out, d_out, s)
            assert bf.counter("dm_wide_mask") == (dm_paths.mask_of(fits) if mode == "shared" else 0), (case, n_t_out, mode)
            assert bf.counter("dm_wide_groups") == (int(fits.sum()) if mode == "shared" else 0)
            torch.cuda.synchronize()
            got[mode] = d_out.cpu().numpy()
        bf.set_switch("dm_wide", 1)
        assert np.array_equal(got["shared"], want), (case, n_t_out)
        assert np.array_equal(got["thread"], want), (case, n_t_out)
    bf.close()


def _conj_symmetric(w):
    out = w.copy()
    b = w.shape[2]
    out[:, :, b // 2:, 0] = w[:, :, :b // 2, 0][:, :, ::-1]
    out[:, :, b // 2:, 1] = -w[:, :, :b // 2, 1][:, :, ::-1]
    return out


@pytest.mark.parametrize("n_ant,n_beams,n_avg", [(100, 512, 8), (100, 512, 16), (100, 480, 32), (100, 512, 32), (128, 512, 16),
                                                 (128, 1024, 8), (128, 512, 32), (112, 512, 8), (112, 1024, 16), (108, 512, 16),
                                                 (68, 288, 8), (124, 992, 32)])
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_wide_launches_of_the_two_kstep_classes_bit_exact(torch, bfmod, orc, monkeypatch, n_ant, n_beams, n_avg, paired, mode):
    """The two-k-step classes at n_ipo >= 16 (bf_kernels.hip): the conjugate-pair kernel runs 8 output slots per wave where the
    beams come in whole groups of 512 and the instantiation fits its registers (fused_col_tiles: not the run-time dword class, not
    100 antennas at n_ipo 64); otherwise, with an even number of 256-beam groups, 8-wave workgroups (fused_wg_waves).  Both
    compile-time classes and both run-time ones, full and ragged last groups (480, 288, 992 beams), canonical / contracted /
    fast detect, general and conjugate-pair kernel: bit-exact against the oracle (fast: within its tolerance), and bit-identical
    to the same geometry forced onto the plain 4-wave, 4-slot launch."""
    g = orc.Geom(n_beams=n_beams, n_ant=n_ant, n_freq=3, n_avg=n_avg, n_out_per_gemm=6)
    n_units = max(2, -(-500 // g.n_time))
    rng = np.random.default_rng(n_ant * 7 + n_beams + n_avg + 17 * paired)
    w = rng.integers(-127, 128, size=(g.n_freq, g.n_ant, g.n_beams, 2), dtype=np.int8)
    w[0, :, 5] = 127
    if paired:
        w = _conj_symmetric(w)
    packed = rng.integers(0, 256, size=(n_units, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    packed[0, 0, :4] = 0x88
    cfg = bfmod.production_config(n_beams=g.n_beams, n_ant=g.n_ant, n_freq=g.n_freq, n_avg=g.n_avg, n_out_per_gemm=g.n_out_per_gemm,
                                  detect_mode=mode)
    with orc.detect_contract(orc.CONTRACT_NVCC if mode == 2 else orc.CONTRACT_NONE):
        want = orc.beamform(g, w, packed)
    s = torch.cuda.current_stream().cuda_stream
    d_in = torch.from_numpy(packed).cuda()
    got = {}
    for forced in (None, "4"):
        if forced:
            monkeypatch.setenv("DSABF_WG_WAVES", forced)
            monkeypatch.setenv("DSABF_COL_TILES", forced)
        bf = bfmod.Beamformer(cfg)
        bf.set_weights(w)
        info = bf.kernel_info(n_units)
        assert ("PAIRED" in info["kernel"]) == paired
        d_out = torch.full((want.size,), float("nan"), dtype=torch.float32, device="cuda")
        bf.beamform(d_in, n_units, d_out, s)
        torch.cuda.synchronize()
        got[forced] = (info, d_out.cpu().numpy().reshape(want.shape))
        bf.close()
    info, out = got[None]
    slots8 = paired and n_beams % 512 == 0 and (n_ant % 16 == 0 or (n_ant == 100 and n_avg < 32))
    assert ("SLOTS=8" in info["kernel"]) == slots8 and ("WAVES=8" in info["kernel"]) == (not slots8)
    assert info["block"] == (256 if slots8 else 512)
    assert got["4"][0]["block"] == 256 and "=8" not in got["4"][0]["kernel"]
    assert np.array_equal(out, got["4"][1])
    if mode == 1:
        rel = np.abs(out.astype(np.float64) - want) / np.maximum(want.astype(np.float64), 1e-30)
        assert rel.max() <= 4 * g.n_ipo * 2.0 ** -24
    else:
        assert np.array_equal(out, want)


def test_mfma_peak_microbenchmark_runs_and_counts_its_ops(torch, bfmod):
    """bf_mfma_peak_device (the measured peak beside the nominal one): the launch executes the ops it reports --
    n_cus x 4 workgroups x 4 waves x iters x 16 MFMAs x 32,768 int8 ops -- lasts in proportion to iters, lands between 40 % and
    100 % of the nominal 5 POP/s on random operands, and refuses short buffers."""
    bf = bfmod.Beamformer(bfmod.production_config())
    s = torch.cuda.current_stream()
    src = torch.randint(0, 256, (4 << 20,), dtype=torch.uint8, device="cuda")
    sink = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda")
    ms = {}
    for iters in (500, 2000):
        for _ in range(5):
            ops = bf.mfma_peak(src, src.numel(), sink, sink.numel(), iters, s.cuda_stream)
        assert ops == 256 * 4 * 4 * iters * 16 * 32768
        ms[iters] = bench.time_launches(torch, lambda i: bf.mfma_peak(src, src.numel(), sink, sink.numel(), iters, s.cuda_stream), 20, s)[1]
    assert 3.0 < ms[2000] / ms[500] < 4.6
    tops = 256 * 4 * 4 * 2000 * 16 * 32768 / (ms[2000] * 1e-3) / 1e12
    assert 2000 < tops <= 5000 * 1.02, tops
    assert sink.view(torch.int32)[: 1024 * 256].abs().sum().item() > 0          # the accumulators were stored
    with pytest.raises(bfmod.DsabfError):
        bf.mfma_peak(src, 1 << 20, sink, sink.numel(), 100, s.cuda_stream)
    bf.close()
