"""GPU tests (-m gpu) of the gain solver and the calibrated weights (include/dsabf.h: bf_solve_gains_device,
bf_calibrate_weights_device; docs/CALIBRATION.md).  The reference is tests/support/cal_oracle.py -- numpy float64 in the contract's one
summation order -- and every comparison of gains, info and weights is np.array_equal on the raw bits: outputs are filled with a sentinel
first (a NaN payload for the float64 gains, 0x7F bytes for info and weights) and compared whole.

Every test is ONE function that loops over its cases, as tests/test_gpu_corr.py does."""
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

pytestmark = pytest.mark.gpu

BF_ERR_INVALID = -1
NAN_BITS = 0x7FF8DEADBEEF0001        # a quiet NaN with a payload no arithmetic produces
INFO_FILL = 0x7F7F7F7F
K = 2.0 ** 20


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _cfg(bfmod, n_ant, n_pol=1, n_freq=1, n_beams=8, **over):
    kw = dict(n_ant=n_ant, n_pol=n_pol, n_avg=1, n_beams=n_beams, n_freq=n_freq, n_out_per_gemm=2, n_gemms_per_block=4, n_blocks_on_gpu=2,
              n_streams=4)
    kw.update(over)
    return bfmod.debug_config(**kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _outputs(torch, cfg, joint):
    n_po = 1 if joint else cfg.n_pol
    return (torch.full((n_po, cfg.n_freq, cfg.n_ant, 2), NAN_BITS, dtype=torch.int64, device="cuda"),
            torch.full((n_po, cfg.n_freq, 2), INFO_FILL, dtype=torch.int32, device="cuda"))


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _solve(torch, bf, vis, model=None, flags=None, joint=False, **opt):
    """One solve through the Python API: (bits of the gains as int64, info)."""
    d_g, d_i = _outputs(torch, bf.cfg, joint)
    d_vis, d_m, d_f = _dev(torch, vis), _dev(torch, model), _dev(torch, flags)
    bf.solve_gains(d_vis, d_g, d_i, model=d_m, flags=d_f, joint_pol=joint, **opt)
    torch.cuda.synchronize()
    return d_g.cpu().numpy(), d_i.cpu().numpy()


def _model(rng, n_freq, n_ant):
    ph = 2 * np.pi * rng.uniform(size=(n_freq, n_ant))
    return np.stack([np.cos(ph), np.sin(ph)], axis=-1)


def _flags(rng, vis, n_ant):
    """Antennas 0 and n - 2 flagged, and garbage wherever they take part in `vis`."""
    flags = np.zeros(n_ant, np.uint8)
    flags[[0, n_ant - 2]] = 1
    for a in (0, n_ant - 2):
        idx = [cal_oracle.bl(max(a, b), min(a, b)) for b in range(n_ant)]
        vis[:, :, idx] = rng.integers(-2 ** 40, 2 ** 40, size=vis.shape[:2] + (n_ant, 2))
    return flags


# (n_ant, n_freq, n_pol, joint_pol, flags, model, path): path "auto" is what the library picks (LDS-resident up to 64 antennas, streamed
# above), "streamed" forces the re-reading path where the resident one would run.  4 and 256 antennas -- the smallest and the largest --
# meet every option value.
COUNT_CASES = [(4, 1, 1, False, False, False, "auto"), (4, 3, 2, True, True, True, "auto"), (4, 3, 2, False, True, False, "streamed"),
               (4, 1, 2, True, False, True, "auto"), (4, 3, 1, True, False, False, "auto"),
               (20, 3, 2, False, True, True, "auto"), (20, 1, 2, True, False, False, "streamed"),
               (64, 3, 2, False, False, True, "auto"),          # exactly one term per lane: the LDS-resident path at its largest
               (64, 1, 2, True, True, False, "streamed"),       # the same antennas on the streamed path
               (68, 3, 2, True, True, True, "auto"),            # the first second term of a lane: the streamed path at its smallest
               (100, 1, 1, False, False, False, "auto"), (132, 3, 2, False, True, True, "auto"),
               (256, 1, 1, False, False, True, "auto"), (256, 3, 2, True, True, False, "auto"), (256, 1, 2, False, True, True, "auto"),
               (256, 3, 1, True, False, False, "auto")]


def test_every_antenna_count_to_the_bit(torch, bfmod):
    """Antenna counts 4, 20, 64, 68, 100, 132, 256; 1 and 3 channels; 1 and 2 polarisations; joint_pol off and on; no flags or {0, n - 2}
    flagged (the default reference then moves to antenna 1) with garbage in the flagged rows; no model or random unit phasors; both
    storage paths.  Gains and info whole, to the bit."""
    for idx, values in ((0, (4, 20, 64, 68, 100, 132, 256)), (1, (1, 3)), (2, (1, 2)), (3, (False, True)), (4, (False, True)), (5, (False, True))):
        for n_ant in (4, 256) if idx else (None,):
            have = {c[idx] for c in COUNT_CASES if n_ant is None or c[0] == n_ant}
            assert have == set(values), (idx, n_ant, have)
    assert {(c[0], c[6]) for c in COUNT_CASES} >= {(64, "auto"), (64, "streamed"), (68, "auto")}
    rng = np.random.default_rng(20261018)
    t0 = time.perf_counter()
    for case in COUNT_CASES:
        n_ant, n_freq, n_pol, joint, flagged, with_model, path = case
        cfg = _cfg(bfmod, n_ant, n_pol, n_freq)
        model = _model(rng, n_freq, n_ant) if with_model else None
        vis, _ = cal_oracle.synth_vis(rng, n_ant, n_freq, n_pol, K, model, same_gains=joint)
        flags = _flags(rng, vis, n_ant) if flagged else None
        want_g, want_i = cal_oracle.solve(vis, n_ant, model=model, flags=flags, joint_pol=joint)
        bf = bfmod.Beamformer(cfg)
        assert bf.gain_entries(joint) * 2 == want_g.size
        if path == "streamed":
            bf.set_switch("cal_resident", 0)
        got_g, got_i = _solve(torch, bf, vis, model, flags, joint)
        bf.close()
        assert np.array_equal(got_i, want_i), (case, got_i.tolist(), want_i.tolist())
        bad = np.argwhere(got_g != _bits(want_g))
        assert bad.size == 0, (case, len(bad), bad[:4], got_g[tuple(bad[0])], _bits(want_g)[tuple(bad[0])])
        assert np.all(want_i[..., 1] == 1) or n_ant == 4, (case, want_i.tolist())
        if flagged:
            assert not want_g[:, :, [0, n_ant - 2]].any()
    print("solve_kernel: %d cases, %.1f s" % (len(COUNT_CASES), time.perf_counter() - t0))


def test_known_gains_are_recovered(torch, bfmod):
    """No noise: after undoing the reference phase and sqrt(K), max |g - g_true| / max |g_true| <= 1e-5 over the unflagged antennas --
    about four times the worst relative rounding of one entry of V = rint(K ...), 0.5 sqrt(2) / 2^18 = 2.7e-6 -- and flagged gains are
    exactly 0.  The oracle meets the bar too."""
    rng = np.random.default_rng(7)
    for n_ant, flagged, with_model in ((4, False, False), (20, True, True), (64, False, True), (100, True, False), (256, False, False)):
        cfg = _cfg(bfmod, n_ant, 2, 3)
        model = _model(rng, 3, n_ant) if with_model else None
        vis, g_true = cal_oracle.synth_vis(rng, n_ant, 3, 2, K, model)
        flags = _flags(rng, vis, n_ant) if flagged else None
        ref = 1 if flagged else 0
        bf = bfmod.Beamformer(cfg)
        got_g, got_i = _solve(torch, bf, vis, model, flags)
        bf.close()
        want_g, want_i = cal_oracle.solve(vis, n_ant, model=model, flags=flags)
        live = np.ones(n_ant, bool) if flags is None else flags == 0
        truth = g_true * np.exp(-1j * np.angle(g_true[..., ref:ref + 1]))
        for name, g in (("device", got_g.view(np.float64)), ("oracle", want_g)):
            z = (g[..., 0] + 1j * g[..., 1]) / np.sqrt(K)
            err = np.abs(z - truth)[..., live].max() / np.abs(truth[..., live]).max()
            print("%d antennas, %s: max |g - g_true| / max |g_true| = %.3g" % (n_ant, name, err))
            assert err <= 1e-5, (n_ant, name, err)
            assert not g[..., ~live, :].any()
        assert np.all(got_i[..., 1] == 1) and np.array_equal(got_i, want_i) and np.array_equal(got_g, _bits(want_g))


def test_iteration_control(torch, bfmod):
    """max_iter = 3: status 0, iterations 3 and the oracle's gains after three iterations; max_iter = 1; a huge tol stops at iteration 2;
    ref_ant given explicitly, without flags and with them (the one flag byte is read back)."""
    rng = np.random.default_rng(11)
    n_ant = 20
    cfg = _cfg(bfmod, n_ant, 2, 3)
    vis, _ = cal_oracle.synth_vis(rng, n_ant, 3, 2, K, noise=2000)
    flags = np.zeros(n_ant, np.uint8)
    flags[[3, 9]] = 1
    bf = bfmod.Beamformer(cfg)
    for opt, fl, expect in ((dict(max_iter=3), None, (3, 0)), (dict(max_iter=1), None, (1, 0)), (dict(tol=1e3), None, (2, 1)),
                            (dict(max_iter=2, tol=0.0), None, (2, 0)), (dict(ref_ant=5), None, None), (dict(ref_ant=19), flags, None),
                            (dict(ref_ant=0, max_iter=7), flags, (7, 0))):
        got_g, got_i = _solve(torch, bf, vis, None, fl, **opt)
        want_g, want_i = cal_oracle.solve(vis, n_ant, flags=fl, **opt)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_g, _bits(want_g)), (opt, got_i.tolist(), want_i.tolist())
        if expect:
            assert np.all(got_i == np.array(expect)), (opt, got_i.tolist())
        if "ref_ant" in opt:
            r = want_g[:, :, opt["ref_ant"]]
            assert np.all(r[..., 0] > 0) and np.all(np.abs(r[..., 1]) <= 4 * 2.0 ** -52 * r[..., 0])
    bf.close()


def test_degenerate_inputs_give_zeros_not_nans(torch, bfmod):
    """All-zero visibilities; one unflagged antenna; a dead antenna (a zero row) among live ones; a negative diagonal.  No NaN or Inf
    anywhere, and the oracle's bits."""
    rng = np.random.default_rng(13)
    n_ant = 8
    cfg = _cfg(bfmod, n_ant, 2, 3)
    base, _ = cal_oracle.synth_vis(rng, n_ant, 3, 2, K)
    dead = base.copy()
    dead[:, :, [cal_oracle.bl(max(5, b), min(5, b)) for b in range(n_ant)]] = 0
    neg = base.copy()
    neg[:, :, cal_oracle.bl(2, 2), 0] = -5
    one = np.ones(n_ant, np.uint8)
    one[3] = 0
    bf = bfmod.Beamformer(cfg)
    for name, vis, flags in (("zeros", np.zeros_like(base), None), ("one antenna", base, one), ("dead antenna", dead, None), ("negative", neg, None)):
        for joint in (False, True):
            got_g, got_i = _solve(torch, bf, vis, None, flags, joint)
            want_g, want_i = cal_oracle.solve(vis, n_ant, flags=flags, joint_pol=joint)
            assert np.isfinite(want_g).all() and np.isfinite(got_g.view(np.float64)).all(), name
            assert np.array_equal(got_i, want_i) and np.array_equal(got_g, _bits(want_g)), (name, joint, got_i.tolist(), want_i.tolist())
        if name in ("zeros", "one antenna"):
            assert not want_g.any(), name
        if name == "dead antenna":
            assert not want_g[:, :, 5].any() and want_g[:, :, 4].any()
    bf.close()


def test_invalid_arguments_launch_nothing(torch, bfmod):
    """260 antennas, max_iter 0, a negative tol, ref_ant out of range or flagged, a NULL output, an unknown mode: BF_ERR_INVALID each,
    and the sentinels stay intact."""
    rng = np.random.default_rng(17)
    n_ant = 8
    cfg = _cfg(bfmod, n_ant, 2, 3)
    vis, _ = cal_oracle.synth_vis(rng, n_ant, 3, 2, K)
    flags = np.zeros(n_ant, np.uint8)
    flags[2] = 1
    bf = bfmod.Beamformer(cfg)
    d_vis, d_f = _dev(torch, vis), _dev(torch, flags)
    d_g, d_i = _outputs(torch, cfg, False)
    d_w = torch.full((3, n_ant, 8, 2), 0x7F, dtype=torch.int8, device="cuda")
    d_gl = torch.ones((3, n_ant, 2), dtype=torch.float64, device="cuda")
    bad = [lambda: bf.solve_gains(d_vis, d_g, d_i, max_iter=0), lambda: bf.solve_gains(d_vis, d_g, d_i, tol=-1e-3),
           lambda: bf.solve_gains(d_vis, d_g, d_i, tol=float("nan")),
           lambda: bf.solve_gains(d_vis, d_g, d_i, ref_ant=n_ant), lambda: bf.solve_gains(d_vis, d_g, d_i, ref_ant=-2),
           lambda: bf.solve_gains(d_vis, d_g, d_i, flags=d_f, ref_ant=2),
           lambda: bf.solve_gains(d_vis, None, d_i), lambda: bf.solve_gains(d_vis, d_g, None), lambda: bf.solve_gains(None, d_g, d_i),
           lambda: bf._lib.bf_solve_gains_device(bf._h, d_vis.data_ptr(), None, None, None, d_g.data_ptr(), d_i.data_ptr(), None),
           lambda: bf._lib.bf_calibrate_weights_device(bf._h, d_w.data_ptr(), d_gl.data_ptr(), None, 2, d_w.data_ptr(), None),
           lambda: bf.calibrate_weights(None, d_gl, d_w), lambda: bf.calibrate_weights(d_w, None, d_w), lambda: bf.calibrate_weights(d_w, d_gl, None)]
    for i, call in enumerate(bad):
        try:
            rc = call()
        except bfmod.DsabfError as e:
            rc = e.code
        assert rc == BF_ERR_INVALID, i
    with pytest.raises(ValueError):
        bf.calibrate_weights(d_w, d_gl, d_w, mode="both")
    bf.close()
    wide = bfmod.Beamformer(_cfg(bfmod, 260, 1, 1))
    d_wvis = torch.zeros((1, 1, 260 * 261 // 2, 2), dtype=torch.int64, device="cuda")
    d_wg, d_wi = _outputs(torch, wide.cfg, False)
    d_ww = torch.full((1, 260, 8, 2), 0x7F, dtype=torch.int8, device="cuda")
    d_wgl = torch.ones((1, 260, 2), dtype=torch.float64, device="cuda")
    for call in (lambda: wide.solve_gains(d_wvis, d_wg, d_wi), lambda: wide.calibrate_weights(d_ww, d_wgl, d_ww)):
        with pytest.raises(bfmod.DsabfError, match="256") as e:
            call()
        assert e.value.code == BF_ERR_INVALID
    wide.close()
    torch.cuda.synchronize()
    for t, fill in ((d_g, NAN_BITS), (d_i, INFO_FILL), (d_w, 0x7F), (d_wg, NAN_BITS), (d_wi, INFO_FILL), (d_ww, 0x7F)):
        assert torch.all(t == fill).item()


def test_two_solves_on_two_streams_without_synchronisation(torch, bfmod):
    """Two solves of different inputs into separate outputs on two streams, no synchronisation in between (the solver keeps nothing in
    the handle); then a solve queued on the stream of the bf_correlate_device that produces its input."""
    rng = np.random.default_rng(19)
    n_ant = 64
    cfg = _cfg(bfmod, n_ant, 2, 3, n_avg=4, n_out_per_gemm=8)
    bf = bfmod.Beamformer(cfg)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    fields = [cal_oracle.synth_vis(rng, n_ant, 3, 2, K, noise=500)[0] for _ in range(2)]
    d_vis = [_dev(torch, v) for v in fields]
    outs = [_outputs(torch, cfg, False) for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        bf.solve_gains(d_vis[k], outs[k][0], outs[k][1], stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        want_g, want_i = cal_oracle.solve(fields[k], n_ant)
        assert np.array_equal(outs[k][1].cpu().numpy(), want_i) and np.array_equal(outs[k][0].cpu().numpy(), _bits(want_g)), k
    assert not np.array_equal(outs[0][0].cpu().numpy(), outs[1][0].cpu().numpy())
    # correlate -> solve on one stream: random voltages are noise, so the iterations may run out; the bits still match
    n_units = 4
    packed = rng.integers(0, 256, size=(n_units, 3, cfg.n_out_per_gemm * 2 * cfg.n_avg, n_ant), dtype=np.uint8)
    d_in = torch.from_numpy(packed).cuda()
    d_v = torch.full((3, 2, corr_oracle.n_baselines(n_ant), 2), -1, dtype=torch.int64, device="cuda")
    d_g, d_i = _outputs(torch, cfg, True)
    torch.cuda.synchronize()
    s = streams[0].cuda_stream
    bf.correlate(d_in, n_units, d_v, stream=s)
    bf.solve_gains(d_v, d_g, d_i, joint_pol=True, max_iter=20, stream=s)
    torch.cuda.synchronize()
    vis = corr_oracle.visibilities(packed, 2)
    want_g, want_i = cal_oracle.solve(vis, n_ant, joint_pol=True, max_iter=20)
    assert np.array_equal(d_v.cpu().numpy(), vis)
    assert np.array_equal(d_i.cpu().numpy(), want_i) and np.array_equal(d_g.cpu().numpy(), _bits(want_g))
    bf.close()


def test_calibrated_weights_to_the_bit(torch, bfmod):
    """All 256 x 256 int8 (re, im) weight pairs, shuffled over one [4][64][256] array, against gains at random phases and amplitudes, in
    both modes, with flagged and zero-gain antennas.  BF_CAL_PHASE: a (127, 127) weight turned by 45 degrees clips to 127.  BF_CAL_FULL:
    amplitudes 1 and 2 in one channel make c = 0.5 exactly, which pins the ties to even.  No byte is -128."""
    rng = np.random.default_rng(23)
    n_freq, n_ant, n_beams = 4, 64, 256
    cfg = _cfg(bfmod, n_ant, 2, n_freq, n_beams=n_beams)
    pairs = rng.permutation(65536)
    w = np.stack([(pairs >> 8).astype(np.uint8).view(np.int8), (pairs & 255).astype(np.uint8).view(np.int8)], axis=-1).reshape(n_freq, n_ant, n_beams, 2)
    w[0, 0, 0] = (127, 127)
    w[1, 1, :8, 0] = (5, 7, -5, 1, 3, -1, 127, -127)                         # halves after c = 0.5: 2.5, 3.5, -2.5, 0.5, 1.5, -0.5, 63.5
    w[1, 1, :8, 1] = (0, 0, 0, 0, 0, 0, -128, 127)
    amp = rng.uniform(0.5, 1.5, size=(n_freq, n_ant))
    g = amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape))
    g[0, 0] = np.sqrt(0.5) - 1j * np.sqrt(0.5)                               # conj(g) / |g| turns by +45 degrees
    g[1] = np.where(np.arange(n_ant) % 2, 2.0, 1.0)                          # channel 1: amplitudes 1 and 2 only, zero phase
    g[2, 5] = 0.0                                                            # a zero gain
    gains = np.stack([g.real, g.imag], axis=-1)
    flags = np.zeros(n_ant, np.uint8)
    flags[[7, 62]] = 1
    bf = bfmod.Beamformer(cfg)
    d_w, d_gl = _dev(torch, w), _dev(torch, gains)
    for mode, code in (("phase", cal_oracle.PHASE), ("full", cal_oracle.FULL)):
        for fl in (None, flags):
            want = cal_oracle.calibrate_weights(w, gains, fl, code)
            d_out = torch.full(w.shape, 0x7F, dtype=torch.int8, device="cuda")
            bf.calibrate_weights(d_w, d_gl, d_out, flags=_dev(torch, fl), mode=mode)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            bad = np.argwhere(got != want)
            assert bad.size == 0, (mode, fl is not None, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])], w[tuple(bad[0][:3])])
            assert got.min() >= -127 and not got[2, 5].any()
            if fl is not None:
                assert not got[:, [7, 62]].any()
            if mode == "phase":
                assert got[0, 0, 0].tolist() == [0, 127]                     # 179.6i: clipped
                assert np.array_equal(got[1, 0], np.clip(w[1, 0], -127, 127))
            else:
                assert got[1, 1, :8, 0].tolist() == [2, 4, -2, 0, 2, 0, 64, -64]   # ties to even
                assert got[1, 1, 6:8, 1].tolist() == [-64, 64]
    d_same = d_w.clone()                                                     # in place
    bf.calibrate_weights(d_same, d_gl, d_same)
    torch.cuda.synchronize()
    assert np.array_equal(d_same.cpu().numpy(), cal_oracle.calibrate_weights(w, gains))
    bf.close()


def _calibrator_field(seed, n_ant, n_freq, n_units, n_out, n_avg):
    """4-bit voltages of one source at the phase centre, v = quantise(2 g_a x_t + 1.5 noise), |g| in 0.7 ... 1.3, random phases: the same
    gains for both polarisations.  -> (g complex [freq][ant], packed uint8 [unit][freq][time][ant])."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.7, 1.3, size=(n_freq, n_ant)) * np.exp(2j * np.pi * rng.uniform(size=(n_freq, n_ant)))
    n_t = n_out * n_avg * 2
    x = (rng.standard_normal((n_units, n_freq, n_t)) + 1j * rng.standard_normal((n_units, n_freq, n_t))) / np.sqrt(2)
    nz = (rng.standard_normal((n_units, n_freq, n_t, n_ant)) + 1j * rng.standard_normal((n_units, n_freq, n_t, n_ant))) / np.sqrt(2)
    v = 2 * g[None, :, None, :] * x[..., None] + 1.5 * nz
    re, im = np.clip(np.rint(v.real), -8, 7).astype(np.int64), np.clip(np.rint(v.imag), -8, 7).astype(np.int64)
    return g, (((re & 15) << 4) | (im & 15)).astype(np.uint8)


def test_a_calibrator_restores_the_beam(torch, bfmod):
    """End to end: 64 antennas, 3 channels, 8 beams, 2 polarisations, 2048 columns per polarisation of a calibrator seen through unknown
    gains.  bf_correlate_device -> bf_solve_gains_device (joint) -> bf_calibrate_weights_device on all-(127, 0) weights for beam 0 ->
    bf_set_weights_device -> bf_beamform_device.  (a) gains and weights equal corr_oracle -> cal_oracle to the bit; (b) the summed power
    of beam 0 is >= 0.95 x the power with weights made from the TRUE gains; (c) the uncalibrated power is <= 0.1 x it.  (On the CPU,
    from the oracles, this seed gives 1.0001 and 0.023.)"""
    n_ant, n_freq, n_beams, n_out, n_avg, n_units = 64, 3, 8, 8, 16, 16
    assert n_units * n_out * n_avg == 2048
    cfg = _cfg(bfmod, n_ant, 2, n_freq, n_beams=n_beams, n_avg=n_avg, n_out_per_gemm=n_out, n_gemms_per_block=n_units)
    g_true, packed = _calibrator_field(20261018, n_ant, n_freq, n_units, n_out, n_avg)
    w_in = np.zeros((n_freq, n_ant, n_beams, 2), np.int8)
    w_in[:, :, 0, 0] = 127
    bf = bfmod.Beamformer(cfg)
    d_in, d_w_in = torch.from_numpy(packed).cuda(), torch.from_numpy(w_in).cuda()
    d_vis = torch.full((n_freq, 2, corr_oracle.n_baselines(n_ant), 2), -1, dtype=torch.int64, device="cuda")
    d_g, d_i = _outputs(torch, cfg, True)
    d_w = torch.full(w_in.shape, 0x7F, dtype=torch.int8, device="cuda")
    bf.correlate(d_in, n_units, d_vis)
    bf.solve_gains(d_vis, d_g, d_i, joint_pol=True)
    bf.calibrate_weights(d_w_in, d_g, d_w)
    torch.cuda.synchronize()
    vis = corr_oracle.visibilities(packed, 2)
    want_g, want_i = cal_oracle.solve(vis, n_ant, joint_pol=True)
    want_w = cal_oracle.calibrate_weights(w_in, want_g[0])
    assert np.all(want_i[..., 1] == 1), want_i.tolist()
    assert np.array_equal(d_vis.cpu().numpy(), vis) and np.array_equal(d_i.cpu().numpy(), want_i)
    assert np.array_equal(d_g.cpu().numpy(), _bits(want_g)) and np.array_equal(d_w.cpu().numpy(), want_w)
    w_true = cal_oracle.calibrate_weights(w_in, np.stack([g_true.real, g_true.imag], axis=-1))

    def power(d_weights):
        d_out = torch.zeros((n_units * n_out, n_freq, n_beams), dtype=torch.float32, device="cuda")
        bf.set_weights_device(d_weights)
        bf.beamform(d_in, n_units, d_out)
        torch.cuda.synchronize()
        return float(d_out.cpu().numpy().astype(np.float64)[..., 0].sum())

    p_cal, p_true, p_raw = power(d_w), power(torch.from_numpy(w_true).cuda()), power(d_w_in)
    print("beam 0: calibrated / true = %.4f, uncalibrated / true = %.4f" % (p_cal / p_true, p_raw / p_true))
    assert p_true > 0 and p_cal >= 0.95 * p_true and p_raw <= 0.1 * p_true
    bf.close()


def test_beam_solve_mode_and_apply(torch, bfmod, tmp_path):
    """`beam -j 27 -a 1 -V vis.bin` as tests/test_gpu_corr.py runs it, then `beam -E vis.bin -G gains.bin` and the same with -P: every
    record equals the oracle on host.read_vis_file's records to the bit (the junk source is noise: status may be 0).  Then the DEBUG run
    `-p / -d / -s ... -A gains.bin -o data.py` completes, and the library's DEBUG flow with the same gains file (the flow `beam` calls)
    writes the same table and reports the weights it set: cal_oracle.calibrate_weights of the steering weights."""
    from dsabeamformer_amd import build, host

    vis_path = str(tmp_path / "vis.bin")
    r = subprocess.run([build.BEAM, "-j", "27", "-a", "1", "-V", vis_path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    vhdr, dumps = host.read_vis_file(vis_path)
    assert len(dumps) == 2
    n_ant, n_freq, n_pol = int(vhdr["NANT"]), int(vhdr["NFREQ"]), int(vhdr["NPOL"])
    for extra, joint in (([], False), (["-P"], True)):
        gains_path = str(tmp_path / ("gains%d.bin" % joint))
        r = subprocess.run([build.BEAM, "-E", vis_path, "-G", gains_path] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Wrote 2 gain records" in r.stdout, r.stdout + r.stderr
        ghdr, recs = host.read_gains_file(gains_path)
        assert ghdr["CONTENT"] == "gains" and ghdr["DTYPE"] == "float64" and ghdr["LAYOUT"] == "pol,freq,ant,reim"
        assert (int(ghdr["NANT"]), int(ghdr["NPOL"]), int(ghdr["NFREQ"]), int(ghdr["FIRST_CHANNEL"])) == (n_ant, 1 if joint else n_pol, n_freq, 0)
        assert len(recs) == 2
        for (first_block, n_columns, vis), (b, c, g, info) in zip(dumps, recs):
            want_g, want_i = cal_oracle.solve(vis, n_ant, joint_pol=joint)
            assert (b, c) == (first_block, n_columns) and np.array_equal(info, want_i) and np.array_equal(_bits(g), _bits(want_g))
    # ---- -A in the DEBUG run: a gains file of the DEBUG geometry, one joint layer with phases and amplitudes
    dbg = bfmod.debug_config()
    rng = np.random.default_rng(31)
    amp = rng.uniform(0.5, 1.5, size=(1, dbg.n_freq, dbg.n_ant))
    g = amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape))
    layer = np.stack([g.real, g.imag], axis=-1)
    apply_path = str(tmp_path / "apply.bin")
    host.write_gains_file(apply_path, n_ant=dbg.n_ant, n_pol=1, n_freq=dbg.n_freq, first_channel=0,
                          records=[(0, 1, np.zeros_like(layer), np.zeros((1, dbg.n_freq, 2), np.int32)),      # the LAST record counts
                                   (1, 1, layer, np.ones((1, dbg.n_freq, 2), np.int32))])
    cfgdir = os.path.join(ROOT, "tests", "golden", "config")
    files = ["-p", os.path.join(cfgdir, "linear_positions.txt"), "-d", os.path.join(cfgdir, "linear_directions.txt"),
             "-s", os.path.join(cfgdir, "linear_source_directions_1024.txt")]
    out_cli, out_plain = str(tmp_path / "data.py"), str(tmp_path / "plain.py")
    r = subprocess.run([build.BEAM] + files + ["-A", apply_path, "-o", out_cli], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Calibrated the weights" in r.stdout and os.path.getsize(out_cli) > 0, r.stdout + r.stderr
    r = subprocess.run([build.BEAM] + files + ["-o", out_plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out_cli).read() != open(out_plain).read()                    # the gains changed the beams
    out_lib = str(tmp_path / "lib.py")
    res = host.run_debug_observation(dbg, positions=files[1], directions=files[3], sources=files[5], output=out_lib, gains=apply_path,
                                     return_weights=True)
    assert open(out_lib).read() == open(out_cli).read()
    steering = host.make_weights(host.read_positions(files[1], dbg.n_ant), host.read_directions(files[3], dbg.n_beams), dbg.n_freq)
    assert np.array_equal(res["weights"], cal_oracle.calibrate_weights(steering, layer[0]))
    assert not np.array_equal(res["weights"], steering)
