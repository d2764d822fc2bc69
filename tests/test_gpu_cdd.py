"""GPU tests (-m gpu) of coherent dedispersion (include/dsabf.h: bf_stokes_voltages_device, bf_cdd_*; docs/COHERENT_DEDISPERSION.md).
The references are tests/support/stokes_oracle.py (exact integers) and tests/support/cdd_oracle.py (the fixed float32 operation order
in numpy, and a complex128 restatement on numpy.fft).  Outputs are sentinel-filled with guard cells behind them and compared whole and
BIT FOR BIT (as uint32 words) unless a test says otherwise.

Every test is ONE function that loops over its cases, as tests/test_gpu_stokes.py does: none of the cases may be thinned out."""
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

SUPPORT = os.path.join(ROOT, "tests", "support")
sys.path.insert(0, SUPPORT)
import cdd_oracle as co  # noqa: E402
import stokes_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
SENTINEL = -0x3EDCBA99          # as int32: a NaN pattern no arithmetic here produces
GUARD = 8                       # float32 words behind every output
BW = 250.0 / 2048               # MHz: one channel


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
def handle(bfmod):
    """The chirp filter takes nothing from the handle's geometry: one small handle serves every test of it."""
    bf = bfmod.Beamformer(_cfg(bfmod, 4, 1, 1, n_beams=4, n_freq=1))
    yield bf
    bf.close()


def _cfg(bfmod, n_ant, n_avg, n_out, n_beams=32, n_freq=3, **over):
    kw = dict(n_ant=n_ant, n_pol=2, n_avg=n_avg, n_beams=n_beams, n_freq=n_freq, n_out_per_gemm=n_out, n_gemms_per_block=4,
              n_blocks_on_gpu=2, n_streams=4)
    kw.update(over)
    return bfmod.debug_config(**kw)


def _sentinels(torch, n_words, shift_words=0):
    """A device float32 buffer of n_words + GUARD words (plus the shift), every word the sentinel; returns (buffer, view to write into)."""
    buf = torch.full((shift_words + n_words + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[shift_words:]


def _words(buf, n_words, shift_words=0):
    """The n_words written, as uint32; everything around them must still be the sentinel."""
    got = buf.cpu().numpy()
    assert (got[:shift_words] == SENTINEL).all() and (got[shift_words + n_words:] == SENTINEL).all(), "a guard word was written"
    return got[shift_words:shift_words + n_words].view(np.uint32)


def _same_bits(got_words, want, case):
    want_words = np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    assert got_words.shape == want_words.shape, (case, got_words.shape, want_words.shape)
    bad = np.flatnonzero(got_words != want_words)
    assert bad.size == 0, (case, len(bad), bad[:4], got_words[bad[:4]], want_words[bad[:4]])


def _c64(re, im):
    out = np.empty(np.shape(re), np.complex64)
    out.real, out.imag = re, im
    return out


# ---- A. the beam voltages ---------------------------------------------------------------------------------------------------------
def _want_voltages(packed, w, beams):
    """stokes_oracle.beam_samples as complex64 [freq][k][pol][n_units * S]."""
    re, im = so.beam_samples(packed, w, beams)                                   # int64 [u][f][c][k]
    u, f, c, k = re.shape
    assert max(np.abs(re).max(), np.abs(im).max()) <= 2 ** 19 + 2 ** 12          # exact in float32
    z = _c64(re.astype(np.float32), im.astype(np.float32)).reshape(u, f, c // 2, 2, k)
    return np.ascontiguousarray(z.transpose(1, 4, 3, 0, 2)).reshape(f, k, 2, u * (c // 2))


def _run_voltages(torch, stage, packed, n_units, want, case, shift_words=0):
    buf, view = _sentinels(torch, want.size * 2, shift_words)
    stage.voltages(torch.from_numpy(packed).cuda(), n_units, view)
    torch.cuda.synchronize()
    _same_bits(_words(buf, want.size * 2, shift_words), want, case)


DESC16 = list(range(31, 15, -1))
# (n_ant, beams, n_avg, n_out, n_freq, n_units): S = n_avg * n_out = 1, 3 (odd: the 8-byte tail store), 8, 24, 256
# 128, 132, 192 and 252 antennas: with 4 / 12, 64, 68 and 256 every (k-steps, 16-byte loads) pair of stokes_kernel runs its voltages mode
VOLTAGE_CASES = [(4, [0], 1, 1, 1, 1), (4, [31, 0, 7], 1, 3, 3, 3), (12, [5], 1, 3, 1, 1), (12, DESC16, 8, 1, 3, 3), (12, [9, 3, 31], 8, 3, 1, 3),
                 (68, [31, 0, 15], 1, 3, 3, 1), (68, DESC16, 8, 3, 1, 3), (68, [1], 16, 16, 1, 1), (64, DESC16, 16, 16, 3, 1), (64, [31], 1, 1, 1, 3),
                 (64, [2, 31, 0], 8, 1, 3, 3), (256, DESC16, 1, 3, 1, 3), (256, [0, 16, 31], 8, 3, 3, 1), (256, [31], 16, 16, 1, 3),
                 (128, DESC16, 8, 3, 1, 3), (128, [7], 1, 1, 3, 1), (132, [31, 0, 15], 1, 3, 3, 3), (132, DESC16, 8, 1, 1, 1),
                 (192, [0, 16, 31], 8, 3, 3, 1), (192, [4], 1, 3, 1, 3), (252, DESC16, 1, 1, 3, 3), (252, [9, 3, 31], 8, 3, 1, 1)]


def test_beam_voltages_to_the_bit(torch, bfmod):
    """bf_stokes_voltages_device against stokes_oracle.beam_samples: random bytes (every code) and weights over all of int8 on every
    shape; an output that is only 8-byte aligned; the all-byte-codes scene with the weight extremes; the 2^19 bound."""
    from dsabeamformer_amd import api

    for lst, idx in (((4, 12, 68, 64, 128, 132, 192, 252, 256), 0), ((1, 3), 4), ((1, 3), 5)):
        assert {c[idx] for c in VOLTAGE_CASES} == set(lst), idx
    assert {len(c[1]) for c in VOLTAGE_CASES} == {1, 3, 16} and {c[2] * c[3] for c in VOLTAGE_CASES} == {1, 3, 8, 24, 256}
    rng = np.random.default_rng(20261021)
    t0 = time.perf_counter()
    for case in VOLTAGE_CASES:
        n_ant, beams, n_avg, n_out, n_freq, n_units = case
        cfg = _cfg(bfmod, n_ant, n_avg, n_out, n_freq=n_freq)
        packed = rng.integers(0, 256, size=(n_units, n_freq, 2 * n_avg * n_out, n_ant), dtype=np.uint8)
        w = rng.integers(-128, 128, size=(n_freq, n_ant, 32, 2), dtype=np.int8)
        want = _want_voltages(packed, w, beams)
        bf = bfmod.Beamformer(cfg)
        stage = api.StokesBeams(bf, 1)
        stage.set_weights(w, beams)
        assert bf._lib.bf_stokes_voltage_entries(cfg, len(beams)) * n_units == want.size, case
        for shift in (0, 2):                                                     # 16-byte aligned, and 8-byte aligned only
            api.stage_launches(clear=True)
            _run_voltages(torch, stage, packed, n_units, want, (case, shift), shift)
            name = "stokes_kernel<%d, %s, 3>" % ((n_ant + 63) // 64, "true" if n_ant % 16 == 0 else "false")   # mode 3: the voltages
            assert name in api.stage_launches(), (case, api.stage_launches())
        stage.close()
        bf.close()
    # every byte code at every byte position of a lane's word, weights from the extremes of int8 (the scene of tests/test_gpu_stokes.py)
    for n_ant in (64, 68):
        cfg = _cfg(bfmod, n_ant, 16, 8, n_freq=2)
        c, a = np.meshgrid(np.arange(256), np.arange(n_ant), indexing="ij")
        packed = np.broadcast_to(((c + a) % 256).astype(np.uint8), (2, 2, 256, n_ant)).copy()
        w = rng.choice(np.array([-128, -127, -1, 0, 1, 127], np.int8), size=(2, n_ant, 32, 2))
        bf = bfmod.Beamformer(cfg)
        stage = api.StokesBeams(bf, 16)                                          # (the stage's own n_int does not matter to the voltages)
        stage.set_weights(torch.from_numpy(w).cuda(), [31, 0, 16, 5])
        _run_voltages(torch, stage, packed, 2, _want_voltages(packed, w, [31, 0, 16, 5]), ("codes", n_ant))
        stage.close()
        bf.close()
    # 256 antennas, every voltage (-8, -8): weights (-128, -128) give (0, 2^19), weights (-128, 127) give (522240, 2048)
    cfg = _cfg(bfmod, 256, 16, 8, n_freq=1)
    packed = np.full((1, 1, 256, 256), 0x88, np.uint8)
    bf = bfmod.Beamformer(cfg)
    stage = api.StokesBeams(bf, 1)
    for (wr, wi), (re, im) in (((-128, -128), (0, 2 ** 19)), ((-128, 127), (522240, 2048))):
        w = np.empty((1, 256, 32, 2), np.int8)
        w[..., 0], w[..., 1] = wr, wi
        stage.set_weights(w, [0, 31])
        want = np.full((1, 2, 2, 128), re + 1j * im, np.complex64)
        assert np.array_equal(want, _want_voltages(packed, w, [0, 31]))
        _run_voltages(torch, stage, packed, 1, want, ("bound", wr, wi))
    stage.close()
    bf.close()
    print("voltages: %d shapes, %.1f s" % (len(VOLTAGE_CASES), time.perf_counter() - t0))


# ---- B. the chirp filter ----------------------------------------------------------------------------------------------------------
def _random_table(rng, n_chan, n):
    """Any table is legal: unit-modulus bins of random phase, a different row per channel, with the 1 / n of the inverse transform."""
    phi = rng.uniform(0, 2 * np.pi, size=(n_chan, n))
    return _c64((np.cos(phi) / n).astype(np.float32), (np.sin(phi) / n).astype(np.float32))


def _full_scale(rng, shape):
    return _c64(rng.integers(-2 ** 19, 2 ** 19 + 1, size=shape).astype(np.float32), rng.integers(-2 ** 19, 2 ** 19 + 1, size=shape).astype(np.float32))


def _run_cdd(torch, stage, x, n_int, want, case, shift_words=0):
    """n_int 0: the voltage output.  x complex64 [chan][k][2][n_time] is uploaded behind one spare sample, so that a shift makes the
    first series start on an address that is 8-byte aligned only."""
    n_chan, K, _, n_time = x.shape
    d_x = torch.zeros((x.size + 1) * 2, dtype=torch.float32, device="cuda")
    off = 2 if shift_words else 0
    d_x[off:off + 2 * x.size] = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(-1)).cuda()
    n_words = want.size * (2 if n_int == 0 else 1)
    buf, view = _sentinels(torch, n_words, shift_words)
    if n_int == 0:
        stage.voltages(d_x[off:], K, n_time, view)
    else:
        stage.stokes(d_x[off:], K, n_time, n_int, view)
    torch.cuda.synchronize()
    _same_bits(_words(buf, n_words, shift_words), want, case)


def test_every_fft_length_and_edge_to_the_bit(torch, bfmod, handle):
    """N 64, 128, 256, 512, 1024, 2048, 4096 (every cdd_kernel<log2 N, *>; 512 and 2048 behind the others, which keep their inputs);
    n_edge 0, 1, N / 4; n_time 1, V - 1, V, V + 1, 2 V, 3 V + 5 and an odd length (every second series
    starts on an address that is 8-byte aligned only); 1 and 3 channels with a row of their own each; K 1, 3, 16; both outputs, n_int
    1, 2, V wherever it divides; full-scale integers, and an impulse at the first, the last and a seam sample."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(20261022)
    t0, n_cases, n_words = time.perf_counter(), 0, 0
    shapes = [(1, 1), (3, 3), (1, 16), (3, 1)]                                   # (n_chan, K), taken in turn
    turn = 0
    for n in (64, 128, 256, 1024, 4096, 512, 2048):
        for n_edge in (0, 1, n // 4):
            v = n - 2 * n_edge
            lengths = [1, v - 1, v, v + 1, 2 * v, 3 * v + 5]
            lengths.append(3 * v + 5 + (3 * v + 5) % 2 + 1)                      # and one that is certainly odd
            assert any(t % 2 for t in lengths) and all(t >= 1 for t in lengths)
            for n_time in lengths:
                n_chan, K = shapes[turn % 4] if n <= 1024 else shapes[turn % 2]  # (the two longest transforms at the two smaller shapes)
                turn += 1
                table = _random_table(rng, n_chan, n)
                stage = api.CoherentDedisperser(handle, n_chan, n, n_edge, table)
                assert stage.n_valid == v
                inputs = [("full scale", _full_scale(rng, (n_chan, K, 2, n_time)))]
                for name, at in (("first", 0), ("last", n_time - 1), ("seam", min(v - 1, n_time - 1)), ("behind the seam", min(v, n_time - 1))):
                    x = np.zeros((n_chan, K, 2, n_time), np.complex64)
                    x[..., at] = 2 ** 19 - 1j * 2 ** 19
                    x[:, :, 1, at] *= 1j                                         # (Y differs from X)
                    inputs.append((name, x))
                for name, x in inputs:
                    y = co.dedisperse(x, table, n_edge)
                    assert y.shape == x.shape and np.isfinite(y.view(np.float32)).all()
                    case = (n, n_edge, n_time, n_chan, K, name)
                    for shift in ((0, 2) if name == "full scale" else (0,)):
                        api.stage_launches(clear=True)
                        _run_cdd(torch, stage, x, 0, y, case + ("voltages", shift), shift)
                        assert set(api.stage_launches()) == {"cdd_kernel<%d, false>" % (n.bit_length() - 1)}, (case, api.stage_launches())
                    for n_int in (1, 2, v):
                        if n_time % n_int:
                            continue
                        want = co.stokes(y, n_int)
                        assert want.shape == (n_time // n_int, n_chan, K, 4)
                        api.stage_launches(clear=True)
                        _run_cdd(torch, stage, x, n_int, want, case + ("stokes", n_int), 2 if n_int == 2 else 0)
                        assert set(api.stage_launches()) == {"cdd_kernel<%d, true>" % (n.bit_length() - 1)}, (case, api.stage_launches())
                        n_words += want.size
                    n_cases += 1
                    n_words += 2 * y.size
                stage.close()
    print("cdd_kernel: %d inputs, %d words compared, %.1f s" % (n_cases, n_words, time.perf_counter() - t0))


def test_accuracy_against_fp64(torch, bfmod, handle):
    """The device's own voltage output against complex128 on numpy.fft, n_edge = 0, whole segments: per segment the relative 2-norm
    error is at most (14 log2 N + 4) 2^-24 -- Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: m eta per radix-2
    transform with eta about 6.7 u for correctly rounded twiddles, two transforms, 4 u for the rounded table and the multiply."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(5)
    for n in (64, 128, 256, 1024, 4096, 512, 2048):
        table = _random_table(rng, 2, n)
        x = _full_scale(rng, (2, 3, 2, 4 * n))
        stage = api.CoherentDedisperser(handle, 2, n, 0, table)
        d_x = torch.from_numpy(x.view(np.float32)).cuda()
        d_y = torch.zeros_like(d_x)
        stage.voltages(d_x, 3, 4 * n, d_y)
        torch.cuda.synchronize()
        got = d_y.cpu().numpy().view(np.complex64).reshape(x.shape).astype(np.complex128)
        want = co.dedisperse64(x, table, 0)
        err = np.linalg.norm((got - want).reshape(-1, n), axis=1) / np.linalg.norm(want.reshape(-1, n), axis=1)
        bound = (14 * np.log2(n) + 4) * 2.0 ** -24
        print("N %d: largest relative error of a segment %.2f u, bound %.0f u" % (n, err.max() * 2 ** 24, bound * 2 ** 24))
        assert err.shape == (2 * 3 * 2 * 4,) and err.max() <= bound, (n, err.max(), bound)
        stage.close()


def test_a_dispersed_impulse_comes_back(torch, bfmod, handle):
    """DM 500 at 1.28 GHz, N = 256, the edge of bf_cdd_edge: an impulse dispersed by one transform of 8192 samples (complex128, the
    conjugate chirp), placed at every 1 / 64 of one V -- 64 series, the K axis of one launch -- comes back through the device with at
    least 0.99 of the output energy in the impulse's sample, and the peak there."""
    from dsabeamformer_amd import api

    dm, f, n = 500.0, 1.28, 256
    n_edge = api.cdd_edge(dm, [f], BW)
    assert n_edge == 30
    v = n - 2 * n_edge
    table = api.cdd_chirp(dm, [f], BW, 1, n)
    at = [3000 + (i * v) // 64 for i in range(64)]
    x = np.zeros((1, 64, 2, 8192), np.complex64)
    for k, a in enumerate(at):
        d = co.dispersed_impulse(dm, f, BW, 1, a) * 2 ** 19
        x[0, k, 0], x[0, k, 1] = d, 1j * d
    before = np.abs(x[0, 0, 0].astype(np.complex128)) ** 2
    assert before.max() / before.sum() < 0.1                                    # (smeared over tens of samples)
    stage = api.CoherentDedisperser(handle, 1, n, n_edge, table)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    d_y = torch.zeros_like(d_x)
    stage.voltages(d_x, 64, 8192, d_y)
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().view(np.complex64).reshape(x.shape)
    p = np.abs(y.astype(np.complex128)) ** 2
    worst = 1.0
    for k, a in enumerate(at):
        for pol in (0, 1):
            assert int(np.argmax(p[0, k, pol])) == a, (k, pol)
            worst = min(worst, p[0, k, pol, a] / p[0, k, pol].sum())
    print("smallest fraction of the energy in the impulse's sample: %.4f" % worst)
    assert worst >= 0.99, worst
    stage.close()


def test_cut_to_coherent_stokes(torch, bfmod):
    """A pulse dispersed over 3 channels at 64 antennas (the scene of tests/test_gpu_vcut.py): VoltageHistory.cut ->
    StokesBeams.voltages -> CoherentDedisperser.stokes on one stream with nothing synchronised in between equals the three oracles
    chained."""
    import vcut_oracle as vo

    from dsabeamformer_amd import api

    rng = np.random.default_rng(8)
    cfg = _cfg(bfmod, 64, 2, 8, n_freq=3)
    S, n_units = 16, 6
    delays = np.array([[0, 0, 0], [0, 9, 21]], np.int32)
    units = rng.integers(0, 256, size=(n_units, 3, S, 128), dtype=np.uint8) & 0x11
    pulse_at = 2 * S + 3
    series = vo.series_of(units)
    for f in range(3):
        series[pulse_at + delays[1][f]:pulse_at + delays[1][f] + 4, f] = rng.integers(0, 256, size=(4, 128), dtype=np.uint8)
    units = np.ascontiguousarray(series.reshape(n_units, S, 3, 128).transpose(0, 2, 1, 3))
    w = rng.integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8)
    beams, n_out_units, n_fft, n_edge, n_int = [31, 0, 7], 2, 64, 8, 4
    n_time = n_out_units * S                                                     # 32 samples: one segment of V = 48
    freq = [1.28 + 0.01 * f for f in range(3)]
    table = api.cdd_chirp(60.0, freq, BW, -1, n_fft)
    t0 = pulse_at - S - 3
    want_cut, st_want = vo.cut(units, delays, [(t0, 1)], n_out_units, 0, n_units)
    assert list(st_want) == [0]
    volts = _want_voltages(want_cut[0].reshape(n_out_units, 3, S * 2, 64), w, beams)
    want = co.stokes(co.dedisperse(volts, table, n_edge), n_int)
    assert want.shape == (n_time // n_int, 3, 3, 4) and want[..., 0].max() > 0

    bf = bfmod.Beamformer(cfg)
    vh = api.VoltageHistory(bf, delays, n_units)
    stage = api.StokesBeams(bf, 1)
    stage.set_weights(w, beams)
    cdd = api.CoherentDedisperser(bf, 3, n_fft, n_edge, table)
    st = torch.cuda.Stream()
    d_units = torch.from_numpy(units).cuda()
    d_cut = torch.full((want_cut.size,), vo.SENTINEL, dtype=torch.uint8, device="cuda")
    d_volts = torch.zeros(volts.size * 2, dtype=torch.float32, device="cuda")
    buf, view = _sentinels(torch, want.size)
    torch.cuda.synchronize()
    vh.push(d_units, n_units, st.cuda_stream)
    assert list(vh.cut([(t0, 1)], n_out_units, d_cut, st.cuda_stream)) == [0]
    stage.voltages(d_cut, n_out_units, d_volts, st.cuda_stream)
    cdd.stokes(d_volts, len(beams), n_time, n_int, view, st.cuda_stream)
    st.synchronize()
    _same_bits(_words(buf, want.size), want, "the chain")
    cdd.close()
    stage.close()
    vh.close()
    bf.close()


def test_set_chirp_is_ordered(torch, bfmod, handle):
    """A kernel queued behind a busy stream, set_chirp with another table, then a second kernel: each result matches its own table --
    the upload waits for the first kernel, the second kernel for the upload."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(47)
    n, n_edge, n_time = 256, 16, 1000
    ta, tb = _random_table(rng, 2, n), _random_table(rng, 2, n)
    x = _full_scale(rng, (2, 3, 2, n_time))
    wa, wb = co.dedisperse(x, ta, n_edge), co.dedisperse(x, tb, n_edge)
    assert not np.array_equal(wa, wb)
    stage = api.CoherentDedisperser(handle, 2, n, n_edge, ta)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    buf_a, view_a = _sentinels(torch, 2 * x.size)
    buf_b, view_b = _sentinels(torch, 2 * x.size)
    big = torch.randn((8192, 8192), device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            torch.mm(big, big)
    stage.voltages(d_x, 3, n_time, view_a, s1.cuda_stream)                       # runs when s1 gets to it, with table A
    stage.set_chirp(tb)                                                          # must not land under that kernel
    stage.voltages(d_x, 3, n_time, view_b, s2.cuda_stream)
    torch.cuda.synchronize()
    _same_bits(_words(buf_a, 2 * x.size), wa, "the kernel before set_chirp")
    _same_bits(_words(buf_b, 2 * x.size), wb, "the kernel after set_chirp")
    stage.close()


def test_refusals_and_lifetime(torch, bfmod):
    """Every BF_ERR_INVALID / BF_ERR_STATE of both pieces with the outputs' sentinels intact, then the handle destroyed first."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(37)

    def refused(code, call):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == code and str(e.value), (e.value.code, str(e.value))

    cfg = _cfg(bfmod, 64, 2, 4)                                                  # S = 8
    bf = bfmod.Beamformer(cfg)
    packed = rng.integers(0, 256, size=(2, 3, 16, 64), dtype=np.uint8)
    w = rng.integers(-128, 128, size=(3, 64, 32, 2), dtype=np.int8)
    d_in = torch.from_numpy(packed).cuda()
    buf, view = _sentinels(torch, 2 * 3 * 2 * 2 * 16 * 2)
    sb = api.StokesBeams(bf, 1)
    refused(BF_ERR_STATE, lambda: sb.voltages(d_in, 1, view))                    # before any weights
    sb.set_weights(w, [3, 1])
    refused(BF_ERR_INVALID, lambda: sb.voltages(None, 1, view))
    refused(BF_ERR_INVALID, lambda: sb.voltages(d_in, 1, None))
    refused(BF_ERR_INVALID, lambda: sb.voltages(d_in, 0, view))
    refused(BF_ERR_INVALID, lambda: sb.voltages(d_in, -1, view))
    refused(BF_ERR_INVALID, lambda: sb.voltages(d_in, 1, view.data_ptr() + 4))   # not 8-byte aligned
    refused(BF_ERR_INVALID, lambda: sb.voltages(d_in, 2 ** 28, view))            # 2^28 units of 8 samples: a series of 2^31
    assert bf._lib.bf_stokes_voltage_entries(cfg, 2) == 3 * 2 * 2 * 8 and bf._lib.bf_stokes_voltage_entries(cfg, 17) == 0

    n, n_edge = 64, 8
    table = _random_table(rng, 2, n)
    for bad_n in (0, 32, 96, 8192, -64):
        refused(BF_ERR_INVALID, lambda: api.CoherentDedisperser(bf, 2, bad_n, 0, np.zeros((2, max(bad_n, 1)), np.complex64)))
    for bad_edge in (-1, n // 4 + 1):
        refused(BF_ERR_INVALID, lambda: api.CoherentDedisperser(bf, 2, n, bad_edge, table))
    refused(BF_ERR_INVALID, lambda: api.CoherentDedisperser(bf, 0, n, n_edge, np.zeros((0, n), np.complex64)))
    refused(BF_ERR_INVALID, lambda: api.CoherentDedisperser(bf, 2, n, n_edge, None))
    cdd = api.CoherentDedisperser(bf, 2, n, n_edge, table)                       # V = 48
    x = _full_scale(rng, (2, 3, 2, 96))
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    calls = [lambda: cdd.voltages(None, 3, 96, view), lambda: cdd.voltages(d_x, 3, 96, None), lambda: cdd.stokes(None, 3, 96, 1, view),
             lambda: cdd.voltages(d_x, 0, 96, view), lambda: cdd.stokes(d_x, -1, 96, 1, view),
             lambda: cdd.voltages(d_x, 3, 0, view), lambda: cdd.voltages(d_x, 3, -5, view), lambda: cdd.voltages(d_x, 3, 2 ** 31, view),
             lambda: cdd.stokes(d_x, 3, 2 ** 31, 1, view),
             lambda: cdd.stokes(d_x, 3, 96, 0, view), lambda: cdd.stokes(d_x, 3, 96, -2, view),
             lambda: cdd.stokes(d_x, 3, 96, 5, view),                            # divides neither
             lambda: cdd.stokes(d_x, 3, 96, 32, view),                           # divides n_time, not V = 48
             lambda: cdd.stokes(d_x, 3, 88, 16, view),                           # divides V, not n_time = 88
             lambda: cdd.voltages(d_x.data_ptr() + 4, 3, 96, view), lambda: cdd.voltages(d_x, 3, 96, view.data_ptr() + 4),
             lambda: cdd.stokes(d_x, 3, 96, 1, view.data_ptr() + 4),
             lambda: cdd.voltages(d_x, 2 ** 30, 96, view),                       # 2 segments x 2 channels x 2^30 beams: the grid axis
             lambda: cdd.set_chirp(None)]
    for call in calls:
        refused(BF_ERR_INVALID, call)
    torch.cuda.synchronize()
    _words(buf, 0)                                                               # every word is still the sentinel
    # and the stage still works: both outputs at K = 3
    y = co.dedisperse(x, table, n_edge)
    _run_cdd(torch, cdd, x, 0, y, "after the refusals")
    _run_cdd(torch, cdd, x, 16, co.stokes(y, 16), "after the refusals, Stokes")
    bf.close()                                                                   # the handle first
    for call in (lambda: cdd.voltages(d_x, 3, 96, view), lambda: cdd.stokes(d_x, 3, 96, 1, view), lambda: cdd.set_chirp(table),
                 lambda: sb.voltages(d_in, 1, view)):
        refused(BF_ERR_STATE, call)
    cdd.close()
    sb.close()


def test_beam_coherent_mode(bfmod, tmp_path):
    """`beam -j 33 ... --voltages v.bin --voltage-units 2` as in tests/test_gpu_vcut.py, then `beam --coherent v.bin --coherent-out c.bin -M 250
    -N 8`: every record of c.bin equals the oracle chain over ITS cut -- the beam voltages of the record's beam with the weights the run
    used, the chirp at the DM of its trial, the edge of bf_cdd_edge, the smallest FFT length of at least 256 -- there is at least one
    record, and the first run's files are the same bytes afterwards."""
    import subprocess

    from dsabeamformer_amd import api, build, host

    names = ("det.bin", "dm.bin", "cands.txt", "ev.txt", "v.bin", "c.bin", "c2.bin")
    det_file, dm_file, cand_file, ev_file, v_file, c_file, c2_file = (str(tmp_path / n) for n in names)
    base = [build.BEAM, "-j", "33", "-M", "250", "-N", "8", "-S", "4", "-B", "6", "-i", "255"]
    r = subprocess.run(base + ["-w", det_file, "-W", dm_file, "-C", cand_file, "--events", ev_file, "--voltages", v_file, "--voltage-units", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    first_run = {f: open(f, "rb").read() for f in (det_file, dm_file, cand_file, ev_file, v_file)}
    r = subprocess.run([build.BEAM, "--coherent", v_file, "--coherent-out", c_file, "-M", "250", "-N", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    for f, data in first_run.items():
        assert open(f, "rb").read() == data, f
    vhdr, cuts = host.read_voltage_file(v_file)
    hdr, recs = host.read_coherent_file(c_file)
    assert len(recs) == len(cuts) >= 1
    line = "Coherent dedispersion: %d of %d cuts of 256 samples x 256 channels, windows of 1 samples; refused: 0 with" % (len(cuts), len(cuts))
    assert line in r.stdout and "Wrote %d coherently dedispersed cuts" % len(cuts) in r.stdout, r.stdout[-1500:]
    assert [hdr[k] for k in ("CONTENT", "DTYPE", "NFREQ", "NFFT", "NINT", "SIDEBAND", "LAYOUT", "NTIME", "FIRST_CHANNEL")] == \
        ["coherent_stokes", "float32", "256", "0", "1", "1", "time,freq,iquv", "256", "0"]
    cfg = bfmod.production_config()
    S = cfg.n_out_per_gemm * cfg.n_avg
    dms = host.dm_trials(dm_max=250.0)
    dms = [float(dms[int(i * (len(dms) - 1) / 7)]) for i in range(8)]
    freq = [float(np.float32(host.channel_frequency(0, ch))) for ch in range(cfg.n_freq)]
    bw = cfg.n_avg / (1000.0 * 0.131)
    w = host.make_weights(host.default_positions(cfg.n_ant), host.default_directions(cfg.n_beams), cfg.n_freq, 0, 0)

    def chain(cut, n_fft, n_int):
        dm = dms[cut["dm"]]
        n_edge = api.cdd_edge(dm, freq, bw)
        n = n_fft or next(m for m in (256, 512, 1024, 2048, 4096) if n_edge <= m // 4)
        volts = _want_voltages(cut["data"].reshape(2, cfg.n_freq, 2 * S, cfg.n_ant), w, [cut["beam"]])
        return dm, n_edge, n, co.stokes(co.dedisperse(volts, api.cdd_chirp(dm, freq, bw, 1, n), n_edge), n_int)[:, :, 0, :]

    for cut, rec in zip(cuts, recs):
        dm, n_edge, n, want = chain(cut, 0, 1)
        assert (rec["t0"], rec["dm"], rec["beam"], rec["width"], rec["snr"]) == (cut["t0"], cut["dm"], cut["beam"], cut["width"], cut["snr"])
        assert (rec["dm_value"], rec["n_edge"], rec["n_fft"]) == (dm, n_edge, n) and n == 256
        _same_bits(np.ascontiguousarray(rec["data"]).view(np.uint32).reshape(-1), want, ("record", cut["t0"], cut["dm"], cut["beam"]))
    # a given length, windows of 2 samples, the other sideband
    r = subprocess.run([build.BEAM, "--coherent", v_file, "--coherent-out", c2_file, "-M", "250", "-N", "8", "--coherent-fft", "128", "--coherent-int", "2",
                        "--coherent-sideband", "-1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    hdr2, recs2 = host.read_coherent_file(c2_file)
    assert (hdr2["NFFT"], hdr2["NINT"], hdr2["SIDEBAND"]) == ("128", "2", "-1") and len(recs2) == len(cuts)
    for cut, rec in zip(cuts, recs2):
        dm = dms[cut["dm"]]
        n_edge = api.cdd_edge(dm, freq, bw)
        volts = _want_voltages(cut["data"].reshape(2, cfg.n_freq, 2 * S, cfg.n_ant), w, [cut["beam"]])
        want = co.stokes(co.dedisperse(volts, api.cdd_chirp(dm, freq, bw, -1, 128), n_edge), 2)[:, :, 0, :]
        assert (rec["n_edge"], rec["n_fft"]) == (n_edge, 128)
        _same_bits(np.ascontiguousarray(rec["data"]).view(np.uint32).reshape(-1), want, ("second run", cut["t0"]))
