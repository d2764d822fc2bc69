"""GPU tests (-m gpu) of Faraday synthesis (include/dsabf.h: bf_rm_*; docs/FARADAY.md).  The reference is tests/support/rm_oracle.py:
the fixed float32 operation order in numpy, with the fused multiply-add emulated exactly.  Outputs are sentinel-filled with guard
cells behind them and compared whole and BIT FOR BIT (as uint32 words, the integer fields of the records included).

Every test is ONE function that loops over its cases, as tests/test_gpu_cdd.py does: none of the cases may be thinned out."""
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

SUPPORT = os.path.join(ROOT, "tests", "support")
sys.path.insert(0, SUPPORT)
import cdd_oracle as co  # noqa: E402
import rm_oracle as ro  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
SENTINEL = -0x3EDCBA99          # as int32: a NaN pattern no arithmetic here produces
GUARD = 8                       # float32 words behind every output


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
    """The synthesis takes nothing from the handle's geometry: one small handle serves every test of it."""
    bf = bfmod.Beamformer(bfmod.debug_config(n_ant=4, n_pol=2, n_avg=1, n_beams=4, n_freq=1, n_out_per_gemm=1, n_gemms_per_block=4,
                                             n_blocks_on_gpu=2, n_streams=4))
    yield bf
    bf.close()


def _sentinels(torch, n_words, shift_words=0):
    buf = torch.full((shift_words + n_words + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[shift_words:]


def _words(buf, n_words, shift_words=0):
    got = buf.cpu().numpy()
    assert (got[:shift_words] == SENTINEL).all() and (got[shift_words + n_words:] == SENTINEL).all(), "a guard word was written"
    return got[shift_words:shift_words + n_words].view(np.uint32)


def _same_bits(got_words, want, case):
    want_words = np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    assert got_words.shape == want_words.shape, (case, got_words.shape, want_words.shape)
    bad = np.flatnonzero(got_words != want_words)
    assert bad.size == 0, (case, len(bad), bad[:4], got_words[bad[:4]], want_words[bad[:4]])


def _upload(torch, a, shift_words):
    """a float32 array on the device behind shift_words spare words (2: an address that is 8-byte aligned only)."""
    flat = np.ascontiguousarray(a, np.float32).reshape(-1)
    d = torch.zeros(flat.size + 4, dtype=torch.float32, device="cuda")
    d[shift_words:shift_words + flat.size] = torch.from_numpy(flat).cuda()
    return d, d[shift_words:]


def _run(torch, stage, s, base, want, case, mode, shift=0, stream=0):
    """mode 'spec', 'peaks' or 'both'; shift 0 or 2 words on the input, the baseline and both outputs.  Returns the peak words."""
    want_spec, want_peaks = want
    n_rows, _, K, _ = s.shape
    keep_s, d_s = _upload(torch, s, shift)
    keep_b, d_b = _upload(torch, base, shift) if base is not None else (None, None)
    assert d_s.data_ptr() % 16 == (8 if shift else 0)
    sbuf, sview = _sentinels(torch, 2 * want_spec.size, shift)
    pbuf, pview = _sentinels(torch, 8 * want_peaks.size, shift)
    stage.run(d_s, K, n_rows, base=d_b, spec=sview if mode != "peaks" else None, peaks=pview if mode != "spec" else None, stream=stream)
    torch.cuda.synchronize()
    if mode == "peaks":
        _words(sbuf, 0, 0)
    else:
        _same_bits(_words(sbuf, 2 * want_spec.size, shift), want_spec, (case, mode, shift, "spectrum"))
    if mode == "spec":
        _words(pbuf, 0, 0)
        return None
    got = _words(pbuf, 8 * want_peaks.size, shift)
    _same_bits(got, want_peaks, (case, mode, shift, "peaks"))
    return got


def _c64(re, im):
    out = np.empty(np.shape(re), np.complex64)
    out.real, out.imag = re, im
    return out


def _random_table(rng, n_phi, n_chan):
    """Any table is legal: unit-modulus entries of random phase scaled by wn = 1 / n_chan."""
    a = rng.uniform(0, 2 * np.pi, size=(n_phi, n_chan))
    return _c64((np.cos(a) / n_chan).astype(np.float32), (np.sin(a) / n_chan).astype(np.float32)), np.full(n_chan, 1.0 / n_chan, np.float32)


# (n_rows, K, n_phi, n_chan): pairs n_rows K = 1, 31, 32, 33, 100 and their neighbours at K = 3 and 16; the tile edges of the depths
# (15, 16, 17, 33), one whole pass (512), one depth beyond it and three passes; the chunk edges of the channels (64, 256, 257)
SHAPES = [(1, 1, 1, 1), (31, 1, 2, 2), (32, 1, 15, 3), (33, 1, 16, 64), (100, 1, 17, 256), (11, 3, 33, 257), (1, 3, 512, 3), (2, 16, 513, 64),
          (7, 16, 33, 2), (1, 16, 1100, 65), (34, 3, 512, 257), (100, 1, 1, 64), (33, 1, 2, 1)]


def test_every_shape_to_the_bit(torch, bfmod, handle):
    """Gaussian cells on every shape, with and without a baseline, spectrum only, peaks only and both, on 16- and 8-byte addresses;
    the records of the peaks-only launch and of the launch that also writes the spectrum are the same words."""
    from dsabeamformer_amd import api

    assert {r * k for r, k, _, _ in SHAPES} >= {1, 31, 32, 33, 100} and {k for _, k, _, _ in SHAPES} == {1, 3, 16}
    assert {p for _, _, p, _ in SHAPES} >= {1, 2, 15, 16, 17, 33, 512} and {c for _, _, _, c in SHAPES} >= {1, 2, 3, 64, 256, 257}
    rng = np.random.default_rng(20261101)
    t0, n_words = time.perf_counter(), 0
    for turn, (n_rows, K, n_phi, n_chan) in enumerate(SHAPES):
        rot, wn = _random_table(rng, n_phi, n_chan)
        stage = api.FaradaySynthesis(handle, n_chan, n_phi, rot, wn)
        s = rng.standard_normal((n_rows, n_chan, K, 4)).astype(np.float32)
        base = rng.standard_normal((n_chan, K, 4)).astype(np.float32)
        for b in (None, base):
            want = ro.synthesize(s, rot, wn, b)
            assert want[0].shape == (n_rows, K, n_phi) and want[1].shape == (n_rows, K) and np.isfinite(want[0].view(np.float32)).all()
            case = (n_rows, K, n_phi, n_chan, b is not None)
            both = _run(torch, stage, s, b, want, case, "both", 0)
            only = _run(torch, stage, s, b, want, case, "peaks", 0)
            assert np.array_equal(both, only), case
            _run(torch, stage, s, b, want, case, "spec", 0)
            _run(torch, stage, s, b, want, case, "spec", 2)
            _run(torch, stage, s, b, want, case, ("both", "peaks")[turn % 2], 2)
            n_words += 4 * want[0].size
        stage.close()
    print("rm_kernel: %d shapes, %d spectrum words compared, %.1f s" % (len(SHAPES), n_words, time.perf_counter() - t0))


def test_data_edges_to_the_bit(torch, bfmod, handle):
    """Full-scale cells (to 2^40, what bf_cdd_stokes_device yields); a row of zeros (p = 0, a +0 spectrum); two equal maxima in two
    tiles, two waves' tiles and two passes (the first wins); the peak at p = 0, n_phi - 1 and on both sides of every pass seam (the
    neighbours come from the other pass); products in the subnormal range (nothing is flushed)."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(20261102)
    n_rows, K, n_chan = 5, 3, 67
    for n_phi in (40, 1100):
        rot, wn = _random_table(rng, n_phi, n_chan)
        # full scale
        s = (rng.integers(-2 ** 40, 2 ** 40, size=(n_rows, n_chan, K, 4)).astype(np.float32))
        s[..., 0] = np.abs(s[..., 0])
        base = rng.integers(-2 ** 30, 2 ** 30, size=(n_chan, K, 4)).astype(np.float32)
        stage = api.FaradaySynthesis(handle, n_chan, n_phi, rot, wn)
        for mode in ("both", "peaks"):
            _run(torch, stage, s, base, ro.synthesize(s, rot, wn, base), ("full scale", n_phi), mode)
        # a row of zeros among Gaussian rows
        s = rng.standard_normal((n_rows, n_chan, K, 4)).astype(np.float32)
        s[2] = 0
        want = ro.synthesize(s, rot, wn)
        assert (want[1][2]["p"] == 0).all() and (want[0][2].view(np.uint32) == 0).all() and (want[1][2]["pow_pk"] == 0).all()
        for mode in ("both", "peaks"):
            _run(torch, stage, s, None, want, ("zero row", n_phi), mode)
        live = np.ones(n_rows, bool)
        live[2] = False
        # a forced peak: the table row of that depth is 1024 times as large, so its power is about 10^6 times the others'
        forced = [0, n_phi - 1, 17, 31, 32] + ([511, 512, 1023, 1024, 1099] if n_phi > 512 else [])
        for p in forced:
            t = rot.copy()
            t[p] *= np.float32(1024)
            stage.set_table(t, wn)
            want = ro.synthesize(s, t, wn)
            assert (want[1][live]["p"] == p).all(), p
            if 0 < p < n_phi - 1:
                assert (want[1][live]["pow_lo"] > 0).all() and (want[1][live]["pow_hi"] > 0).all()
            for mode in ("both", "peaks"):
                _run(torch, stage, s, None, want, ("peak at", p, n_phi), mode)
        # two equal maxima: identical table rows give identical spectra to the bit
        pairs = [(5, 37), (3, 35), (0, n_phi - 1)] + ([(3, 3 + 128), (40, 40 + 32), (500, 700), (511, 512), (100, 1099)] if n_phi > 512 else [])
        for p1, p2 in pairs:
            t = rot.copy()
            t[p1] *= np.float32(1024)
            t[p2] = t[p1]
            stage.set_table(t, wn)
            want = ro.synthesize(s, t, wn)
            assert (want[1][live]["p"] == p1).all() and np.array_equal(want[0][live][..., p1].copy().view(np.uint32), want[0][live][..., p2].copy().view(np.uint32))
            for mode in ("both", "peaks"):
                _run(torch, stage, s, None, want, ("equal maxima", p1, p2, n_phi), mode)
        # subnormal products: cells near 2^-70 against a table near 2^-70 / n_chan
        tiny = _c64(rot.real * np.float32(2.0 ** -64), rot.imag * np.float32(2.0 ** -64))
        s_small = (rng.standard_normal((n_rows, n_chan, K, 4)) * 2.0 ** -70).astype(np.float32)
        want = ro.synthesize(s_small, tiny, wn)
        words = want[0].view(np.uint32)
        assert ((words & 0x7F800000) == 0).all() and ((words & 0x007FFFFF) != 0).mean() > 0.9, "the case is meant to be subnormal and non-zero"
        stage.set_table(tiny, wn)
        for mode in ("both", "spec"):
            _run(torch, stage, s_small, None, want, ("subnormal", n_phi), mode)
        stage.close()


def test_stokes_to_synthesis_on_one_stream(torch, bfmod, handle):
    """CoherentDedisperser.stokes -> FaradaySynthesis.run on one stream with nothing synchronised in between equals the two oracles
    chained; the Stokes output is placed on an address that is 8-byte aligned only."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(20261103)
    n_chan, K, n_fft, n_edge, n_time, n_int, n_phi = 3, 3, 64, 8, 96, 4, 33
    phi = rng.uniform(0, 2 * np.pi, size=(n_chan, n_fft))
    chirp = _c64((np.cos(phi) / n_fft).astype(np.float32), (np.sin(phi) / n_fft).astype(np.float32))
    x = _c64(rng.integers(-2 ** 19, 2 ** 19 + 1, size=(n_chan, K, 2, n_time)).astype(np.float32),
             rng.integers(-2 ** 19, 2 ** 19 + 1, size=(n_chan, K, 2, n_time)).astype(np.float32))
    stokes = co.stokes(co.dedisperse(x, chirp, n_edge), n_int)
    n_rows = n_time // n_int
    rot, wn = _random_table(rng, n_phi, n_chan)
    want_spec, want_peaks = ro.synthesize(stokes, rot, wn)
    cdd = api.CoherentDedisperser(handle, n_chan, n_fft, n_edge, chirp)
    rm = api.FaradaySynthesis(handle, n_chan, n_phi, rot, wn)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    d_stokes = torch.zeros(stokes.size + 4, dtype=torch.float32, device="cuda")[2:]
    sbuf, sview = _sentinels(torch, 2 * want_spec.size)
    pbuf, pview = _sentinels(torch, 8 * want_peaks.size)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    cdd.stokes(d_x, K, n_time, n_int, d_stokes, st.cuda_stream)
    rm.run(d_stokes, K, n_rows, spec=sview, peaks=pview, stream=st.cuda_stream)
    st.synchronize()
    _same_bits(_words(sbuf, 2 * want_spec.size), want_spec, "the chain's spectrum")
    _same_bits(_words(pbuf, 8 * want_peaks.size), want_peaks, "the chain's peaks")
    rm.close()
    cdd.close()


def test_an_injected_rm_comes_back(torch, bfmod, handle):
    """256 channels over 1.28 ... 1.53 GHz, Q + i U = L exp(2 i (chi0 + RM lambda^2)) on a unit intensity, a grid of fwhm / 8: through
    the device and rm_refine the rotation measure comes back within dphi / 2, the angle within what that subtends, the fraction L / I."""
    from dsabeamformer_amd import api

    freq = np.linspace(1.28, 1.53, 256)
    w = np.ones(256)
    fwhm, _ = api.rm_resolution(freq, w)
    dphi, n_phi, L, chi0 = fwhm / 8, 512, 0.4, 0.3
    l2 = ro.lambda2(freq)
    rms = [-2000.0, -37.5, 0.0, 410.0, 1500.0]
    for rm_true in rms:
        phi0 = np.round(rm_true / dphi) * dphi - 200.3 * dphi                   # (the grid does not contain RM exactly)
        rot, wn, l0 = api.rm_table(freq, w, phi0, dphi, n_phi)
        pol = L * np.exp(2j * (chi0 + rm_true * l2))
        s = np.zeros((4, 256, 2, 4), np.float32)
        s[..., 0], s[..., 1], s[..., 2] = 1.0, pol.real[None, :, None], pol.imag[None, :, None]
        stage = api.FaradaySynthesis(handle, 256, n_phi, rot, wn)
        want = ro.synthesize(s, rot, wn)
        got = _run(torch, stage, s, None, want, ("injected", rm_true), "peaks")
        fits = api.rm_refine(got.view(api.rm_peak_dtype()).reshape(4, 2), phi0, dphi, n_phi, l0)
        err = np.abs(fits["rm"] - rm_true).max()
        pa_err = np.abs((fits["pa"] - chi0 + np.pi / 2) % np.pi - np.pi / 2).max()
        print("RM %8.1f: |rm - RM| = %.4f = %.4f dphi, |pa - chi0| = %.2e rad, frac %.6f" % (rm_true, err, err / dphi, pa_err, fits["frac"].max()))
        assert err <= dphi / 2 and pa_err <= dphi / 2 * l0, (rm_true, err, pa_err)
        # the record holds the power AT the grid point, at most dphi / 2 from RM: the fraction is L |RMSF(offset)|, between L |RMSF(dphi / 2)|
        # and L (1e-5: the float32 chain, section 2's bound at 256 channels is 3e-5 of the sum of moduli and is met to a few per cent)
        floor = L * abs(api.rm_rmsf(freq, w, dphi / 2, dphi, 1)[0])
        assert (fits["frac"] >= floor * (1 - 1e-5)).all() and (fits["frac"] <= L * (1 + 1e-5)).all(), (rm_true, fits["frac"], floor)
        stage.close()


def test_set_table_is_ordered(torch, bfmod, handle):
    """A kernel queued behind a busy stream, set_table with another table, then a second kernel: each result matches its own table --
    the upload waits for the first kernel, the second kernel for the upload."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(20261104)
    n_rows, K, n_chan, n_phi = 40, 3, 64, 100
    (ta, wa), (tb, wb) = _random_table(rng, n_phi, n_chan), _random_table(rng, n_phi, n_chan)
    wb = (wb * np.float32(0.5)).astype(np.float32)
    s = rng.standard_normal((n_rows, n_chan, K, 4)).astype(np.float32)
    want_a, want_b = ro.synthesize(s, ta, wa), ro.synthesize(s, tb, wb)
    assert not np.array_equal(want_a[0], want_b[0]) and not np.array_equal(want_a[1]["isum"], want_b[1]["isum"])
    stage = api.FaradaySynthesis(handle, n_chan, n_phi, ta, wa)
    d_s = torch.from_numpy(s).cuda()
    bufs = [(_sentinels(torch, 2 * want_a[0].size), _sentinels(torch, 8 * want_a[1].size)) for _ in range(2)]
    big = torch.randn((8192, 8192), device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            torch.mm(big, big)
    stage.run(d_s, K, n_rows, spec=bufs[0][0][1], peaks=bufs[0][1][1], stream=s1.cuda_stream)   # runs when s1 gets to it, with table A
    stage.set_table(tb, wb)                                                                      # must not land under that kernel
    stage.run(d_s, K, n_rows, spec=bufs[1][0][1], peaks=bufs[1][1][1], stream=s2.cuda_stream)
    torch.cuda.synchronize()
    for (sb, pb), want, name in ((bufs[0], want_a, "before set_table"), (bufs[1], want_b, "after set_table")):
        _same_bits(_words(sb[0], 2 * want[0].size), want[0], "the spectrum of the kernel " + name)
        _same_bits(_words(pb[0], 8 * want[1].size), want[1], "the peaks of the kernel " + name)
    stage.close()


def test_refusals_and_lifetime(torch, bfmod):
    """Every BF_ERR_INVALID / BF_ERR_STATE with the outputs' sentinels intact, then the handle destroyed first."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(20261105)

    def refused(code, call):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == code and str(e.value), (e.value.code, str(e.value))

    bf = bfmod.Beamformer(bfmod.debug_config(n_ant=4, n_pol=2, n_avg=1, n_beams=4, n_freq=1, n_out_per_gemm=1, n_gemms_per_block=4,
                                             n_blocks_on_gpu=2, n_streams=4))
    n_rows, K, n_chan, n_phi = 5, 3, 6, 20
    rot, wn = _random_table(rng, n_phi, n_chan)
    for bad in (0, -1, 4097):
        refused(BF_ERR_INVALID, lambda: api.FaradaySynthesis(bf, bad, n_phi, np.zeros((n_phi, max(bad, 1)), np.complex64), np.zeros(max(bad, 1), np.float32)))
        refused(BF_ERR_INVALID, lambda: api.FaradaySynthesis(bf, n_chan, bad, np.zeros((max(bad, 1), n_chan), np.complex64), wn))
    refused(BF_ERR_INVALID, lambda: api.FaradaySynthesis(bf, n_chan, n_phi, None, wn))
    refused(BF_ERR_INVALID, lambda: api.FaradaySynthesis(bf, n_chan, n_phi, rot, None))
    lib = bf._lib
    out = api.C.c_void_p()
    assert lib.bf_rm_create(None, n_chan, n_phi, rot.ctypes.data, wn.ctypes.data, api.C.byref(out)) == BF_ERR_INVALID and not out.value
    assert lib.bf_rm_device(None, None, 1, 1, None, None, None, None) == BF_ERR_INVALID and lib.bf_rm_set_table(None, None, None) == BF_ERR_INVALID
    assert lib.bf_rm_destroy(None) == 0
    stage = api.FaradaySynthesis(bf, n_chan, n_phi, rot, wn)
    s = rng.standard_normal((n_rows, n_chan, K, 4)).astype(np.float32)
    base = rng.standard_normal((n_chan, K, 4)).astype(np.float32)
    d_s, d_b = torch.from_numpy(s).cuda(), torch.from_numpy(base).cuda()
    sbuf, sview = _sentinels(torch, 2 * n_rows * K * n_phi)
    pbuf, pview = _sentinels(torch, 8 * n_rows * K)
    calls = [lambda: stage.run(None, K, n_rows, spec=sview, peaks=pview), lambda: stage.run(d_s, K, n_rows),
             lambda: stage.run(d_s, 0, n_rows, spec=sview, peaks=pview), lambda: stage.run(d_s, -3, n_rows, spec=sview, peaks=pview),
             lambda: stage.run(d_s, K, 0, spec=sview, peaks=pview), lambda: stage.run(d_s, K, -1, spec=sview, peaks=pview),
             lambda: stage.run(d_s, K, (2 ** 31 + K - 1) // K, spec=sview, peaks=pview),          # n_rows K >= 2^31
             lambda: stage.run(d_s, 2 ** 16, 2 ** 15, spec=sview, peaks=pview),
             lambda: stage.run(d_s.data_ptr() + 4, K, n_rows, spec=sview, peaks=pview),
             lambda: stage.run(d_s, K, n_rows, base=d_b.data_ptr() + 4, spec=sview, peaks=pview),
             lambda: stage.run(d_s, K, n_rows, spec=sview.data_ptr() + 4, peaks=pview),
             lambda: stage.run(d_s, K, n_rows, spec=sview, peaks=pview.data_ptr() + 4),
             lambda: stage.run(d_s, K, n_rows, peaks=pview.data_ptr() + 12),
             lambda: stage.set_table(None, wn), lambda: stage.set_table(rot, None)]
    for call in calls:
        refused(BF_ERR_INVALID, call)
    torch.cuda.synchronize()
    _words(sbuf, 0)
    _words(pbuf, 0)                                                              # every word is still the sentinel
    before = torch.cuda.current_device()
    want = ro.synthesize(s, rot, wn, base)
    _run(torch, stage, s, base, want, "after the refusals", "both")              # and the stage still works
    assert torch.cuda.current_device() == before
    bf.close()                                                                   # the handle first
    for call in (lambda: stage.run(d_s, K, n_rows, spec=sview, peaks=pview), lambda: stage.set_table(rot, wn)):
        refused(BF_ERR_STATE, call)
    stage.close()


def test_beam_faraday_mode(bfmod, tmp_path):
    """`beam -j 33 ... --voltages v.bin` and `beam --coherent v.bin --coherent-out c.bin` as in tests/test_gpu_cdd.py, then `beam --faraday
    c.bin --faraday-out f.bin` twice -- the default grid and window, then an explicit grid with a window and a channel mask: every record of
    both files equals the oracle chain over ITS coherent record (rm_oracle.faraday_record and api.rm_refine of row 0), there is at least one
    record, and the earlier files are the same bytes afterwards.  On the explicit grid (129 depths) every row of every record is compared;
    on the default grid (1981 depths, 7 s of numpy per record with all rows) row 0's whole spectrum, and the peak records of row 0, the
    window's rows and their neighbours, the first and last row and every 16th (rm_oracle.sparse_rows).  A truncated input is refused and leaves no file."""
    import subprocess

    from dsabeamformer_amd import api, build, host

    names = ("det.bin", "dm.bin", "cands.txt", "ev.txt", "v.bin", "c.bin", "f.bin", "f2.bin", "mask.txt")
    det_file, dm_file, cand_file, ev_file, v_file, c_file, f_file, f2_file, mask_file = (str(tmp_path / n) for n in names)
    base = [build.BEAM, "-j", "33", "-M", "250", "-N", "8", "-S", "4", "-B", "6", "-i", "255"]
    r = subprocess.run(base + ["-w", det_file, "-W", dm_file, "-C", cand_file, "--events", ev_file, "--voltages", v_file, "--voltage-units", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    r = subprocess.run([build.BEAM, "--coherent", v_file, "--coherent-out", c_file, "-M", "250", "-N", "8", "--coherent-int", "2"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    earlier = {f: open(f, "rb").read() for f in (det_file, dm_file, cand_file, ev_file, v_file, c_file)}
    chdr, crecs = host.read_coherent_file(c_file)
    n_chan, first, n_rows = int(chdr["NFREQ"]), int(chdr["FIRST_CHANNEL"]), int(chdr["NTIME"]) // int(chdr["NINT"])
    assert len(crecs) >= 1 and (n_chan, n_rows, chdr["NINT"], chdr["NAVG"]) == (256, 128, "2", "16")
    freq = [float(np.float32(host.channel_frequency(0, first + ch))) for ch in range(n_chan)]
    masked = [5, 100, 255]
    open(mask_file, "w").write("# masked channels\n" + "".join("%d\n" % c for c in masked))

    def check(path, extra, w, grid, window, rows):
        r = subprocess.run([build.BEAM, "--faraday", c_file, "--faraday-out", path] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr
        phi0, dphi, n_phi = grid
        rot, wn, l0 = api.rm_table(freq, w, phi0, dphi, n_phi)
        fwhm, phi_max = api.rm_resolution(freq, w)
        hdr, recs = host.read_faraday_file(path)
        assert (hdr["CONTENT"], hdr["NFREQ"], hdr["FIRST_CHANNEL"], hdr["NROWS"], hdr["NPHI"]) == ("faraday", str(n_chan), str(first), str(n_rows), str(n_phi))
        assert [float(hdr[k]) for k in ("PHI0", "DPHI", "LAMBDA0_2", "FWHM", "PHI_MAX")] == [phi0, dphi, l0, fwhm, phi_max]
        kept = 0
        for c in crecs:
            win = window or max(1, c["width"] * 16 // 2)                               # the search width in rows of the file: NAVG / NINT each
            want = ro.faraday_record(c["data"], win, rot, wn, rows)
            if want is None:
                continue
            rec = recs[kept]
            kept += 1
            lo, spec, peaks = want
            assert all(rec[k] == c[k] for k in ("t0", "dm", "beam", "width", "snr", "dm_value", "n_edge", "n_fft")) and (rec["lo"], rec["w"]) == (lo, min(win, n_rows))
            _same_bits(np.ascontiguousarray(rec["spec"]).view(np.uint32), spec, (path, c["t0"], "spectrum"))
            got_peaks = rec["peaks"] if rows is None else rec["peaks"][rows(lo, min(win, n_rows), n_rows)]
            assert len(got_peaks) == len(peaks) >= (1 + n_rows if rows is None else 10)
            _same_bits(np.frombuffer(got_peaks.tobytes(), np.uint32), np.frombuffer(peaks.tobytes(), np.uint32), (path, c["t0"], "peaks"))
            fit = api.rm_refine(peaks[:1], phi0, dphi, n_phi, l0)[0]
            assert (rec["rm"], rec["pa"], rec["lin"], rec["frac"]) == (fit["rm"], fit["pa"], fit["lin"], fit["frac"])
        assert kept == len(recs) >= 1
        assert "Faraday synthesis: %d of %d records of %d rows x %d channels on %d depths" % (kept, len(crecs), n_rows, n_chan, n_phi) in r.stdout, r.stdout[-1500:]
        assert "left out: %d with fewer than 8 baseline rows" % (len(crecs) - kept) in r.stdout and "Wrote %d Faraday records" % kept in r.stdout

    ones = np.ones(n_chan)
    check(f_file, [], ones, ro.default_grid(freq, ones), 0, ro.sparse_rows)
    w = ones.copy()
    w[masked] = 0
    check(f2_file, ["--faraday-phi", "-300:340:129", "--faraday-window", "3", "-F", mask_file], w, (-300.0, 5.0, 129), 3, None)
    for f, data in earlier.items():
        assert open(f, "rb").read() == data, f
    # a truncated input is refused before the device is touched, and no output file appears
    cut_file, f3_file = str(tmp_path / "c_short.bin"), str(tmp_path / "f3.bin")
    open(cut_file, "wb").write(earlier[c_file][:-100])
    r = subprocess.run([build.BEAM, "--faraday", cut_file, "--faraday-out", f3_file, "--faraday-phi", "-300:340:129"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "does not end with a whole record" in r.stderr and not r.stdout and not os.path.exists(f3_file), (r.returncode, r.stderr)
