"""CPU checks of coherent dedispersion (docs/COHERENT_DEDISPERSION.md): the float32 oracle of the fixed operation order against a
complex128 restatement on numpy.fft at a bound derived from the error analysis of the FFT; the physics in float64 (a dispersed impulse
comes back into one sample); the host helpers against their formulas and known answers; the exports' error convention without a handle
or stage; the Python surface.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cdd_oracle as co  # noqa: E402

BF_ERR_INVALID = -1
BW = 250.0 / 2048                                                                # MHz: one channel; a sample is 1 / BW = 8.192 us


def _lib():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import build as b

    b.build()
    return l.load()


def test_float32_order_against_fp64_within_the_derived_bound():
    """Per segment, the relative 2-norm error of the float32 oracle is at most (14 log2 N + 4) 2^-24: Higham, Accuracy and Stability of
    Numerical Algorithms, Thm 24.2, gives m eta per radix-2 transform of length 2^m with eta about 6.7 u for correctly rounded
    twiddles; there are two transforms, plus 4 u for the rounded table and the complex multiply.  Full-scale integer input (|re|,
    |im| <= 2^19, what bf_stokes_voltages_device writes), a chirp row and random rows, with and without an edge."""
    rng = np.random.default_rng(11)
    for n in (64, 128, 256, 512, 1024, 2048, 4096):
        bound = (14 * np.log2(n) + 4) * 2.0 ** -24
        for n_edge, n_time in ((0, 3 * n), (n // 4, 2 * n + 5), (3, n - 7)):
            shape = (2, 2, 2, n_time)
            x = np.empty(shape, np.complex64)
            x.real, x.imag = rng.integers(-2 ** 19, 2 ** 19 + 1, size=shape), rng.integers(-2 ** 19, 2 ** 19 + 1, size=shape)
            phi = rng.uniform(0, 2 * np.pi, n)
            table = np.stack([co.chirp(500.0, [1.28], BW, 1, n)[0], (np.exp(1j * phi) / n).astype(np.complex64)])
            seg = co.segments(x, n, n_edge)
            assert seg.shape == shape[:3] + (co.n_segments(n_time, n, n_edge), n)
            got = co.filter_segments(seg, table).astype(np.complex128)
            want = np.fft.ifft(np.fft.fft(seg.astype(np.complex128), axis=-1) * table.astype(np.complex128)[:, None, None, None], axis=-1) * n
            err = np.linalg.norm((got - want).reshape(-1, n), axis=1) / np.linalg.norm(want.reshape(-1, n), axis=1)
            assert err.max() <= bound, (n, n_edge, err.max() * 2 ** 24, bound * 2 ** 24)
            assert err.max() > 0                                                 # (float32 really was used)
            # and the two whole-series forms agree with their segments
            a, b = co.dedisperse(x, table, n_edge), co.dedisperse64(x, table, n_edge)
            assert a.shape == b.shape == shape and a.dtype == np.complex64
            assert np.abs(a - b).max() <= 8 * bound * np.abs(b).max()


def test_the_oracle_is_a_convolution():
    """Overlap-save with a table whose impulse response fits the edge is the circular convolution of the whole series cut to it: a
    delay of 3 samples (a linear phase) with n_edge = 3 shifts the series, zeros coming in at the start -- seams included."""
    n, n_edge, n_time = 64, 3, 300
    rng = np.random.default_rng(2)
    x = (rng.integers(-99, 100, size=(1, 1, 2, n_time)) + 1j * rng.integers(-99, 100, size=(1, 1, 2, n_time))).astype(np.complex64)
    j = np.arange(n)
    table = (np.exp(-2j * np.pi * 3 * j / n) / n)[None]
    y = co.dedisperse64(x, table, n_edge)
    want = np.concatenate([np.zeros((1, 1, 2, 3)), x[..., :-3]], axis=-1)
    assert np.abs(y - want).max() < 1e-9
    y32 = co.dedisperse(x, table.astype(np.complex64), n_edge)
    assert np.abs(y32 - want).max() < 1e-3


CASES = [(500.0, 1.28, 256), (3000.0, 1.28, 1024), (500.0, 1.4, 128), (100.0, 1.53, 64), (1000.0, 1.28, 256)]


def test_a_dispersed_impulse_comes_back_into_its_sample():
    """Physics, float64 only: an impulse dispersed by ONE transform of 8192 samples with the conjugate chirp is dedispersed by the
    segment algorithm with bf_cdd_edge's edge, at every 1 / 64 of one V: at least 0.99 of the output energy lies in the impulse's
    sample in all five cases (measured 0.9990 ... 0.9999); without dedispersion it is 0.065 at DM 500."""
    fractions = []
    for dm, f, n in CASES:
        n_edge = co.edge(dm, [f], BW)
        assert 0 < n_edge <= n // 4
        v = n - 2 * n_edge
        table = co.chirp64(dm, [f], BW, 1, n)
        worst = 1.0
        for i in range(64):
            at = 3000 + (i * v) // 64
            d = co.dispersed_impulse(dm, f, BW, 1, at)
            p = np.abs(co.dedisperse64(d.reshape(1, 1, 1, -1), table, n_edge)[0, 0, 0]) ** 2
            assert int(np.argmax(p)) == at
            worst = min(worst, p[at] / p.sum())
        fractions.append(worst)
        assert worst >= 0.99, (dm, f, n, worst)
    d = np.abs(co.dispersed_impulse(500.0, 1.4, BW, 1, 3000)) ** 2
    assert d.max() / d.sum() < 0.07
    print("smallest fractions:", ["%.4f" % w for w in fractions])


def test_sweep_and_edge_known_answers():
    lib = _lib()
    from dsabeamformer_amd import api

    for dm, f, sweep, edge in ((500.0, 1.4, 22.5, 23), (500.0, 1.28, 29.5, 30), (3000.0, 1.28, 176.9, 177)):
        got = lib.bf_cdd_sweep_samples(dm, f, BW)
        assert abs(got - sweep) < 0.05 and got == api.cdd_sweep_samples(dm, f, BW), (dm, f, got)
        assert abs(got - co.sweep_samples(dm, f, BW)) <= 1e-12 * got
        assert api.cdd_edge(dm, [f], BW) == edge == co.edge(dm, [f], BW)
    freqs = [1.53, 1.4, 1.28, 1.35]                                              # the largest sweep is at the lowest frequency, wherever it stands
    assert api.cdd_edge(500.0, freqs, BW) == 30 and api.cdd_edge(0.0, freqs, BW) == 0
    arr = (C.c_double * 4)(*freqs)
    assert lib.bf_cdd_edge(500.0, arr, 4, BW) == 30
    assert lib.bf_cdd_edge(500.0, None, 4, BW) == BF_ERR_INVALID and lib.bf_last_error()
    assert lib.bf_cdd_edge(500.0, arr, 0, BW) == BF_ERR_INVALID


def test_chirp_table_against_the_formula():
    from dsabeamformer_amd import api

    freqs = [1.28, 1.4, 1.53]
    for n in (64, 256, 4096):
        for dm in (0.0, 100.0, 3000.0):
            got, want = api.cdd_chirp(dm, freqs, BW, 1, n), co.chirp(dm, freqs, BW, 1, n)
            assert got.shape == want.shape == (3, n) and got.dtype == np.complex64
            for g, w in ((got.real, want.real), (got.imag, want.imag)):          # one unit in the last place: two libms may differ in
                ulp = np.maximum(np.spacing(np.abs(g)), np.spacing(np.abs(w)))  # the last bit of a double
                assert (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= ulp).all(), (n, dm)
            assert np.abs(np.abs(got.astype(np.complex128)) * n - 1).max() <= 2.0 ** -23, (n, dm)
            if dm == 0.0:
                assert (got == np.complex64(1.0 / n)).all()
            minus = api.cdd_chirp(dm, freqs, BW, -1, n)
            j = np.arange(n)
            keep = j != n // 2                                                   # (bin n / 2 is nu = -bw / 2 for one sideband, +bw / 2 for the other)
            reversed_bins = np.ascontiguousarray(got[:, (n - j) % n][:, keep])
            assert np.array_equal(np.ascontiguousarray(minus[:, keep]).view(np.uint32), reversed_bins.view(np.uint32)), (n, dm)
    lib = _lib()
    one = (C.c_double * 1)(1.28)
    out = np.zeros(128, np.float32)
    bad = [lambda: lib.bf_cdd_chirp(1.0, None, 1, BW, 1, 64, out.ctypes.data), lambda: lib.bf_cdd_chirp(1.0, one, 1, BW, 1, 64, None),
           lambda: lib.bf_cdd_chirp(1.0, one, 0, BW, 1, 64, out.ctypes.data), lambda: lib.bf_cdd_chirp(1.0, one, 1, BW, 0, 64, out.ctypes.data),
           lambda: lib.bf_cdd_chirp(1.0, one, 1, BW, 2, 64, out.ctypes.data), lambda: lib.bf_cdd_chirp(1.0, one, 1, BW, 1, 96, out.ctypes.data),
           lambda: lib.bf_cdd_chirp(1.0, one, 1, BW, 1, 32, out.ctypes.data), lambda: lib.bf_cdd_chirp(1.0, one, 1, BW, 1, 8192, out.ctypes.data)]
    for i, call in enumerate(bad):
        assert call() == BF_ERR_INVALID and lib.bf_last_error(), i
    assert not out.any()


def test_every_new_export_refuses_a_null_handle_or_stage():
    lib = _lib()
    out = C.c_void_p()
    table = np.zeros(128, np.float32)
    calls = [lambda: lib.bf_cdd_create(None, 1, 64, 0, table.ctypes.data, C.byref(out)),
             lambda: lib.bf_cdd_create(None, 1, 64, 0, table.ctypes.data, None),
             lambda: lib.bf_cdd_set_chirp(None, table.ctypes.data),
             lambda: lib.bf_cdd_voltages_device(None, None, 1, 1, None, None),
             lambda: lib.bf_cdd_stokes_device(None, None, 1, 1, 1, None, None),
             lambda: lib.bf_stokes_voltages_device(None, None, 1, None, None)]
    for i, call in enumerate(calls):
        assert call() == BF_ERR_INVALID and lib.bf_last_error(), i
    assert out.value is None
    assert lib.bf_cdd_destroy(None) == 0                                         # like free(): nothing to destroy
    assert lib.bf_stokes_voltage_entries(None, 4) == 0


def test_voltage_entries():
    from dsabeamformer_amd import api

    lib = _lib()
    c3 = api.production_config()
    assert lib.bf_stokes_voltage_entries(C.byref(c3), 4) == 256 * 4 * 2 * 128    # 128 units of it: the 512 MiB of the measurements
    assert lib.bf_stokes_voltage_entries(C.byref(c3), 16) == 256 * 16 * 2 * 128
    for k in (0, -1, 17):
        assert lib.bf_stokes_voltage_entries(C.byref(c3), k) == 0
    assert lib.bf_stokes_voltage_entries(C.byref(api.production_config(n_pol=1)), 4) == 0


def test_python_surface_and_signature_table():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import api

    names = ["bf_stokes_voltage_entries", "bf_stokes_voltages_device", "bf_cdd_sweep_samples", "bf_cdd_edge", "bf_cdd_chirp", "bf_cdd_create",
             "bf_cdd_destroy", "bf_cdd_set_chirp", "bf_cdd_voltages_device", "bf_cdd_stokes_device"]
    assert all(n in l.SIGNATURES for n in names)
    assert l.SIGNATURES["bf_cdd_sweep_samples"] == (C.c_double, [C.c_double] * 3)
    assert l.SIGNATURES["bf_cdd_voltages_device"][1][3] is C.c_int64 and l.SIGNATURES["bf_cdd_stokes_device"][1][3] is C.c_int64
    assert l.SIGNATURES["bf_stokes_voltage_entries"][0] is C.c_size_t
    for member in ("set_chirp", "voltages", "stokes", "close"):
        assert callable(getattr(api.CoherentDedisperser, member)), member
    assert isinstance(api.CoherentDedisperser.n_valid, property)
    assert callable(api.StokesBeams.voltages)
    for fn in (api.cdd_sweep_samples, api.cdd_edge, api.cdd_chirp):
        assert callable(fn)


def test_the_build_keeps_the_stage_outside_the_kernel_id():
    from dsabeamformer_amd import build

    srcs = [os.path.relpath(p, build.CSRC) for p in build.sources()]
    assert os.path.join("cdd", "bf_cdd.hip") in srcs and "bf_cdd.cpp" in srcs
    assert any(p.endswith(os.path.join("cdd", "bf_cdd_kernels.h")) for p in build._headers())
    before = build.kernel_build_id()
    real = build.CDD
    try:
        build.CDD = os.path.join(build.CSRC, "no_such_directory")                # the id does not look there
        assert build.kernel_build_id() == before
    finally:
        build.CDD = real


BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")                # no device either way: nothing here may need one


def _voltage_file(path, n_records=1):
    """A two-unit file of voltage cuts in the production geometry's layout, by hand (docs/VOLTAGE_CUTS.md section 5), tiny: 4 antennas."""
    head = ("HDR_SIZE 4096\nCONTENT voltages\nDTYPE packed4+4\nNANT 4\nNFREQ 2\nNPOL 2\nNAVG 16\nNOUT 8\nUNITS 2\nFIRST_CHANNEL 0\n"
            "LAYOUT unit,freq,time,pol,ant\nRECORD_HEADER_BYTES 28\n").encode()
    with open(path, "wb") as f:
        f.write(head + b"\0" * (4096 - len(head)))
        for r in range(n_records):
            f.write(np.array([128 * r], "<u8").tobytes() + np.array([3, 1, 2], "<i4").tobytes() + np.array([9.5], "<f8").tobytes())
            f.write(bytes(2 * 2 * 128 * 2 * 4))


def test_beam_usage_errors_come_before_any_device(tmp_path):
    import subprocess

    _lib()
    env = dict(os.environ, **NO_DEVICE)
    v, o = str(tmp_path / "v.bin"), str(tmp_path / "o.bin")
    _voltage_file(v)
    bad = str(tmp_path / "not_voltages.bin")
    with open(bad, "wb") as f:
        f.write(b"HDR_SIZE 4096\nCONTENT stokes\n" + b"\0" * 4096)
    full = ["--coherent", v, "--coherent-out", o, "-M", "250"]
    cases = [(full + ["-j", "27"], "-j"),                                        # with an observation
             (full + ["-k", "dada"], "-k"),
             (full + ["-E", "vis.bin", "-G", "g.bin"], "-E"),                     # with the solver
             (["--coherent-out", o, "-M", "250"], "--coherent V_FILE"),          # the children without the parent
             (["--coherent-fft", "256"], "--coherent V_FILE"),
             (["--coherent-int", "2"], "--coherent V_FILE"),
             (["--coherent-sideband", "-1"], "--coherent V_FILE"),
             (["--coherent", v, "-M", "250"], "--coherent-out"),                 # nowhere to write
             (["--coherent", v, "--coherent-out", o], "-M"),                     # no ladder
             (full + ["--coherent-fft", "100"], "--coherent-fft"),               # not a power of two
             (full + ["--coherent-fft", "32"], "--coherent-fft"),                # out of range
             (full + ["--coherent-fft", "8192"], "--coherent-fft"),
             (full + ["--coherent-fft", "256x"], "--coherent-fft"),
             (full + ["--coherent-int", "0"], "--coherent-int"),
             (full + ["--coherent-sideband", "0"], "--coherent-sideband"),
             (full + ["--coherent-sideband", "2"], "--coherent-sideband"),
             (["--coherent", str(tmp_path / "missing.bin"), "--coherent-out", o, "-M", "250"], "missing.bin"),
             (["--coherent", bad, "--coherent-out", o, "-M", "250"], "not a file of"),
             (full + ["-A", str(tmp_path / "no_gains.bin")], "-A")]
    before = sorted(os.listdir(str(tmp_path)))
    for args, word in cases:
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
        assert r.returncode != 0 and r.stderr.startswith("beam: ") and word in r.stderr and "GPUassert" not in r.stderr, (args, r.stdout, r.stderr)
        assert "Selected" not in r.stdout and "hip" not in r.stderr.lower(), (args, r.stdout, r.stderr)
    assert sorted(os.listdir(str(tmp_path))) == before                           # and nothing was created


def test_extended_usage_lists_the_options():
    import subprocess

    _lib()
    r = subprocess.run([BEAM, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for text in (" --coherent V_FILE --coherent-out FILE -M dm_max", "[--coherent-fft N]", "[--coherent-int n]", "[--coherent-sideband +1|-1]"):
        assert text in r.stdout, text
    h = subprocess.run([BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert "coherent" not in h.stdout                                            # the reference's own text stays as it is


def test_coherent_file_round_trip_and_the_default_length(tmp_path):
    from dsabeamformer_amd import host

    rng = np.random.default_rng(3)
    recs = [(7, 3, 255, 4, 9.25, 123.5, 15, 256, rng.standard_normal((128, 3, 4)).astype(np.float32)),
            (99999999999, 0, 0, 1, -1.0, 0.0, 0, 256, rng.standard_normal((128, 3, 4)).astype(np.float32))]
    path = str(tmp_path / "c.bin")
    co.write_coherent_file(path, 3, 128, 0, 2, -1, 256, recs)
    hdr, got = host.read_coherent_file(path)
    assert (hdr["CONTENT"], hdr["DTYPE"], hdr["LAYOUT"]) == ("coherent_stokes", "float32", "time,freq,iquv") and host.COHERENT_LAYOUT == hdr["LAYOUT"]
    assert (int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"]), int(hdr["NFFT"]), int(hdr["NINT"]), int(hdr["SIDEBAND"]), int(hdr["NTIME"])) == (3, 128, 0, 2, -1, 256)
    assert len(got) == 2
    for want, g in zip(recs, got):
        assert (g["t0"], g["dm"], g["beam"], g["width"], g["snr"], g["dm_value"], g["n_edge"], g["n_fft"]) == want[:8]
        assert g["data"].dtype == np.float32 and np.array_equal(g["data"], want[8])
