"""CPU checks of Faraday synthesis (include/dsabf.h: bf_rm_*; docs/FARADAY.md): the oracle's fused multiply-add against exact
rationals, its accuracy against float64, the physics in float64, the host helpers of the library against the formulas, and the
surface (refusals without a device, the ctypes table, the api, the build).  No GPU."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import rm_oracle as ro  # noqa: E402

BF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def api():
    from dsabeamformer_amd import api as a
    from dsabeamformer_amd import build as b

    b.build()
    return a


# ---- the oracle itself ------------------------------------------------------------------------------------------------------------
def _round32(f):
    """A Fraction rounded to the nearest float32, ties to even, subnormals included."""
    if f == 0:
        return np.float32(0)
    sign, f = (-1, -f) if f < 0 else (1, f)
    e = f.numerator.bit_length() - f.denominator.bit_length()
    while Fraction(2) ** e > f:
        e -= 1
    while Fraction(2) ** (e + 1) <= f:
        e += 1
    e = max(e, -126)
    q = f / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


def test_the_emulated_fma_is_exact():
    """fma32 against exact rationals on 6000 triples: random scales down to 2^-60, c = -round(a b) (cancellation), the ties
    (1 + 2^-12)^2 + k 2^-24 and those ties moved off by 2^-80 through a third operand scale, and subnormal results."""
    rng = np.random.default_rng(1)
    n = 6000
    a = (rng.standard_normal(n) * rng.choice([1, 1e-3, 1e3, 2.0 ** -60], n)).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * rng.choice([1, 1e-4, 1e4, 0], n)).astype(np.float32)
    c[:1500] = -(a[:1500] * b[:1500])
    a[1500:2500] = b[1500:2500] = np.float32(1 + 2.0 ** -12)                     # a b = 1 + 2^-11 + 2^-24: a tie at 24 bits
    c[1500:2500] = (rng.integers(-4, 5, 1000) * 2.0 ** -24).astype(np.float32)
    a[2500:3000] = np.float32(1 + 2.0 ** -12)                                    # the same ties, off by +-2^-80 ...
    b[2500:3000] = np.float32(1 + 2.0 ** -12)
    c[2500:3000] = (rng.choice([-1.0, 1.0], 500) * 2.0 ** -80).astype(np.float32)
    a[3000:3500] = (rng.standard_normal(500) * 2.0 ** -70).astype(np.float32)    # subnormal products and sums
    b[3000:3500] = (rng.standard_normal(500) * 2.0 ** -70).astype(np.float32)
    c[3000:3500] = (rng.standard_normal(500) * 2.0 ** -138).astype(np.float32)
    got = ro.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    bad = wrong_naive = 0
    for i in range(n):
        want = _round32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        bad += int(want != got[i])
        wrong_naive += int(want != naive[i])
    print("fma32: %d mismatches of %d; the plain float64 evaluation: %d" % (bad, n, wrong_naive))
    assert bad == 0 and wrong_naive > 0
    # the sign of an exact zero: round to nearest gives +0 unless both terms are -0
    z = ro.fma32(np.float32([0, -0.0, 1, 0]), np.float32([-1, 1, 1, 5]), np.float32([0, -0.0, -1, 0]))
    assert list(z.view(np.uint32)) == [0, 0x80000000, 0, 0]


def _gamma(n):
    u = 2.0 ** -24
    return n * u / (1 - n * u)


def test_the_chain_is_within_the_dot_product_bound():
    """The oracle's spectrum against float64 on the same float32 operands: |error| <= gamma_2C sum_c (|q| + |u|)(|r| + |s|)
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a dot product of 2 C terms)."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for n_chan in (1, 3, 64, 257, 1024):
        a = rng.uniform(0, 2 * np.pi, size=(48, n_chan))
        rot = np.empty((48, n_chan), np.complex64)
        rot.real, rot.imag = (np.cos(a) / n_chan).astype(np.float32), (np.sin(a) / n_chan).astype(np.float32)
        s = rng.standard_normal((8, n_chan, 3, 4)).astype(np.float32)
        spec, _ = ro.synthesize(s, rot, np.full(n_chan, 1.0 / n_chan, np.float32))
        want = ro.synthesize64(s, rot)
        _, q, u = ro.cells(s)
        bound = _gamma(2 * n_chan) * (np.abs(q) + np.abs(u)).astype(np.float64) @ (np.abs(rot.real) + np.abs(rot.imag)).astype(np.float64).T
        got = spec.reshape(24, 48).astype(np.complex128)
        ratio = max((np.abs(got.real - want.real) / bound).max(), (np.abs(got.imag - want.imag) / bound).max())
        print("n_chan %4d: largest error / bound = %.4f" % (n_chan, ratio))
        assert ratio <= 1.0, (n_chan, ratio)
        worst = max(worst, ratio)
    assert worst > 0


# ---- the physics, float64 ----------------------------------------------------------------------------------------------------------
FREQ = np.linspace(1.28, 1.53, 256)


def _float64_peaks(pol, inten, rot64, wn):
    """The records of one row through float64 arithmetic: (peaks array of one record)."""
    F = rot64 @ pol
    power = np.abs(F) ** 2
    p = int(np.argmax(power))
    rec = np.zeros(1, ro.PEAK)
    rec["p"], rec["pow_pk"], rec["re"], rec["im"], rec["isum"] = p, power[p], F[p].real, F[p].imag, np.sum(inten * wn)
    rec["pow_lo"] = power[p - 1] if p > 0 else 0
    rec["pow_hi"] = power[p + 1] if p < len(power) - 1 else 0
    return rec


def test_an_injected_rotation_measure_is_found(api):
    """Q + i U = L exp(2 i (chi0 + RM lambda^2)) over 256 channels of 1.28 ... 1.53 GHz on a grid of fwhm / 8: the argmax is the grid
    point nearest RM, rm_refine is within dphi / 2 of RM, pa within the angle that subtends, frac within 1e-3 of L / I; a masked
    channel that carries garbage changes nothing."""
    w = np.ones(256)
    fwhm, phi_max = api.rm_resolution(FREQ, w)
    dphi, n_phi, L, inten, chi0 = fwhm / 8, 512, 0.35, 2.0, -0.4
    l2 = ro.lambda2(FREQ)
    for rm_true in (-2000.0, -37.5, 0.0, 410.0, 1500.0):
        phi0 = np.round(rm_true / dphi) * dphi - 255.3 * dphi
        grid = phi0 + np.arange(n_phi) * dphi
        pol = L * np.exp(2j * (chi0 + rm_true * l2))
        records = []
        for mask in (None, 100):
            wt = w.copy()
            data = pol.copy()
            if mask is not None:
                wt[mask], data[mask] = 0.0, 1e6 - 3e5j
            l0 = ro.lambda0_2(FREQ, wt)
            rot64 = (wt / wt.sum()) * np.exp(-1j * ro.angles(FREQ, wt, phi0, dphi, n_phi))
            rec = _float64_peaks(data, np.full(256, inten), rot64, wt / wt.sum())
            assert rec["p"][0] == int(np.argmin(np.abs(grid - rm_true))), (rm_true, mask)
            fit = api.rm_refine(rec, phi0, dphi, n_phi, l0)[0]
            mine = [v[0] for v in ro.refine(rec, phi0, dphi, n_phi, l0)]
            assert np.allclose([fit["rm"], fit["pa"], fit["lin"], fit["frac"]], mine, rtol=1e-13, atol=1e-13)
            err, pa_err = abs(fit["rm"] - rm_true), abs((fit["pa"] - chi0 + np.pi / 2) % np.pi - np.pi / 2)
            print("RM %8.1f mask %s: |rm - RM| = %.3e dphi, |pa - chi0| = %.2e, frac - L / I = %.2e" % (rm_true, mask, err / dphi, pa_err, fit["frac"] - L / inten))
            assert err <= dphi / 2 and pa_err <= dphi / 2 * l0 and abs(fit["frac"] - L / inten) <= 1e-3
            records.append(rec)
        # (the masked run differs only by the one channel's share of the sums)
        assert records[0]["p"][0] == records[1]["p"][0]
    # the garbage itself: with the weight zero the spectrum does not see the channel at all
    wt = w.copy()
    wt[100] = 0
    rot, wn, _ = api.rm_table(FREQ, wt, -100.0, dphi, 64)
    assert (rot[:, 100] == 0).all() and wn[100] == 0
    s = np.zeros((1, 256, 1, 4), np.float32)
    s[0, :, 0, 1], s[0, :, 0, 2] = pol.real, pol.imag
    clean = ro.synthesize(s, rot, wn)
    s[0, 100, 0] = [7e5, 1e6, -3e5, 1.0]
    dirty = ro.synthesize(s, rot, wn)
    assert np.array_equal(clean[0].view(np.uint32), dirty[0].view(np.uint32)) and clean[1].tobytes() == dirty[1].tobytes()


# ---- the helpers of the library -------------------------------------------------------------------------------------------------------
def test_helpers_against_the_formulas(api):
    assert api.rm_lambda2(1.4) == (0.299792458 / 1.4) ** 2
    rng = np.random.default_rng(3)
    w = rng.uniform(0, 2, 256)
    w[[0, 17, 255]] = 0
    rot, wn, l0 = api.rm_table(FREQ, w, -300.0, 2.5, 77)
    want_rot, want_wn, want_l0 = ro.table(FREQ, w, -300.0, 2.5, 77)
    assert abs(l0 - want_l0) <= 1e-15 and rot.shape == (77, 256) and rot.dtype == np.complex64 and wn.dtype == np.float32
    # one float32 ulp of the entry: the library and numpy may round cos and sin differently in the last place of a double
    ulp = np.spacing(np.maximum(np.abs(want_rot.real), np.abs(want_rot.imag)).astype(np.float32))
    assert (np.abs(rot.real - want_rot.real) <= ulp).all() and (np.abs(rot.imag - want_rot.imag) <= ulp).all()
    assert (np.abs(wn - want_wn) <= np.spacing(want_wn)).all() and wn[0] == 0 and (rot[:, 17] == 0).all()
    # the RMSF: modulus 1 at depth 0, nowhere larger, and equal to the formula
    r = api.rm_rmsf(FREQ, w, -64 * 2.5, 2.5, 129)
    assert abs(abs(r[64]) - 1.0) <= 1e-14 and int(np.argmax(np.abs(r))) == 64
    assert np.allclose(r, ro.rmsf(FREQ, w, -64 * 2.5, 2.5, 129), rtol=0, atol=1e-12)
    # the width of the RMSF's main lobe is the fwhm of the resolution, to the few per cent of that approximation
    fwhm, phi_max = api.rm_resolution(FREQ, np.ones(256))
    fine = np.abs(api.rm_rmsf(FREQ, np.ones(256), -fwhm, fwhm / 500, 1001))
    above = np.flatnonzero(fine >= 0.5)
    assert abs((above[-1] - above[0]) * fwhm / 500 / fwhm - 1.0) < 0.12
    # known answers: two channels at 1 and 2 GHz
    c2 = 0.299792458 ** 2
    fwhm2, pmax2 = api.rm_resolution([1.0, 2.0], [1.0, 1.0])
    assert abs(fwhm2 - 2 * np.sqrt(3) / (0.75 * c2)) <= 1e-12 * fwhm2 and abs(pmax2 - np.sqrt(3) / (0.75 * c2)) <= 1e-12 * pmax2
    want_fwhm, want_pmax = ro.resolution(FREQ, w)
    got_fwhm, got_pmax = api.rm_resolution(FREQ, w)
    assert abs(got_fwhm - want_fwhm) <= 1e-12 * want_fwhm and abs(got_pmax - want_pmax) <= 1e-12 * want_pmax
    # the fit: the parabola's vertex, the grid ends, a flat top, no intensity
    pk = np.zeros(5, api.rm_peak_dtype())
    pk["p"], pk["pow_lo"], pk["pow_pk"], pk["pow_hi"], pk["re"], pk["im"], pk["isum"] = [3, 0, 9, 3, 3], [1, 0, 3, 4, 4], 4, [3, 2, 0, 4, 1], 2, 0, [4, 4, 4, 0, -1]
    fit = api.rm_refine(pk, 10.0, 2.0, 10, 0.0)
    assert np.allclose(fit["rm"], [10 + 2 * (3 + 0.5 * (1 - 3) / (1 - 8 + 3)), 10.0, 28.0, 16.0, 10 + 2 * (3 + 0.5 * 3 / (4 - 8 + 1))], rtol=1e-15)
    assert list(fit["lin"]) == [2.0] * 5 and list(fit["frac"]) == [0.5, 0.5, 0.5, 0.0, 0.0] and (fit["pa"] == 0).all()
    # pa is wrapped into [-pi / 2, pi / 2)
    pk2 = np.zeros(3, api.rm_peak_dtype())
    pk2["p"], pk2["pow_pk"], pk2["re"], pk2["im"] = 1, 1, [-1, -1, 1], [1e-9, -1e-9, 0]
    pa = api.rm_refine(pk2, 0.0, 1.0, 3, 0.0)["pa"]
    assert (pa >= -np.pi / 2).all() and (pa < np.pi / 2).all() and abs(pa[0] - np.pi / 2) < 1e-8 and abs(pa[1] + np.pi / 2) < 1e-8
    pa = api.rm_refine(pk2, 0.0, 1.0, 3, 100.0)["pa"]                            # rm = 1: pa0 - 100
    assert (pa >= -np.pi / 2).all() and (pa < np.pi / 2).all() and abs(pa[2] - ((-100 + np.pi / 2) % np.pi - np.pi / 2)) < 1e-12


# ---- the surface -----------------------------------------------------------------------------------------------------------------------
def test_every_export_refuses_null_and_bad_arguments(api):
    lib = api.load()
    f = (C.c_double * 3)(1.3, 1.4, 1.5)
    w = (C.c_double * 3)(1, 1, 1)
    z = (C.c_double * 3)(0, 0, 0)
    neg = (C.c_double * 3)(1, -1, 1)
    x, y = C.c_double(), C.c_double()
    buf = (C.c_float * 64)()
    out = C.c_void_p(5)
    assert lib.bf_rm_create(None, 3, 4, buf, buf, C.byref(out)) == BF_ERR_INVALID and out.value is None and b"handle" in lib.bf_last_error()
    assert lib.bf_rm_create(None, 3, 4, buf, buf, None) == BF_ERR_INVALID
    assert lib.bf_rm_destroy(None) == 0
    assert lib.bf_rm_set_table(None, buf, buf) == BF_ERR_INVALID
    assert lib.bf_rm_device(None, None, 1, 1, None, None, None, None) == BF_ERR_INVALID and b"bf_rm_device" in lib.bf_last_error()
    assert lib.bf_rm_resolution(None, w, 3, C.byref(x), C.byref(y)) == BF_ERR_INVALID
    assert lib.bf_rm_resolution(f, w, 3, None, C.byref(y)) == BF_ERR_INVALID
    assert lib.bf_rm_resolution(f, z, 3, C.byref(x), C.byref(y)) == BF_ERR_INVALID and b"masked" in lib.bf_last_error()
    assert lib.bf_rm_resolution(f, neg, 3, C.byref(x), C.byref(y)) == BF_ERR_INVALID
    assert lib.bf_rm_resolution(f, w, 1, C.byref(x), C.byref(y)) == BF_ERR_INVALID      # one channel spans nothing
    assert lib.bf_rm_resolution(f, w, 0, C.byref(x), C.byref(y)) == BF_ERR_INVALID
    assert lib.bf_rm_table(f, w, 3, 0.0, 1.0, 4, None, buf, None) == BF_ERR_INVALID
    assert lib.bf_rm_table(f, w, 3, 0.0, 1.0, 0, buf, buf, None) == BF_ERR_INVALID
    assert lib.bf_rm_table(f, w, 3, 0.0, 1.0, 4097, buf, buf, None) == BF_ERR_INVALID
    assert lib.bf_rm_table(f, w, 4097, 0.0, 1.0, 4, buf, buf, None) == BF_ERR_INVALID
    assert lib.bf_rm_table(f, w, 3, float("nan"), 1.0, 4, buf, buf, None) == BF_ERR_INVALID
    assert lib.bf_rm_table(f, w, 3, 0.0, 1.0, 4, buf, buf, None) == 0
    assert lib.bf_rm_rmsf(f, w, 3, 0.0, 1.0, 4, None) == BF_ERR_INVALID and lib.bf_rm_rmsf(f, None, 3, 0.0, 1.0, 4, buf) == BF_ERR_INVALID
    pk = np.zeros(2, api.rm_peak_dtype())
    fits = np.zeros(2, api.rm_fit_dtype())
    assert lib.bf_rm_refine(None, 2, 0.0, 1.0, 4, 0.0, fits.ctypes.data) == BF_ERR_INVALID
    assert lib.bf_rm_refine(pk.ctypes.data, 2, 0.0, 1.0, 4, 0.0, None) == BF_ERR_INVALID
    pk["p"][1] = 4
    assert lib.bf_rm_refine(pk.ctypes.data, 2, 0.0, 1.0, 4, 0.0, fits.ctypes.data) == BF_ERR_INVALID and b"outside the grid" in lib.bf_last_error()


def test_lib_table_api_surface_and_build(api):
    from dsabeamformer_amd import _lib, build

    names = ["bf_rm_lambda2", "bf_rm_resolution", "bf_rm_table", "bf_rm_rmsf", "bf_rm_refine", "bf_rm_create", "bf_rm_destroy", "bf_rm_set_table",
             "bf_rm_device"]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("bf_rm_")) == sorted(names)
    assert _lib.SIGNATURES["bf_rm_lambda2"][0] is C.c_double and len(_lib.SIGNATURES["bf_rm_device"][1]) == 8
    for name in ("FaradaySynthesis", "rm_lambda2", "rm_resolution", "rm_table", "rm_rmsf", "rm_refine", "rm_peak_dtype", "rm_fit_dtype"):
        assert hasattr(api, name), name
    for method in ("set_table", "run", "close"):
        assert callable(getattr(api.FaradaySynthesis, method))
    assert api.rm_peak_dtype() == ro.PEAK and api.rm_peak_dtype().itemsize == 32 and api.rm_fit_dtype().itemsize == 32
    assert api.rm_peak_dtype().names == ("p", "pow_lo", "pow_pk", "pow_hi", "re", "im", "isum", "zero")
    # the device code is built into the library from a directory of its own, outside the kernel build id
    rm_dir = os.path.join(build.CSRC, "rm")
    assert build.RM == rm_dir and os.path.join(rm_dir, "bf_rm.hip") in build.sources() and os.path.join(rm_dir, "bf_rm_kernels.h") in build._headers()
    assert os.path.join(build.CSRC, "bf_rm.cpp") in build.sources()
    src = open(os.path.join(ROOT, "dsabeamformer_amd", "build.py")).read()
    assert "RM" not in src.split("def kernel_build_id")[1].split("\ndef ")[0]
    import glob

    hashed = glob.glob(os.path.join(build.CSRC, "*.hip")) + glob.glob(os.path.join(build.CSRC, "*.h*")) + glob.glob(os.path.join(build.CSRC, "*.inc"))
    assert not any(os.sep + "rm" + os.sep in p for p in hashed)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def _header(**kv):
    text = "".join("%s %s\n" % (k, v) for k, v in kv.items()).encode()
    return text + b"\0" * (4096 - len(text))


def test_beam_refuses_every_usage_error_before_a_device(api, tmp_path):
    """Every usage error of `beam --faraday`, with no device visible: exit status 1, a line `beam: ...`, nothing on stdout, no file."""
    import subprocess

    from dsabeamformer_amd import build

    ok = str(tmp_path / "c_ok")
    with open(ok, "wb") as f:
        f.write(_header(HDR_SIZE=4096, CONTENT="coherent_stokes", DTYPE="float32", NFREQ=4, FIRST_CHANNEL=0, NFFT=0, NINT=1, SIDEBAND=1, NTIME=32, NAVG=16,
                        LAYOUT="time,freq,iquv", RECORD_HEADER_BYTES=44))
    volt = str(tmp_path / "v_other")
    with open(volt, "wb") as f:
        f.write(_header(HDR_SIZE=4096, CONTENT="voltages", DTYPE="packed4+4", RECORD_HEADER_BYTES=28, NANT=64, NPOL=2, NFREQ=256, NAVG=16, NOUT=8, UNITS=2,
                        FIRST_CHANNEL=0))
    partial = str(tmp_path / "c_partial")
    open(partial, "wb").write(open(ok, "rb").read() + b"\0" * 100)                # (a record of this header is 44 + 32 * 4 * 16 bytes)
    short = str(tmp_path / "short")
    open(short, "wb").write(b"too short\n")
    mask_bad = str(tmp_path / "mask_bad")
    open(mask_bad, "w").write("3\n9999\n")
    FA = ["--faraday", ok, "--faraday-out", "o"]
    cases = [(["--faraday-out", "o"], "give --faraday"), (["--faraday-phi", "-100:100:64"], "give --faraday"), (["--faraday-window", "4"], "give --faraday"),
             (FA + ["-j", "27"], "leave out -j"), (FA + ["-k", "ring"], "leave out -j"), (FA + ["-E", "vis"], "leave out -j"),
             (FA + ["--coherent", "v", "--coherent-out", "c", "-M", "40"], "leave out -j"),
             (FA + ["-M", "40"], "leave out -M"), (FA + ["-M", "40", "-S", "8"], "leave out -M"), (FA + ["-M", "40", "-n", "4"], "leave out -M"),
             (FA + ["-A", "gains"], "leave out -M"), (FA + ["-Z", "nulls"], "leave out -M"),
             (["--faraday", ok], "needs --faraday-out"),
             (FA + ["--faraday-phi", "abc"], "three numbers"), (FA + ["--faraday-phi", "1:2"], "three numbers"), (FA + ["--faraday-phi", "1:2:3:4"], "three numbers"),
             (FA + ["--faraday-phi", "1:2:3.5"], "three numbers"), (FA + ["--faraday-phi", "1:nan:3"], "three numbers"), (FA + ["--faraday-phi", ""], "three numbers"),
             (FA + ["--faraday-phi", "1:2:0"], "an empty grid"), (FA + ["--faraday-phi", "1:2:-4"], "an empty grid"), (FA + ["--faraday-phi", "2:1:16"], "an empty grid"),
             (FA + ["--faraday-phi", "1:2:1"], "an empty grid"), (FA + ["--faraday-phi", "-100:100:4097"], "at most 4096"),
             (FA + ["--faraday-window", "0"], "at least 1 row"), (FA + ["--faraday-window", "-3"], "at least 1 row"), (FA + ["--faraday-window", "2x"], "whole number"),
             (FA + ["--faraday-window", ""], "whole number"),
             (FA + ["-F", mask_bad], "not a channel index"), (FA + ["-F", str(tmp_path / "missing")], "could not be read"),
             (["--faraday", volt, "--faraday-out", "o"], "is not a file of coherently dedispersed Stokes parameters"),
             (["--faraday", short, "--faraday-out", "o"], "cannot read a 4096-byte header"),
             (["--faraday", partial, "--faraday-out", "o"], "does not end with a whole record"),
             (["--faraday", str(tmp_path / "missing"), "--faraday-out", "o"], "cannot read a 4096-byte header")]
    first_file_case = next(n for n, (argv, _) in enumerate(cases) if "-F" in argv)   # from here on a file speaks, in its own words
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    for n, (argv, text) in enumerate(cases):
        cwd = tmp_path / ("run%d" % n)
        cwd.mkdir()
        r = subprocess.run([build.BEAM] + argv, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stderr.startswith("beam: ") and text in r.stderr and not r.stdout and not list(cwd.iterdir()), (argv, r.returncode, r.stderr, r.stdout)
        if n < first_file_case:   # the refusals of the mode's own rules end in its synopsis
            assert all(word in r.stderr for word in ("usage: beam --faraday C_FILE", "--faraday-out FILE", "[--faraday-phi LO:HI:N]", "[--faraday-window ROWS]",
                                                     "[-F mask_file]")), (argv, r.stderr)
    # a command line without a fault passes every check and fails at the missing device, with no output file
    for argv in (FA, FA + ["--faraday-phi", "-100:100:64", "--faraday-window", "4", "-F", str(tmp_path / "mask_ok")], FA + ["--faraday-phi", "5:5:1"]):
        open(str(tmp_path / "mask_ok"), "w").write("# none of this file's\n200\n")
        cwd = tmp_path / ("pass%d" % len(argv))
        cwd.mkdir()
        r = subprocess.run([build.BEAM] + argv, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stderr.startswith("GPUassert:") and "beam:" not in r.stderr and not list(cwd.iterdir()), (argv, r.stderr)
    # -h is the reference's text (tests/test_beam_cli_cpu.py); the mode is not in it
    assert "faraday" not in subprocess.run([build.BEAM, "-h"], capture_output=True, text=True, timeout=60).stdout


def test_faraday_file_round_trip(api, tmp_path):
    """A file written by hand in the documented layout comes back through host.read_faraday_file."""
    from dsabeamformer_amd import host

    rng = np.random.default_rng(4)
    n_phi, n_rows = 5, 3
    head = _header(HDR_SIZE=4096, CONTENT="faraday", DTYPE="float32", NFREQ=4, FIRST_CHANNEL=7, NROWS=n_rows, NPHI=n_phi, PHI0=-10.5, DPHI=5.25, LAMBDA0_2=0.046,
                   FWHM=42.0, PHI_MAX=9000.0, RECORD_HEADER_BYTES=84)
    want = []
    with open(str(tmp_path / "f.bin"), "wb") as f:
        f.write(head)
        for r in range(2):
            spec = (rng.standard_normal(n_phi) + 1j * rng.standard_normal(n_phi)).astype(np.complex64)
            peaks = np.zeros(1 + n_rows, ro.PEAK)
            peaks["p"], peaks["pow_pk"], peaks["isum"] = rng.integers(0, n_phi, 1 + n_rows), rng.random(1 + n_rows), rng.random(1 + n_rows)
            rec = dict(t0=2 ** 40 + r, dm=3, beam=200 + r, width=4, snr=9.5, dm_value=123.25, n_edge=30, n_fft=256, lo=11, w=2, rm=-37.5, pa=0.3, lin=2.0, frac=0.5)
            f.write(np.array([rec["t0"]], "<u8").tobytes() + np.array([rec["dm"], rec["beam"], rec["width"]], "<i4").tobytes()
                    + np.array([rec["snr"], rec["dm_value"]], "<f8").tobytes() + np.array([rec["n_edge"], rec["n_fft"], rec["lo"], rec["w"]], "<i4").tobytes()
                    + np.array([rec["rm"], rec["pa"], rec["lin"], rec["frac"]], "<f8").tobytes() + spec.tobytes() + peaks.tobytes())
            want.append((rec, spec, peaks))
    hdr, recs = host.read_faraday_file(str(tmp_path / "f.bin"))
    assert (hdr["CONTENT"], hdr["NPHI"], hdr["NROWS"], hdr["FIRST_CHANNEL"], float(hdr["PHI0"]), float(hdr["DPHI"])) == ("faraday", "5", "3", "7", -10.5, 5.25)
    assert len(recs) == 2
    for got, (rec, spec, peaks) in zip(recs, want):
        assert {k: got[k] for k in rec} == rec
        assert np.array_equal(got["spec"], spec) and got["peaks"].tobytes() == peaks.tobytes() and got["peaks"].shape == (1 + n_rows,)


def test_the_file_mode_oracle_on_a_made_up_record():
    """rm_oracle.faraday_record: the window is the first maximum of the boxcar, the baseline leaves the window and w rows on either side
    out, and a record with fewer than 8 baseline rows is left out."""
    rng = np.random.default_rng(5)
    data = rng.standard_normal((40, 4, 4)).astype(np.float32)
    data[17:19, :, 0] += 50
    data[30:32, :, 0] = data[17:19, :, 0]                                       # an equal second burst cannot win: the first maximum
    rot, wn, _ = ro.table([1.3, 1.35, 1.4, 1.45], np.ones(4), -50.0, 10.0, 11)
    lo, spec, peaks = ro.faraday_record(data, 2, rot, wn)
    assert lo == 17 and spec.shape == (11,) and peaks.shape == (41,)
    base = data[np.r_[0:15, 21:40]].astype(np.float64).mean(axis=0)
    row0 = data[17:19].astype(np.float64).mean(axis=0)
    want = ((row0[:, 1] - base[:, 1]) + 1j * (row0[:, 2] - base[:, 2])) @ rot.astype(np.complex128).T
    assert np.abs(spec - want).max() < 1e-5
    assert ro.faraday_record(data[11:24], 2, rot, wn) is None and ro.faraday_record(data[10:24], 2, rot, wn) is not None   # 4 + 3 and 5 + 3 baseline rows
