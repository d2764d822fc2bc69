"""CPU tests of the pulsar folder's host side (include/dsabf.h: bf_psr_model_from_spin, bf_psr_beam_snr, the refusals of
bf_psr_create that need no device; include/dsabf_host.h: bfh_psr_sink_*) against tests/support/psr_oracle.py, the numpy restatement of
docs/PULSAR_FOLDING.md section 1.  Integers are compared exactly, doubles bit for bit."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import psr_oracle  # noqa: E402

BF_ERR_INVALID = -1
ROW = 0.131072e-3      # seconds per row of the detected stream at the production window

SPINS = [(3.3, -2e-3, 0.25, ROW), (1.0 / (30 * 64 * ROW), 0.0, 0.0, ROW), (9000.0, 1e-2, 0.999, ROW),      # the last: f0 * row > 1
         (0.0, 0.0, 0.5, ROW), (716.35, -1.5e-9, -0.3, 1e-3), (29.946923, -3.77535e-10, 7.75, ROW), (-2.5, 3.0, 1.0, 0.01)]


@pytest.fixture(scope="module")
def lib():
    from dsabeamformer_amd import build as b
    from dsabeamformer_amd import _lib

    b.build()
    return _lib.load()


def lib_model(lib, f0, f1, p0, row, epoch=0):
    from dsabeamformer_amd import _lib

    m = _lib.BfPsrModel()
    rc = lib.bf_psr_model_from_spin(f0, f1, p0, row, epoch, C.byref(m))
    return rc, (m.phase0, m.dphase, m.ddphase, m.epoch_row)


def test_model_from_spin_is_the_oracles_integers(lib):
    for k, (f0, f1, p0, row) in enumerate(SPINS):
        rc, got = lib_model(lib, f0, f1, p0, row, 1000 * k - 3)
        assert rc == 0 and got == psr_oracle.model_from_spin(f0, f1, p0, row, 1000 * k - 3), (f0, f1, p0, row)
    assert any(f1 < 0 for _, f1, _, _ in SPINS) and any(f0 * row > 1 for f0, _, _, row in SPINS) and any(f0 == 0 for f0, _, _, _ in SPINS)
    assert lib_model(lib, 0.0, 0.0, 0.5, ROW)[1][:3] == (1 << 63, 0, 0)
    # a fraction that rounds up to 1.0 is phase 0; the refusals
    assert lib_model(lib, 1.0, 0.0, -1e-30, 1.0)[1][:2] == (0, 0) == psr_oracle.model_from_spin(1.0, 0.0, -1e-30, 1.0)[:2]
    for bad in ((float("nan"), 0, 0, ROW), (1.0, float("inf"), 0, ROW), (1.0, 0, float("-inf"), ROW), (1.0, 0, 0, 0.0), (1.0, 0, 0, -1.0),
                (1.0, 0, 0, float("nan")), (1.0, 0.25, 0, 1.0), (1.0, -0.3, 0, 1.0)):
        assert lib_model(lib, *bad)[0] == BF_ERR_INVALID and psr_oracle.model_from_spin(*bad) is None, bad
        assert b"bf_psr_model_from_spin" in lib.bf_last_error()
    assert lib.bf_psr_model_from_spin(1.0, 0.0, 0.0, 1.0, 0, None) == BF_ERR_INVALID
    assert lib_model(lib, 1.0, 0.2499, 0, 1.0)[0] == 0


def test_fixed_point_bins_are_the_bins_of_the_phase_in_fp64(lib):
    """The rule bin = ((phase >> 32) n_bins) >> 32 on the NCO's integers against floor(frac(phi) n_bins) with phi = f0 t + f1 t^2 / 2
    in plain fp64, on 200 rows x 3 channels with their own delays, 5 and 64 bins.  The two differ only where phi n_bins lies within the
    NCO's quantisation of a bin edge: |phi_nco - phi| <= 2^-64 (n + n^2 / 2 + 1) turns plus the fp64 error of phi itself, a few 1e-13
    here; no cell of this case lies within 1e-9 bins of an edge (asserted), so all 600 must agree."""
    f0, f1, p0 = 3.3, -2e-3, 0.0
    rc, model = lib_model(lib, f0, f1, p0, ROW, 17)
    assert rc == 0
    delays = np.array([0, 40, 7], np.int32)
    n = np.arange(200, dtype=np.int64)[:, None] - 17 - delays[None, :].astype(np.int64)
    t = n.astype(np.float64) * ROW
    phi = f0 * t + 0.5 * f1 * t * t
    frac = phi - np.floor(phi)
    for n_bins in (5, 64):
        got = psr_oracle.bins(model, delays, 0, 200, n_bins)
        want = np.floor(frac * n_bins).astype(np.int64)
        edge = (np.abs(frac * n_bins - np.rint(frac * n_bins)) < 1e-9) & (n != 0)      # (n = 0 is phase 0 exactly, in both)
        assert not edge.any()                              # a condition on this test's own 600 cells, not on the rule
        assert got.shape == (200, 3) and np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < n_bins


def _profile(rng, n_f, n_bins, n_b):
    hits = rng.integers(1, 40, (n_f, n_bins)).astype(np.uint64)
    prof = rng.standard_normal((n_f, n_bins, n_b)) * 50.0 + 10.0 * hits[:, :, None].astype(np.float64)
    return prof, hits


def lib_snr(lib, prof, hits, mask=None):
    from dsabeamformer_amd import api

    return api.PulsarFolder.beam_snr(prof, hits, mask)


def test_beam_snr_is_the_oracles_to_the_bit(lib):
    rng = np.random.default_rng(5)
    n_f, n_bins, n_b = 6, 16, 9
    prof, hits = _profile(rng, n_f, n_bins, n_b)
    prof[:, 11, 4] += 4000.0                                   # a pulse in beam 4, bin 11
    mask = np.zeros(n_f, np.uint8)
    mask[2] = 1
    cases = [(prof, hits, None), (prof, hits, mask)]
    p2, h2 = prof.copy(), hits.copy()
    h2[:, 3] = 0                                               # a bin nothing fell into (its profile cells are ignored)
    p2[:, 3, :] = 1e30
    cases.append((p2, h2, mask))
    p3, h3 = _profile(rng, n_f, 7, n_b)                        # an odd number of live bins
    cases.append((p3, h3, None))
    for p, h, m in cases:
        snr, peak = lib_snr(lib, p, h, m)
        want_snr, want_peak = psr_oracle.beam_snr(p, h, m)
        assert np.array_equal(snr.view(np.uint64), want_snr.view(np.uint64)) and np.array_equal(peak, want_peak)
        assert np.all(peak >= 0) and np.all(snr > 0)
    snr, peak = lib_snr(lib, prof, hits, mask)
    assert peak[4] == 11 and np.argmax(snr) == 4
    assert lib_snr(lib, p2, h2, mask)[1].tolist().count(3) == 0
    # an all-equal profile: sigma 0 -> snr 0, peak -1
    flat_h = np.full((n_f, n_bins), 3, np.uint64)
    flat = np.full((n_f, n_bins, n_b), 6.0)
    for got in (lib_snr(lib, flat, flat_h), psr_oracle.beam_snr(flat, flat_h)):
        assert not got[0].any() and np.all(got[1] == -1)
    # fewer than 4 live bins
    few = hits.copy()
    few[:, 3:] = 0
    for got in (lib_snr(lib, prof, few), psr_oracle.beam_snr(prof, few)):
        assert not got[0].any() and np.all(got[1] == -1)
    few[:, 3] = 1
    assert np.all(lib_snr(lib, prof, few)[1] >= 0)
    # every channel masked: no live bin
    assert np.all(lib_snr(lib, prof, hits, np.ones(n_f, np.uint8))[1] == -1)
    assert lib.bf_psr_beam_snr(None, None, 1, 4, 1, None, None, None) == BF_ERR_INVALID


def test_creation_refusals_that_need_no_device(lib):
    from dsabeamformer_amd import _lib

    models = (_lib.BfPsrModel * 4)()
    delays = np.zeros((4, 6), np.int32)

    def create(n_freq=6, rows=8, n_bins=16, n_psr=2, in_flight=2, m=models, d=delays, out=True):
        p = C.c_void_p()
        rc = lib.bf_psr_create(None, n_freq, rows, n_bins, C.cast(m, C.c_void_p) if m is not None else None, d.ctypes.data if d is not None else None, n_psr,
                               in_flight, C.byref(p) if out else None)
        assert not p.value
        return rc, lib.bf_last_error()

    for kw, msg in ((dict(n_bins=1), b"n_bins"), (dict(n_bins=4097), b"n_bins"), (dict(n_psr=0), b"n_psr"), (dict(n_psr=5), b"n_psr"),
                    (dict(n_freq=0), b"n_freq_total"), (dict(rows=0), b"max_rows_per_push"), (dict(in_flight=0), b"max_in_flight"),
                    (dict(m=None), b"NULL"), (dict(d=None), b"NULL"), (dict(out=False), b"out is NULL")):
        rc, err = create(**kw)
        assert rc == BF_ERR_INVALID and msg in err, (kw, err)
    neg = delays.copy()
    neg[1, 3] = -1
    rc, err = create(d=neg)
    assert rc == BF_ERR_INVALID and b"delay[9] = -1" in err
    # everything in range: what is left to refuse is the missing handle
    rc, err = create(n_bins=2)
    assert rc == BF_ERR_INVALID and b"handle is NULL" in err
    assert create(n_bins=4096, n_psr=4)[1] == err
    assert lib.bf_psr_entries(3, 40, 64, 256) == 3 * 40 * 64 * 256
    assert [lib.bf_psr_entries(*a) for a in ((0, 1, 2, 1), (5, 1, 2, 1), (1, 0, 2, 1), (1, 1, 1, 1), (1, 1, 4097, 1), (1, 1, 2, 0))] == [0] * 6
    for call in (lambda: lib.bf_psr_push(None, None, 1, None), lambda: lib.bf_psr_dump(None, None), lambda: lib.bf_psr_pending(None),
                 lambda: lib.bf_psr_collect(None, None, None, None, None), lambda: lib.bf_dm_stream_attach_folder(None, None)):
        assert call() == BF_ERR_INVALID
    assert lib.bf_psr_destroy(None) == 0


def test_file_sink_round_trip(lib, tmp_path):
    rng = np.random.default_rng(8)
    n_psr, n_f, n_bins, n_b = 2, 3, 5, 4
    path = str(tmp_path / "folds.bin")
    s = C.c_void_p()
    assert lib.bfh_psr_sink_create(path.encode(), n_psr, n_f, n_bins, n_b, C.byref(s)) == 0
    sent = []
    for k in range(3):
        hits = rng.integers(0, 1 << 40, (n_psr, n_f, n_bins)).astype(np.uint64)
        prof = (rng.standard_normal((n_psr, n_f, n_bins, n_b)) * 2.0 ** rng.integers(-40, 41, (n_psr, n_f, n_bins, n_b))).astype(np.float64)
        assert lib.bfh_psr_sink_deliver(s, 100 * k, 100 + k, hits.ctypes.data, prof.ctypes.data) == 0
        sent.append((100 * k, 100 + k, hits, prof))
    assert lib.bfh_psr_sink_deliver(s, 0, 0, None, None) == BF_ERR_INVALID
    assert lib.bfh_psr_sink_destroy(s) == 0
    header, recs = psr_oracle.read_file(path)
    assert header["HDR_SIZE"] == "4096" and header["CONTENT"] == "folds" and header["DTYPE"] == "float64"
    assert [int(header[k]) for k in ("NPSR", "NFREQ", "NBINS", "NBEAMS", "RECORD_HEADER_BYTES")] == [n_psr, n_f, n_bins, n_b, 32]
    assert len(recs) == 3 and os.path.getsize(path) == 4096 + 3 * (32 + 8 * n_psr * n_f * n_bins * (1 + n_b))
    for r, (first, n, hits, prof) in zip(recs, sent):
        assert (r["first_row"], r["n_rows"]) == (first, n) and np.array_equal(r["hits"], hits)
        assert np.array_equal(r["profile"].view(np.uint64), prof.view(np.uint64))
    assert lib.bfh_psr_sink_create(str(tmp_path / "no" / "such" / "dir").encode(), 1, 1, 2, 1, C.byref(s)) == BF_ERR_INVALID
    assert lib.bfh_psr_sink_create(path.encode(), 0, 1, 2, 1, C.byref(s)) == BF_ERR_INVALID


def test_the_oracles_fold_is_an_ordered_sum():
    """The oracle against the definition, cell by cell in a Python loop, on a small case whose input makes the order matter."""
    rng = np.random.default_rng(2)
    n_rows, n_f, n_b, n_bins = 60, 2, 3, 5
    x = (rng.standard_normal((n_rows, n_f, n_b)) * 2.0 ** rng.integers(-40, 41, (n_rows, n_f, n_b))).astype(np.float32)
    model = psr_oracle.model_from_spin(3.3e3, -2.0, 0.1, 1e-4, 20)
    delays = np.array([[0, 9]], np.int32)
    prof, hits = psr_oracle.fold(x, [model], delays, n_bins, first_row=5)
    b = psr_oracle.bins(model, delays[0], 5, n_rows, n_bins)
    for f in range(n_f):
        for j in range(n_bins):
            rows = [r for r in range(n_rows) if b[r, f] == j]
            assert hits[0, f, j] == len(rows)
            for beam in range(n_b):
                acc = 0.0
                for r in rows:
                    acc = acc + float(x[r, f, beam])
                assert prof[0, f, j, beam] == acc and math.copysign(1.0, prof[0, f, j, beam]) == math.copysign(1.0, acc)
    back = psr_oracle.fold(x, [model], delays, n_bins, first_row=5, reverse=True)
    assert np.array_equal(back[1], hits) and not np.array_equal(back[0].view(np.uint64), prof.view(np.uint64))
