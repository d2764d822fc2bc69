"""CPU tests of the periodicity search's host side (include/dsabf.h: bf_ffa_rows_of, bf_ffa_entries, bf_ffa_select, the refusals of
bf_ffa_create that need no device; include/dsabf_host.h: bfh_ffa_sink_*) and of tests/support/ffa_oracle.py itself, the numpy
restatement of docs/PERIODICITY.md section 1.  Integers are compared exactly, floats bit for bit."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import ffa_oracle  # noqa: E402
from ffa_stage import EDGE_CASES, PARITY_CASES, case_cfg, case_input, case_lds_bytes, case_max_rows  # noqa: E402

BF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from dsabeamformer_amd import build as b
    from dsabeamformer_amd import _lib

    b.build()
    return _lib.load()


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def _tree_sum(vals):
    """The operand tree of the recursion over one cell's samples (row order): halves, each summed the same way, fp32."""
    if len(vals) == 1:
        return vals[0]
    h = len(vals) // 2
    return np.float32(_tree_sum(vals[:h]) + _tree_sum(vals[h:]))


@pytest.mark.parametrize("length,p", [(100, 9), (64, 8), (200, 13), (70, 33)])
def test_the_oracles_fold_is_the_cell_by_cell_sum_of_the_samples_the_recursion_implies(length, p):
    """Every cell of every final row, summed directly in Python over the sample indices of fold_indices -- first half of the rows
    plus second half, recursively, which is the recursion's operand tree -- equals the vectorised fold bit for bit; the same
    samples added left to right do not (about half the cells differ)."""
    y = ffa_oracle.parity_input(length * 1000 + p, 1, length, 2)
    M = ffa_oracle.rows_of(length, p)
    assert M >= 2
    prof = ffa_oracle.fold(y, p)
    idx = ffa_oracle.fold_indices(M, p)
    assert prof.shape == (1, M, p, 2) and idx.shape == (M, p, M)
    direct = np.empty_like(prof)
    for i in range(M):
        for j in range(p):
            for b in range(2):
                direct[0, i, j, b] = _tree_sum([y[0, t, b] for t in idx[i, j]])
    assert np.array_equal(direct.view(np.uint32), prof.view(np.uint32))
    # entry r of a cell comes from row r, at bin (j + shift[i][r]) mod p
    sh = ffa_oracle.row_shifts(M)
    for i in range(M):
        assert np.array_equal(idx[i], np.arange(M)[None, :] * p + (np.arange(p)[:, None] + sh[i][None, :]) % p)
    if M > 2:
        left = ffa_oracle.fold_left(y, p)
        differ = np.mean(left.view(np.uint32) != prof.view(np.uint32))
        assert 0.2 < differ < 0.8, differ
        assert np.allclose(left, prof, rtol=1e-4, atol=np.abs(y).max() * 1e-5)     # the same sums, other roundings


@pytest.mark.parametrize("M", [2, 4, 8, 16, 64, 256])
def test_row_shifts(M):
    """Final row i rotates the M rows by 0 .. i: monotone, row 0 never moves, the last row by i -- so a pulse train of period
    p + i / (M - 1) stacks fully in row i."""
    sh = ffa_oracle.row_shifts(M)
    assert sh.shape == (M, M)
    assert np.all(sh[:, 0] == 0) and np.array_equal(sh[:, -1], np.arange(M))
    assert np.all(np.diff(sh, axis=1) >= 0) and np.all(np.diff(sh, axis=1) <= 1)
    assert np.array_equal(sh[0], np.zeros(M, np.int64)) and np.array_equal(sh[-1], np.arange(M))


def test_a_pulse_train_stacks_in_its_row():
    M, p = 16, 20
    for i in (0, 5, 15):
        y = np.zeros((1, M * p + 7, 1), np.float32)
        sh = ffa_oracle.row_shifts(M)[i]
        y[0, np.arange(M) * p + (3 + sh) % p, 0] = 1.0
        prof = ffa_oracle.fold(y, p)[0, :, :, 0]
        assert prof[i, 3] == M and np.count_nonzero(prof == M) == 1


def test_every_parity_input_tells_a_left_fold_from_the_contract():
    """The inputs of tests/test_gpu_ffa.py: on each, a kernel that added the rows left to right would leave other record bits."""
    for name in sorted(PARITY_CASES):
        _, _, n_seg, p_lo, p_hi, tdec, n_oct, K, *_ = PARITY_CASES[name]
        assert ffa_oracle.association_matters(case_input(name), tdec, n_seg, n_oct, p_lo, p_hi, K), name
    x = ffa_oracle.parity_input(5, 2, 3 * 64, 64)                      # test_back_pressure_and_collect_order
    assert ffa_oracle.association_matters(x, 1, 64, 1, 8, 13, 2)


def test_every_edge_input_tells_a_left_fold_from_the_contract():
    """The inputs of tests/test_gpu_ffa_shapes.py, timed_geometry included.  max_seg is exempt: at M = 2048 fold_left's index table
    is 2048 x 8 x 2048 int64, 268 MB; that case is there for its addressing (LDS size, rows, octaves), not for the association, which
    max_seg_p511 covers at the same n_seg with M = 32."""
    asked = [name for name in sorted(EDGE_CASES) if case_max_rows(name) <= 512]
    assert sorted(set(EDGE_CASES) - set(asked)) == ["max_seg"]
    for name in asked:
        assert ffa_oracle.association_matters(case_input(name), *case_cfg(name)), name


def test_the_long_decimation_groups_depend_on_the_order_of_their_adds():
    """tdec 200 and 256: the same groups added in descending time give other bits in most decimated samples, so a kernel that
    added a group in another order -- the carried part last, say -- would not pass on these inputs."""
    for name in ("tdec200", "tdec256"):
        tdec = case_cfg(name)[0]
        x = case_input(name)
        n = x.shape[1] // tdec
        groups = x[:, :n * tdec].reshape(x.shape[0], n, tdec, x.shape[2])
        back = np.ascontiguousarray(groups[:, :, ::-1]).reshape(x.shape[0], n * tdec, x.shape[2])
        differ = np.mean(ffa_oracle.decimate(x, tdec).view(np.uint32) != ffa_oracle.decimate(back, tdec).view(np.uint32))
        assert differ > 0.5, (name, differ)


def test_the_edge_cases_sit_on_the_launchers_edges(lib):
    """The dynamic LDS of ffa_search_kernel as launch_search_octave sizes it, 2 ((max_p M p + 3) & ~3) 4 bytes with M from
    bf_ffa_rows_of, against the 48 KiB above which the launcher must raise hipFuncAttributeMaxDynamicSharedMemorySize.  Whoever
    retunes the launcher learns here that the cases have left the edge."""
    lds = {name: case_lds_bytes(name, lib.bf_ffa_rows_of) for name in EDGE_CASES}
    assert lds["lds_48k_exact"] == 48 * 1024 and lds["lds_just_over"] == 48 * 1024 + 128
    for name in ("lds_just_over", "timed_geometry", "max_seg", "max_seg_p511"):
        assert lds[name] > 48 * 1024, name
    assert (lds["timed_geometry"], lds["max_seg"], lds["max_seg_p511"]) == (64 * 1024, 128 * 1024, 130816)
    # lds_just_over alone is above 48 KiB with two widths: the first launch of ffa_search_kernel<2> that needs the opt-in, in any order
    assert [name for name in sorted(EDGE_CASES) if EDGE_CASES[name][7] == 2 and lds[name] > 48 * 1024] == ["lds_just_over"]
    small = [name for name in sorted(EDGE_CASES) if name.startswith("k")]
    assert len(small) == 6 and sorted(EDGE_CASES[name][7] for name in small) == [1, 2, 3, 4, 5, 6]
    for name in small:
        assert lds[name] <= 4096, name
    # every case is one bf_ffa_create takes: each bound of the contract, and two rows at least in every octave
    for name, (_, _, n_seg, p_lo, p_hi, tdec, n_oct, K, *_rest) in EDGE_CASES.items():
        assert 1 <= tdec <= 256 and n_seg <= 16384 and n_seg % (1 << (n_oct - 1)) == 0 and 8 <= p_lo < p_hi <= 512 and (1 << (K - 1)) <= p_lo // 2, name
        assert all(lib.bf_ffa_rows_of(n_seg >> o, p) >= 2 for o in range(n_oct) for p in range(p_lo, p_hi)), name
    assert case_max_rows("max_seg") == 2048


def test_decimation_and_octaves():
    x = ffa_oracle.parity_input(3, 2, 50, 4)
    y = ffa_oracle.decimate(x, 3)
    assert y.shape == (2, 16, 4)
    want = np.float32(np.float32(x[1, 6, 2] + x[1, 7, 2]) + x[1, 8, 2])
    assert y[1, 2, 2].tobytes() == want.tobytes()
    assert np.array_equal(ffa_oracle.decimate(x, 1).view(np.uint32), x.view(np.uint32))
    o = ffa_oracle.octaves(y, 3)
    assert [a.shape[1] for a in o] == [16, 8, 4]
    assert o[2][0, 1, 0].tobytes() == np.float32(np.float32(y[0, 4, 0] + y[0, 5, 0]) + np.float32(y[0, 6, 0] + y[0, 7, 0])).tobytes()


# ---- the library's host functions -----------------------------------------------------------------------------------------
def test_rows_of_and_entries(lib):
    for length in (0, 1, 7, 8, 15, 16, 64, 96, 100, 1000, 8192, 16384):
        for p in (8, 9, 12, 13, 31, 48, 64, 127, 512):
            assert lib.bf_ffa_rows_of(length, p) == ffa_oracle.rows_of(length, p), (length, p)
    assert lib.bf_ffa_rows_of(100, 0) == 0 and lib.bf_ffa_rows_of(-5, 8) == 0
    assert lib.bf_ffa_rows_of(8192, 64) == 128 and lib.bf_ffa_rows_of(8192, 65) == 64 and lib.bf_ffa_rows_of(96, 48) == 2
    assert lib.bf_ffa_entries(3, 64, 128, 5, 64, 256) == 3 * 64 * 5 * 64 * 256
    bad = [(0, 8, 13, 1, 1, 4), (7, 8, 13, 1, 1, 4), (1, 7, 13, 1, 1, 4), (1, 8, 8, 1, 1, 4), (1, 8, 513, 1, 1, 4), (1, 8, 13, 0, 1, 4), (1, 8, 13, 7, 1, 4),
           (1, 8, 13, 1, 0, 4), (1, 8, 13, 1, 1, 0)]
    assert [lib.bf_ffa_entries(*a) for a in bad] == [0] * len(bad)


def _lib_select(value, shift, bin_, ssum, ssq, tdec, n_seg, p_lo, first_row, dm_first, threshold):
    from dsabeamformer_amd import api

    return api.PeriodicitySearch.select((value, shift, bin_), (ssum, ssq), tdec, n_seg, p_lo, first_row, dm_first, threshold)


def _records(rng, n_oct, n_p, K, n_dm, n_b, n_seg):
    shape = (n_oct, n_p, K, n_dm, n_b)
    value = (rng.standard_normal(shape) * 50 + 10).astype(np.float32)
    shift = rng.integers(0, 2, shape).astype(np.uint16)
    bin_ = rng.integers(0, 8, shape).astype(np.uint16)
    ssum = rng.standard_normal((n_dm, n_b)) * n_seg
    ssq = np.abs(rng.standard_normal((n_dm, n_b))) * n_seg + ssum * ssum / n_seg + 1.0
    return value, shift, bin_, ssum, ssq


def test_select_is_the_oracles_to_the_bit_on_random_records(lib):
    rng = np.random.default_rng(2)
    n_cands = 0
    for n_oct, p_lo, p_hi, K, n_dm, n_b, tdec, n_seg, thr in ((1, 8, 13, 1, 2, 4, 1, 64, -1e300), (3, 13, 32, 3, 3, 8, 4, 1000, 2.0), (2, 32, 64, 5, 1, 12, 2, 4096, 5.0),
                                                                (6, 8, 9, 3, 2, 4, 256, 16384, 0.0)):
        rec = _records(rng, n_oct, p_hi - p_lo, K, n_dm, n_b, n_seg)
        want = ffa_oracle.select(*rec, tdec, n_seg, p_lo, first_row=2 ** 41 + 3, dm_first=9, threshold=thr)
        got = _lib_select(*rec, tdec, n_seg, p_lo, 2 ** 41 + 3, 9, thr)
        ffa_oracle.assert_candidates_equal(got, want)
        assert got.dtype == ffa_oracle.CAND_DTYPE
        n_cands += len(want)
        if thr == -1e300:
            assert len(want) == n_dm * n_b and [(c[3], c[4]) for c in want] == [(9 + d, b) for d in range(n_dm) for b in range(n_b)]
    assert n_cands > 20


def test_select_ties_zero_deviation_and_the_threshold_to_one_ulp(lib):
    """Hand-built records of one (trial, beam) pair each.  Equal S/N at two octaves, two periods, two widths: the lowest octave,
    then the lowest period, then the lowest width is kept.  sigma == 0: no candidate.  The threshold met exactly: a candidate;
    one ulp above the S/N: none."""
    n_seg, tdec, p_lo = 256, 2, 8
    shape = (2, 2, 2, 1, 2)                        # octaves, p = 8 and 9, widths 1 and 2, one trial, two beams
    ssum = np.array([[0.0, 512.0]])
    ssq = np.array([[256.0, 1024.0 + 256.0]])      # beam 0: mu 0, sigma 1; beam 1: mu 2, sigma 1
    # with mu = 0 the S/N is value / (sqrt(2^o) sqrt(w M)): M = 32, 16 at octave 0 (p = 8, 9) and 16, 8 at octave 1
    M = np.array([[ffa_oracle.rows_of(n_seg >> o, p) for p in (8, 9)] for o in range(2)])
    assert M.tolist() == [[32, 16], [16, 8]]

    def cands(value, thr=-1e300, s=ssum, q=ssq):
        z = np.zeros(shape, np.uint16)
        sh = z.copy()
        sh[...] = 3
        want = ffa_oracle.select(value, sh, z, s, q, tdec, n_seg, p_lo, 7, 0, thr)
        got = _lib_select(value, sh, z, s, q, tdec, n_seg, p_lo, 7, 0, thr)
        ffa_oracle.assert_candidates_equal(got, want)
        return got

    flat = np.full(shape, -1e30, np.float32)
    # the octave tie: value so that snr = 4 at (o 0, p 8, k 1: w M = 64) and at (o 1, p 8, k 1: sqrt(2) sqrt(32) = 8) -- both exact
    v = flat.copy()
    v[0, 0, 1, 0, 0], v[1, 0, 1, 0, 0] = 32.0, 32.0
    got = cands(v)
    assert (got["octave"][0], got["p"][0], got["width"][0], got["snr"][0]) == (0, 8, 2, 4.0)
    assert got["period_rows"][0] == 2.0 * (8.0 + 3.0 / 31.0) and got["first_row"][0] == 7 and got["n_rows"][0] == 512
    # the period tie: (o 0, p 8, k 0: w M = 32) and (o 0, p 9, k 1: w M = 32)
    v = flat.copy()
    v[0, 0, 0, 0, 0], v[0, 1, 1, 0, 0] = 40.0, 40.0
    got = cands(v)
    assert (got["octave"][0], got["p"][0], got["width"][0]) == (0, 8, 1)
    # the width tie needs mu != 0 (w M differs between widths): beam 1, mu = 2: (v - w M 2) / sqrt(w M), w M = 16 and 32 at (o 0, p 9)
    v = flat.copy()
    v[0, 1, 0, 0, 1] = 32.0 + 4.0 * 3.0                    # snr 3 at k 0
    v[0, 1, 1, 0, 1] = np.float32(64.0 + math.sqrt(32.0) * 3.0)
    got = cands(v)
    one = got[got["beam"] == 1]
    k1 = (float(v[0, 1, 1, 0, 1]) - 64.0) / (1.0 * math.sqrt(32.0))
    assert (one["p"][0], one["width"][0]) == ((9, 1) if k1 <= 3.0 else (9, 2))
    v[0, 1, 1, 0, 1] = v[0, 1, 0, 0, 1]                    # ... and plainly lower at k 1: k 0 stays
    assert cands(v)[-1]["width"] == 1
    # sigma == 0 (sumsq / n == mu^2): the series is skipped, whatever the records say
    got = cands(np.full(shape, 1e30, np.float32), s=np.array([[512.0, 0.0]]), q=np.array([[1024.0, 0.0]]))
    assert len(got) == 0
    # the threshold met exactly, and missed by one ulp
    v = flat.copy()
    v[0, 0, 1, 0, 0] = 36.0                                # snr 4.5 exactly
    assert len(cands(v, thr=4.5)) == 1 and len(cands(v, thr=math.nextafter(4.5, 5.0))) == 0
    assert len(cands(v, thr=math.nextafter(4.5, 0.0))) == 1


def test_select_refusals(lib):
    pk = np.zeros((1, 5, 1, 1, 4), ffa_oracle.PEAK_DTYPE)
    st = np.ones((1, 4), ffa_oracle.STAT_DTYPE)
    out = np.zeros(4, ffa_oracle.CAND_DTYPE)
    n = C.c_size_t()

    def sel(peaks=pk, stats=st, tdec=1, n_seg=64, n_oct=1, p_lo=8, p_hi=13, K=1, n_dm=1, n_b=4, o=out, max_out=4, n_out=n):
        return lib.bf_ffa_select(peaks.ctypes.data if peaks is not None else None, stats.ctypes.data if stats is not None else None, tdec, n_seg, n_oct,
                                 p_lo, p_hi, K, n_dm, n_b, 0, 64, 0, -1e300, o.ctypes.data if o is not None else None, max_out,
                                 C.byref(n_out) if n_out is not None else None)

    assert sel() == 0 and n.value == 4
    for kw in (dict(peaks=None), dict(stats=None), dict(o=None), dict(n_out=None), dict(tdec=0), dict(n_seg=16385), dict(n_oct=7), dict(p_lo=7), dict(K=4),
               dict(n_dm=0), dict(n_b=0), dict(p_hi=40), dict(max_out=3)):
        assert sel(**kw) == BF_ERR_INVALID, kw


def test_creation_refusals_that_need_no_device(lib):
    def create(n_dm=2, dm_first=0, tdec=2, n_seg=64, n_oct=1, p_lo=8, p_hi=13, K=2, max_t=16, in_flight=2, thr=8.0, out=True):
        s = C.c_void_p()
        rc = lib.bf_ffa_create(None, n_dm, dm_first, tdec, n_seg, n_oct, p_lo, p_hi, K, max_t, in_flight, thr, C.byref(s) if out else None)
        assert not s.value
        return rc, lib.bf_last_error()

    for kw, msg in ((dict(tdec=0), b"tdec"), (dict(tdec=257), b"tdec"), (dict(n_seg=0), b"n_seg"), (dict(n_seg=16385), b"n_seg"), (dict(n_oct=0), b"n_oct"),
                    (dict(n_oct=7), b"n_oct"), (dict(n_oct=2, n_seg=63, p_hi=9), b"no multiple"), (dict(p_lo=7), b"p_lo"), (dict(p_hi=8), b"p_lo"),
                    (dict(p_hi=513, n_seg=16384), b"p_lo"), (dict(K=0), b"n_widths"), (dict(K=7, p_lo=200, p_hi=201, n_seg=4096), b"n_widths"),
                    (dict(K=4), b"n_widths"), (dict(p_hi=34), b"fewer than 2 rows"), (dict(n_oct=3, p_hi=10), b"fewer than 2 rows"),
                    (dict(n_dm=0), b"n_dm"), (dict(n_dm=65536), b"n_dm"), (dict(dm_first=-1), b"dm_first"), (dict(max_t=0), b"max_t_per_push"),
                    (dict(in_flight=0), b"max_in_flight"), (dict(thr=float("nan")), b"NaN"), (dict(out=False), b"out is NULL")):
        rc, err = create(**kw)
        assert rc == BF_ERR_INVALID and msg in err, (kw, err)
    # everything in range, at every bound: what is left to refuse is the missing handle
    for kw in (dict(), dict(tdec=1), dict(tdec=256), dict(n_seg=16384, p_lo=8, p_hi=257, n_oct=6, K=3), dict(n_seg=16384, p_lo=256, p_hi=512, K=6), dict(K=6, p_lo=64, p_hi=65, n_seg=1024),
               dict(p_lo=16, p_hi=33, n_seg=64)):
        rc, err = create(**kw)
        assert rc == BF_ERR_INVALID and b"handle is NULL" in err, (kw, err)
    for call in (lambda: lib.bf_ffa_push(None, None, 1, 0, None), lambda: lib.bf_ffa_pending(None), lambda: lib.bf_ffa_collect(None, None, 0, None),
                 lambda: lib.bf_ffa_last_records(None, None, None, None, None), lambda: lib.bf_dm_stream_attach_periodicity(None, None)):
        assert call() == BF_ERR_INVALID
    assert lib.bf_ffa_destroy(None) == 0


def test_the_lib_and_api_surface(lib):
    from dsabeamformer_amd import _lib, api

    for name in ("bf_ffa_entries", "bf_ffa_rows_of", "bf_ffa_create", "bf_ffa_destroy", "bf_ffa_push", "bf_ffa_collect", "bf_ffa_pending",
                 "bf_ffa_last_records", "bf_ffa_select", "bf_dm_stream_attach_periodicity", "bfh_ffa_sink_create", "bfh_ffa_sink_deliver",
                 "bfh_ffa_sink_destroy"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert C.sizeof(_lib.BfFfaPeak) == 8 == ffa_oracle.PEAK_DTYPE.itemsize and C.sizeof(_lib.BfFfaStat) == 16 == ffa_oracle.STAT_DTYPE.itemsize
    assert C.sizeof(_lib.BfFfaCandidate) == 72 == ffa_oracle.CAND_DTYPE.itemsize == api._ffa_candidate_dtype().itemsize
    for f, _ in _lib.BfFfaCandidate._fields_:
        assert getattr(_lib.BfFfaCandidate, f).offset == ffa_oracle.CAND_DTYPE.fields[f][1], f
    for attr in ("push", "collect", "pending", "last_records", "select", "rows_of"):
        assert hasattr(api.PeriodicitySearch, attr), attr
    assert hasattr(api.DmStream, "attach_periodicity")
    assert api.PeriodicitySearch.rows_of(1000, 13) == 64


def test_the_sink_file_reads_back_to_the_same_bits(lib, tmp_path):
    rng = np.random.default_rng(4)
    rec = _records(rng, 2, 5, 3, 3, 4, 256)
    want = ffa_oracle.select(*rec, 4, 256, 8, first_row=2 ** 40 + 1, dm_first=5, threshold=-1e300)
    got = _lib_select(*rec, 4, 256, 8, 2 ** 40 + 1, 5, -1e300)
    assert len(got) == 12
    path = str(tmp_path / "ffa.txt")
    s = C.c_void_p()
    assert lib.bfh_ffa_sink_create(path.encode(), 4, 256, 2, 8, 13, 3, 6.5, C.byref(s)) == 0
    assert lib.bfh_ffa_sink_deliver(s, got[:5].ctypes.data, 5) == 0 and lib.bfh_ffa_sink_deliver(s, got[5:].ctypes.data, 7) == 0
    assert lib.bfh_ffa_sink_deliver(s, None, 0) == 0 and lib.bfh_ffa_sink_deliver(s, None, 1) == BF_ERR_INVALID
    assert lib.bfh_ffa_sink_deliver(None, got.ctypes.data, 1) == BF_ERR_INVALID
    assert lib.bfh_ffa_sink_destroy(s) == 0
    head, rows = ffa_oracle.read_candidates(path)
    assert head == {"tdec": "4", "n_seg": "256", "n_oct": "2", "p_lo": "8", "p_hi": "13", "n_widths": "3", "threshold": "6.5"}
    assert open(path).read().splitlines()[1] == "# " + " ".join(ffa_oracle.CAND_FIELDS)
    back = np.zeros(len(rows), ffa_oracle.CAND_DTYPE)
    for i, f in enumerate(ffa_oracle.CAND_FIELDS):
        back[f] = [r[i] for r in rows]
    ffa_oracle.assert_candidates_equal(back, want)
    assert lib.bfh_ffa_sink_create(str(tmp_path / "no" / "such" / "dir").encode(), 4, 256, 2, 8, 13, 3, 6.5, C.byref(s)) == BF_ERR_INVALID
    assert lib.bfh_ffa_sink_create(None, 4, 256, 2, 8, 13, 3, 6.5, C.byref(s)) == BF_ERR_INVALID
