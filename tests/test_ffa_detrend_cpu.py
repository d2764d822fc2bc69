"""CPU tests of the periodicity search's detrend and harmonic sift (docs/PERIODICITY.md sections 1a and 1b): the oracle
tests/support/ffa_detrend_oracle.py by hand and against its own mutants on every input of the GPU tests, the red-noise case, the
refusals of bf_ffa_set_detrend that need no device, bf_ffa_sift field by field against the oracle, the `_lib` / `api` surface, the
struct layout and the sink's header line.  Integers are compared exactly, floats bit for bit."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import ffa_detrend_oracle as det  # noqa: E402
import ffa_oracle  # noqa: E402
from ffa_detrend_stage import (CASES, COVERS, RED_BEAM, RED_CFG, RED_DETREND, RED_PERIOD, best_per_beam, case_cfg, case_input,  # noqa: E402
                               red_noise_input)

BF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from dsabeamformer_amd import build as b
    from dsabeamformer_amd import _lib

    b.build()
    return _lib.load()


# ---- the detrend oracle ----------------------------------------------------------------------------------------------------------
def test_the_detrend_by_hand_on_sixteen_samples():
    """blk 4, win 3, nb 4.  Means 3, 1, 7, 5.  Windows: {3, 1} (clamped left, even: the LOWER median, 1), {3, 1, 7} -> 3,
    {1, 7, 5} -> 5, {7, 5} (clamped right, even) -> 5.  k = 2u - 3: u 0, 1 before the first centre (r[0]); u 2 .. 5 between centres
    0 and 1 with a = 1/8 (the smallest), 3/8, 5/8, 7/8 (the largest); u 6 .. 9 between 1 and 2; u 10 .. 13 between 2 and 3 (flat);
    u 14, 15 behind the last centre (c0 = 3 >= nb - 1: r[3])."""
    y = np.array([1, 2, 4, 5, 0, 1, 1, 2, 7, 7, 6, 8, 5, 4, 6, 5], np.float32)
    seg = y.reshape(1, 16, 1)
    assert np.array_equal(det.block_means(seg, 4)[0, :, 0], [3, 1, 7, 5])
    r = det.running_median(det.block_means(seg, 4), 3)
    assert np.array_equal(r[0, :, 0], [1, 3, 5, 5])
    assert np.array_equal(det.running_median(det.block_means(seg, 4), 3, upper=True)[0, :, 0], [3, 3, 5, 7])
    trend = np.array([1, 1, 1.25, 1.75, 2.25, 2.75, 3.25, 3.75, 4.25, 4.75, 5, 5, 5, 5, 5, 5], np.float32)
    assert np.array_equal(det.trend_of(r, 16, 4)[0, :, 0], trend)
    assert np.array_equal(det.detrend(seg, 4, 3)[0, :, 0], y - trend)
    assert np.array_equal(det.detrend(seg, 4, 3, mutant="constant")[0, :, 0], y - np.repeat(np.float32([1, 3, 5, 5]), 4))
    # win 1: r = m; blk 16: one block, its mean everywhere
    assert np.array_equal(det.running_median(det.block_means(seg, 4), 1)[0, :, 0], [3, 1, 7, 5])
    assert np.array_equal(det.detrend(seg, 16, 5)[0, :, 0], y - np.float32(y.sum() / 16))


def test_the_order_of_the_median_puts_minus_zero_below_plus_zero_and_selects_bits():
    m = np.array([0.0, -0.0, -0.0, 0.0, -1.0, 1.0], np.float32).reshape(1, 6, 1)
    k = det.keys(m)[0, :, 0]
    assert k[1] < k[0] and k[4] < k[1] and k[0] < k[5]
    assert np.array_equal(det.unkeys(det.keys(m)).view(np.uint32), m.view(np.uint32))
    r = det.running_median(m, 3)[0, :, 0]          # windows {+0,-0} {+0,-0,-0} {-0,-0,+0} {-0,+0,-1} {+0,-1,1} {-1,1}
    assert np.array_equal(r.view(np.uint32), np.array([-0.0, -0.0, -0.0, -0.0, 0.0, -1.0], np.float32).view(np.uint32))
    # three roundings against one.  r0 = 1 + 2^-23, r1 = 4 - 2^-22, a = 3/4 (blk 2, u = 2): r1 - r0 = 3 - 3 2^-23 lies half way between
    # two fp32 of [2, 4) and rounds to the even one, d = 3 - 2^-21; q = 9/4 - 3 2^-22 is exact; r0 + q = 13/4 - 5/2 2^-22 is a tie again
    # and rounds to 13/4 - 2 2^-22.  Unrounded, r0 + a (r1 - r0) = 13/4 - 5/8 2^-22 rounds to 13/4 - 2^-22: the last bit differs.
    r2 = np.array([1.0 + 2.0 ** -23, 4.0 - 2.0 ** -22], np.float32).reshape(1, 2, 1)
    three, one = det.trend_of(r2, 4, 2)[0, 2, 0], det.trend_of(r2, 4, 2, fused=True)[0, 2, 0]
    assert (float(three).hex(), float(one).hex()) == ("0x1.9ffffc0000000p+1", "0x1.9ffffe0000000p+1")


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_gpu_input_tells_each_mutant_from_the_contract_where_the_table_says_so(case):
    """For every parity input of tests/test_gpu_ffa_detrend.py: the upper median, the piecewise-constant trend and the singly
    rounded interpolation change sample bits in every segment of the cases that ffa_detrend_stage.COVERS lists for them -- and
    change nothing in the others, which are therefore no test of that rule (the table says why).  The upper median differs from
    the lower one in windows of even count only, the truncated ones: with win <= nb it changes samples within h blocks and half a
    block of an end and nowhere else."""
    (tdec, n_seg, *_), (blk, win) = case_cfg(case)
    x = case_input(case)
    for mutant in ("upper", "constant", "fused"):
        changes = det.mutant_changes(x, tdec, n_seg, blk, win, mutant)
        assert len(changes) >= 1
        print("detrend %s, mutant %s: %s of the samples change" % (case, mutant, ", ".join("%.1f %%" % (100 * f) for _, f in changes)))
        for where, frac in changes:
            assert bool(where.any()) == (case in COVERS[mutant]), (case, mutant, frac)
            if mutant == "upper" and win <= n_seg // blk:
                h = (win - 1) // 2
                edge = h * blk + blk // 2          # block c shapes the trend between the centres of c - 1 and c + 1
                assert not where[edge:n_seg - edge].any()
    assert all(any(case in COVERS[m] for m in COVERS) for case in CASES if case != "one_block")


def test_red_noise_buries_a_pulse_train_and_the_detrend_recovers_it():
    """docs/PERIODICITY.md section 1a: unit noise, 40 sin(2 pi t / 700) and half a random walk in four beams, a train of height 4
    at period 19.37 in one of them.  Detrended (blk 8, win 9) the train is the best candidate of its beam at S/N >= 8 within
    1 / (M - 1) of its period; on the raw series no beam reaches 8."""
    x = red_noise_input()
    raw = best_per_beam(ffa_oracle.Search(x, *RED_CFG, threshold=-1e300).segments()[0]["cands"])
    got = best_per_beam(det.Search(x, *RED_CFG, *RED_DETREND, threshold=-1e300).segments()[0]["cands"])
    print("red noise: raw %s; detrended %s" % (raw, got))
    snr, period = got[RED_BEAM]
    M = ffa_oracle.rows_of(RED_CFG[1], int(period))
    assert snr >= 8.0 and abs(period - RED_PERIOD) <= 1.0 / (M - 1)
    assert all(s < 8.0 for s, _ in raw.values()) and len(raw) == 4
    assert all(s < 8.0 for b, (s, _) in got.items() if b != RED_BEAM)


# ---- bf_ffa_set_detrend ----------------------------------------------------------------------------------------------------------
def test_set_detrend_refusals_that_need_no_device(lib):
    for blk, win, msg in ((3, 3, b"power of two"), (-1, 3, b"power of two"), (512, 3, b"power of two"), (6, 3, b"power of two"), (8, 0, b"odd"),
                          (8, 4, b"odd"), (8, 131, b"odd"), (8, -3, b"odd"), (1, 2, b"odd")):
        assert lib.bf_ffa_set_detrend(None, blk, win) == BF_ERR_INVALID and msg in lib.bf_last_error(), (blk, win, lib.bf_last_error())
    # everything in range, at every bound: what is left to refuse is the missing stage
    for blk, win in ((0, 0), (0, 7), (1, 1), (256, 129), (8, 9)):
        assert lib.bf_ffa_set_detrend(None, blk, win) == BF_ERR_INVALID and b"stage is NULL" in lib.bf_last_error()
    blk, win = C.c_int(), C.c_int()
    assert lib.bf_ffa_detrend(None, C.byref(blk), C.byref(win)) == BF_ERR_INVALID


# ---- bf_ffa_sift -----------------------------------------------------------------------------------------------------------------
def _cands(rows):
    """CAND_DTYPE array from (period_rows, dm, beam, snr[, first_row]) tuples."""
    out = np.zeros(len(rows), ffa_oracle.CAND_DTYPE)
    for i, r in enumerate(rows):
        out[i]["period_rows"], out[i]["dm"], out[i]["beam"], out[i]["snr"] = r[:4]
        out[i]["first_row"], out[i]["n_rows"] = (r[4] if len(r) > 4 else 0), 4096
        out[i]["p"], out[i]["width"], out[i]["value"], out[i]["shift"] = 8 + i % 5, 1 << (i % 3), i * 0.5, i % 7
    return out


def _sift(lib, cands, tol, max_harm, dm_tol, max_out=None):
    out = np.zeros(max(len(cands), 1), det.GROUP_DTYPE)
    n = C.c_size_t(77)
    rc = lib.bf_ffa_sift(cands.ctypes.data if len(cands) else None, len(cands), tol, max_harm, dm_tol, out.ctypes.data,
                         len(cands) if max_out is None else max_out, C.byref(n))
    return rc, out[:n.value], out


def _check_sift(lib, cands, tol, max_harm, dm_tol):
    """The library's groups against the oracle's, field by field; returns the oracle's."""
    rc, got, _ = _sift(lib, cands, tol, max_harm, dm_tol)
    want = det.sift(cands, tol, max_harm, dm_tol)
    assert rc == 0 and len(got) == len(want), (rc, len(got), len(want))
    for g, w in zip(got, want):
        for f in ffa_oracle.CAND_FIELDS:
            assert g["head"][f].tobytes() == cands[w["head"]][f].tobytes(), f
        assert [int(g[f]) for f in det.GROUP_FIELDS] == [w["n_members"], w["n_beams"], w["dm_lo"], w["dm_hi"], w["n_harmonic"], 0]
    assert sum(w["n_members"] for w in want) == len(cands)
    return want


def test_sift_groups_neighbours_beams_and_harmonics(lib):
    # one source at period 100: the fundamental in three trials and two beams, 2:1, 1:2 and 3:2 of it; a stranger at 137
    c = _cands([(100.0, 10, 3, 30.0), (100.05, 11, 3, 25.0), (99.95, 9, 4, 22.0), (200.0, 10, 3, 12.0), (50.0, 10, 5, 11.0), (150.0, 12, 3, 9.0),
                (137.0, 10, 3, 8.5)])
    w = _check_sift(lib, c, 1e-3, 4, 2)
    assert [(g["head"], g["n_members"], g["n_beams"], g["dm_lo"], g["dm_hi"], g["n_harmonic"]) for g in w] == [(0, 6, 3, 9, 12, 3), (6, 1, 1, 10, 10, 0)]
    # max_harm 1: the three harmonics are heads of their own
    w = _check_sift(lib, c, 1e-3, 1, 2)
    assert [g["n_members"] for g in w] == [3, 1, 1, 1, 1] and all(g["n_harmonic"] == 0 for g in w)
    # 3:2 needs max_harm >= 3
    assert [g["n_members"] for g in _check_sift(lib, c, 1e-3, 2, 2)] == [5, 1, 1]


def test_sift_edges(lib):
    # tol met exactly, and exceeded by one ulp: 1028 / 1024 - 1 is 2^-8 in fp64, exactly
    c = _cands([(1024.0, 5, 0, 20.0), (1028.0, 5, 1, 10.0)])
    assert (1028.0 * 1.0) / (1024.0 * 1.0) - 1.0 == 2.0 ** -8
    assert len(_check_sift(lib, c, 2.0 ** -8, 3, 0)) == 1 and len(_check_sift(lib, c, math.nextafter(2.0 ** -8, 0.0), 3, 0)) == 2
    # ... and below the head: 1020 / 1024 - 1 = -2^-8 + ... is exact too (1 - 2^-8 needs 8 bits)
    c = _cands([(1024.0, 5, 0, 20.0), (1020.0, 5, 1, 10.0)])
    assert len(_check_sift(lib, c, 2.0 ** -8, 1, 0)) == 1 and len(_check_sift(lib, c, math.nextafter(2.0 ** -8, 0.0), 1, 0)) == 2
    # dm_tol at equality and one beyond, on both sides
    c = _cands([(100.0, 10, 0, 20.0), (100.0, 13, 0, 10.0), (100.0, 7, 0, 9.0)])
    assert len(_check_sift(lib, c, 0.0, 1, 3)) == 1 and len(_check_sift(lib, c, 0.0, 1, 2)) == 3
    # links are to heads only: 13 and 7 are within 3 of 10, not of each other -- and with dm_tol 2 the trial 7 does not reach 13 through 10
    assert [g["head"] for g in _check_sift(lib, c, 0.0, 1, 2)] == [0, 1, 2]
    # an snr tie: the lower input index is taken first and becomes the head
    c = _cands([(100.0, 10, 0, 9.0), (100.0, 10, 1, 15.0), (100.0, 10, 2, 15.0)])
    w = _check_sift(lib, c, 0.0, 1, 0)
    assert len(w) == 1 and w[0]["head"] == 1
    # two segments are never grouped
    c = _cands([(100.0, 10, 0, 20.0, 0), (100.0, 10, 0, 10.0, 4096)])
    assert len(_check_sift(lib, c, 0.5, 4, 5)) == 2
    c["first_row"][1], c["n_rows"][1] = 0, 8192
    assert len(_check_sift(lib, c, 0.5, 4, 5)) == 2
    # a candidate that matches two heads joins the earlier one: 200 is 2:1 of the head at 100 and 1:2 of the head at 400
    c = _cands([(100.0, 10, 0, 20.0), (400.0, 10, 0, 18.0), (200.0, 10, 0, 10.0)])
    w = _check_sift(lib, c, 1e-6, 2, 0)
    assert [(g["head"], g["n_members"], g["n_harmonic"]) for g in w] == [(0, 2, 1), (1, 1, 0)]
    c["snr"][0], c["snr"][1] = 18.0, 20.0                       # ... whichever was created first
    w = _check_sift(lib, c, 1e-6, 2, 0)
    assert [(g["head"], g["n_members"], g["n_harmonic"]) for g in w] == [(1, 2, 1), (0, 1, 0)]


def test_sift_on_two_thousand_random_candidates(lib):
    rng = np.random.default_rng(9)
    n = 2000
    jitter = np.where(rng.random(n) < 0.5, 0.0, rng.normal(0, 4e-4, n))            # half of them exactly on a harmonic: tol 0 groups those
    base = rng.choice([64.0, 81.3, 100.0, 173.7], n) * rng.choice([0.5, 1.0, 1.5, 2.0, 3.0, 1.0 / 3.0], n) * (1.0 + jitter)
    rows = list(zip(base, rng.integers(0, 24, n), rng.integers(0, 8, n), np.round(rng.uniform(8, 30, n), 1), rng.integers(0, 3, n) * 4096))
    c = _cands(rows)
    for tol, max_harm, dm_tol in ((1e-3, 4, 2), (2e-4, 16, 0), (0.0, 1, 23), (0.3, 2, 1)):
        w = _check_sift(lib, c, tol, max_harm, dm_tol)
        print("sift %g %d %d: %d candidates in %d groups, the largest of %d" % (tol, max_harm, dm_tol, n, len(w), max(g["n_members"] for g in w)))
        assert 1 < len(w) < n


def test_sift_refusals(lib):
    c = _cands([(100.0, 10, 0, 20.0), (137.0, 10, 0, 10.0)])
    rc, got, _ = _sift(lib, c, 1e-3, 4, 2)
    assert rc == 0 and len(got) == 2
    for kw in (dict(tol=-1e-9), dict(tol=1.0), dict(tol=float("nan")), dict(max_harm=0), dict(max_harm=17), dict(dm_tol=-1), dict(max_out=1)):
        a = dict(dict(tol=1e-3, max_harm=4, dm_tol=2, max_out=None), **kw)
        rc, got, out = _sift(lib, c, a["tol"], a["max_harm"], a["dm_tol"], a["max_out"])
        assert rc == BF_ERR_INVALID and len(got) == 0 and not out.tobytes().strip(b"\0"), kw
    for field, v in (("snr", float("nan")), ("period_rows", 0.0), ("period_rows", -5.0), ("period_rows", float("nan"))):
        bad = c.copy()
        bad[field][1] = v
        rc, got, out = _sift(lib, bad, 1e-3, 4, 2)
        assert rc == BF_ERR_INVALID and len(got) == 0 and not out.tobytes().strip(b"\0"), (field, v)
    n = C.c_size_t(5)
    out = np.zeros(2, det.GROUP_DTYPE)
    assert lib.bf_ffa_sift(None, 2, 1e-3, 4, 2, out.ctypes.data, 2, C.byref(n)) == BF_ERR_INVALID and n.value == 0
    assert lib.bf_ffa_sift(c.ctypes.data, 2, 1e-3, 4, 2, None, 2, C.byref(n)) == BF_ERR_INVALID
    assert lib.bf_ffa_sift(c.ctypes.data, 2, 1e-3, 4, 2, out.ctypes.data, 2, None) == BF_ERR_INVALID
    # n == 0: BF_OK, no group, whatever the pointers
    n = C.c_size_t(5)
    assert lib.bf_ffa_sift(None, 0, 1e-3, 4, 2, None, 0, C.byref(n)) == 0 and n.value == 0
    # at every bound
    for tol, max_harm in ((0.0, 1), (math.nextafter(1.0, 0.0), 16)):
        assert _sift(lib, c, tol, max_harm, 0)[0] == 0


# ---- surface and layouts -----------------------------------------------------------------------------------------------------------
def test_the_lib_and_api_surface(lib):
    from dsabeamformer_amd import _lib, api

    for name in ("bf_ffa_set_detrend", "bf_ffa_detrend", "bf_ffa_sift", "bfh_ffa_sink_create_detrend"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert C.sizeof(_lib.BfFfaGroup) == 96 == det.GROUP_DTYPE.itemsize == api._ffa_group_dtype().itemsize
    for f, _ in _lib.BfFfaGroup._fields_:
        assert getattr(_lib.BfFfaGroup, f).offset == det.GROUP_DTYPE.fields[f][1] == api._ffa_group_dtype().fields[f][1], f
    for attr in ("sift", "detrend", "set_detrend"):
        assert hasattr(api.PeriodicitySearch, attr), attr
    assert isinstance(api.PeriodicitySearch.detrend, property)
    import inspect
    assert inspect.signature(api.PeriodicitySearch.__init__).parameters["detrend"].default is None
    c = _cands([(100.0, 10, 3, 30.0), (200.0, 11, 4, 25.0), (137.0, 10, 3, 8.5)])
    g = api.PeriodicitySearch.sift(c, tol=1e-3, max_harm=2, dm_tol=1)
    assert g.dtype == api._ffa_group_dtype() and [(int(x["n_members"]), int(x["n_beams"]), int(x["n_harmonic"])) for x in g] == [(2, 2, 1), (1, 1, 0)]
    assert g["head"]["period_rows"].tolist() == [100.0, 137.0]
    assert len(api.PeriodicitySearch.sift(c[:0])) == 0
    from dsabeamformer_amd import DsabfError
    with pytest.raises(DsabfError):
        api.PeriodicitySearch.sift(c, tol=1.5)


def test_the_sink_header_names_the_detrend_only_when_it_is_on(lib, tmp_path):
    args = (4, 256, 2, 8, 13, 3, 6.5)
    texts = {}
    for name, make in (("plain", lambda p, s: lib.bfh_ffa_sink_create(p, *args, C.byref(s))),
                       ("off", lambda p, s: lib.bfh_ffa_sink_create_detrend(p, *args, 0, 0, C.byref(s))),
                       ("on", lambda p, s: lib.bfh_ffa_sink_create_detrend(p, *args, 8, 5, C.byref(s)))):
        path, s = str(tmp_path / name), C.c_void_p()
        assert make(path.encode(), s) == 0
        c = _cands([(100.0, 10, 3, 30.0)])
        assert lib.bfh_ffa_sink_deliver(s, c.ctypes.data, 1) == 0 and lib.bfh_ffa_sink_destroy(s) == 0
        texts[name] = open(path, "rb").read()
    assert texts["plain"] == texts["off"] and b"detrend" not in texts["plain"]
    first, rest = texts["on"].split(b"\n", 1)
    assert first == texts["plain"].split(b"\n", 1)[0] + b" detrend=8:5" and rest == texts["plain"].split(b"\n", 1)[1]
    head, rows = ffa_oracle.read_candidates(str(tmp_path / "on"))
    assert head["detrend"] == "8:5" and head["threshold"] == "6.5" and len(rows) == 1
    s = C.c_void_p()
    assert lib.bfh_ffa_sink_create_detrend(None, *args, 8, 5, C.byref(s)) == BF_ERR_INVALID
    assert lib.bfh_ffa_sink_create_detrend(str(tmp_path / "no" / "dir").encode(), *args, 8, 5, C.byref(s)) == BF_ERR_INVALID
