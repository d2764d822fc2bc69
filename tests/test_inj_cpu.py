"""CPU tests of the pulse injector (include/dsabf.h: bf_inj_*; docs/INJECTION.md): the three host helpers against
tests/support/inj_oracle.py, the argument checks that need no device, and the oracle's own conditions on the inputs that
tests/test_gpu_inj.py uploads (tests/support/inj_cases.py) -- a GPU test that compares bits with an oracle shows something only where
the oracle's bits depend on what the contract fixes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import inj_cases  # noqa: E402
import inj_oracle  # noqa: E402
import psr_oracle  # noqa: E402

BF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def api():
    from dsabeamformer_amd import api as a
    from dsabeamformer_amd import build as b

    b.build()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from dsabeamformer_amd import _lib

    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def spacing_steps(a, b):
    """|a - b| in units of the fp32 spacing at the larger of the two (positive finite values, or both zero)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


# ---- bf_inj_burst_profile ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smear", [None, 1, 2, 5, "mixed"])
@pytest.mark.parametrize("W,centre,sigma", [(8, 3.5, 1.0), (64, 20.25, 3.7), (1, 0.0, 0.5), (257, 128.0, 11.0)])
def test_burst_profile_against_the_oracle(api, W, centre, sigma, smear):
    """One fp32 spacing per entry: exp comes from two math libraries, both within a few fp64 ulp of the true value, so the fp32
    roundings of the two results differ by at most one step.  Every channel sums to its fluence within W 2^-23 relative: W entries,
    each rounded to fp32 once (half a spacing, 2^-24 relative), summed here in fp64."""
    n_f = 6
    rng = np.random.default_rng(W)
    fluence = rng.uniform(0.5, 40.0, n_f)
    sm = {None: None, 1: 1, 2: 2, 5: 5, "mixed": np.array([1, 2, 5, 3, 1, 4], np.int32)}[smear]
    got = api.Injector.burst_profile(n_f, W, centre, sigma, fluence, smear=sm)
    want = inj_oracle.burst_profile(n_f, W, centre, sigma, fluence, smear=sm)
    assert got.dtype == np.float32 and got.shape == (n_f, W) and want is not None
    assert np.all(spacing_steps(got, want) <= 1.0), spacing_steps(got, want).max()
    assert np.all(got >= 0.0) and np.all(np.abs(got.astype(np.float64).sum(axis=1) - fluence) <= W * 2.0 ** -23 * fluence)
    if sm is None:                                  # no smearing is a smearing of one row, to the bit
        assert np.array_equal(bits(got), bits(api.Injector.burst_profile(n_f, W, centre, sigma, fluence, smear=1)))


def test_burst_profile_smearing_widens_and_keeps_the_centre(api):
    W, centre = 32, 15.5
    narrow = api.Injector.burst_profile(1, W, centre, 1.0, 10.0, smear=1)[0].astype(np.float64)
    wide = api.Injector.burst_profile(1, W, centre, 1.0, 10.0, smear=5)[0].astype(np.float64)
    t = np.arange(W)
    for p in (narrow, wide):
        assert abs((p * t).sum() / p.sum() - centre) < 1e-6        # the box is centred on the pulse
        assert np.allclose(p, p[::-1], rtol=1e-6, atol=1e-12)
    var = lambda p: (p * (t - centre) ** 2).sum() / p.sum()     # noqa: E731
    assert abs(var(narrow) - 1.0) < 0.1 and abs(var(wide) - (1.0 + (25 - 1) / 12.0)) < 0.1   # a box of 5 rows adds (5^2 - 1) / 12


def test_burst_profile_refusals(api, lib):
    from dsabeamformer_amd import DsabfError

    with pytest.raises(DsabfError, match="holds none of the pulse") as e:
        api.Injector.burst_profile(2, 8, 500.0, 1.0, 6.0)           # a window that misses the pulse: every exp underflows, N == 0
    assert e.value.code == BF_ERR_INVALID and inj_oracle.burst_profile(2, 8, 500.0, 1.0, 6.0) is None
    for centre, sigma, fluence, smear in ((3.5, 0.0, 6.0, None), (3.5, -1.0, 6.0, None), (3.5, float("nan"), 6.0, None), (float("nan"), 1.0, 6.0, None),
                                          (3.5, 1.0, float("nan"), None), (3.5, 1.0, 6.0, 0)):
        with pytest.raises(DsabfError) as e:
            api.Injector.burst_profile(2, 8, centre, sigma, fluence, smear=smear)
        assert e.value.code == BF_ERR_INVALID
        assert inj_oracle.burst_profile(2, 8, centre, sigma, fluence, smear=smear) is None
    out, fl = np.zeros(8, np.float32), np.ones(1)
    assert lib.bf_inj_burst_profile(1, 8, 3.5, 1.0, None, None, out.ctypes.data) == BF_ERR_INVALID
    assert lib.bf_inj_burst_profile(1, 8, 3.5, 1.0, None, fl.ctypes.data, None) == BF_ERR_INVALID
    assert lib.bf_inj_burst_profile(0, 8, 3.5, 1.0, None, fl.ctypes.data, out.ctypes.data) == BF_ERR_INVALID
    assert lib.bf_inj_burst_profile(1, 0, 3.5, 1.0, None, fl.ctypes.data, out.ctypes.data) == BF_ERR_INVALID


# ---- bf_inj_nearest_trial ---------------------------------------------------------------------------------------------------------
def test_nearest_trial_ties_go_to_the_lowest(api, lib):
    ladder = np.array([[d * (15 - f) for f in range(16)] for d in range(8)], np.int32)
    for d in range(8):
        assert api.Injector.nearest_trial(ladder, ladder[d]) == d == inj_oracle.nearest_trial(ladder, ladder[d])
    # half-way between trials 2 and 3 in every channel that differs: a tie, the lower trial
    two = np.array([[0, 0], [4, 2], [8, 4], [4, 2]], np.int32)
    assert api.Injector.nearest_trial(two, [6, 3]) == 1 == inj_oracle.nearest_trial(two, [6, 3])
    assert api.Injector.nearest_trial(two, [4, 2]) == 1                     # a repeated row: the first
    assert api.Injector.nearest_trial(two, [7, 3]) == 2
    rng = np.random.default_rng(3)
    for _ in range(20):
        lad = rng.integers(0, 2 ** 31 - 1, (11, 5)).astype(np.int32)        # the sum needs more than 32 bits
        d = rng.integers(0, 2 ** 31 - 1, 5).astype(np.int32)
        assert api.Injector.nearest_trial(lad, d) == inj_oracle.nearest_trial(lad, d)
    t = C.c_int()
    assert lib.bf_inj_nearest_trial(None, 1, 1, two.ctypes.data, C.byref(t)) == BF_ERR_INVALID
    assert lib.bf_inj_nearest_trial(two.ctypes.data, 0, 2, two.ctypes.data, C.byref(t)) == BF_ERR_INVALID


# ---- bf_inj_match -----------------------------------------------------------------------------------------------------------------
def cands_of(rows):
    from dsabeamformer_amd.api import _candidate_dtype

    out = np.zeros(len(rows), _candidate_dtype())
    for i, (t_start, dm, beam, width, snr) in enumerate(rows):
        out[i] = (t_start, dm, beam, width, 1.0, snr)
    return out


def test_match_on_hand_built_cases(api, lib):
    truth = [(100, 107, 5, 3)]
    both = lambda c, **kw: (list(api.Injector.match(truth, c, **kw)), list(inj_oracle.match(truth, c, **kw)))     # noqa: E731
    # the candidate's interval [t_start, t_start + width - 1] against [t_lo - t_tol, t_hi + t_tol], at the edges exactly
    for t_start, width, t_tol, hit in ((96, 4, 0, False), (96, 4, 1, True), (97, 4, 0, True), (107, 1, 0, True), (108, 2, 0, False), (108, 2, 1, True),
                                       (110, 1, 2, False), (110, 1, 3, True), (90, 8, 2, False), (90, 8, 3, True), (90, 64, 0, True)):
        got, want = both(cands_of([(t_start, 5, 3, width, 9.0)]), t_tol=t_tol)
        assert got == want == [0 if hit else -1], (t_start, width, t_tol)
    # the wrong beam, the wrong trial, the trial within dm_tol
    assert both(cands_of([(100, 5, 4, 2, 9.0)])) == ([-1], [-1])
    assert both(cands_of([(100, 6, 3, 2, 9.0)])) == ([-1], [-1])
    assert both(cands_of([(100, 6, 3, 2, 9.0)]), dm_tol=1) == ([0], [0])
    assert both(cands_of([(100, 3, 3, 2, 9.0)]), dm_tol=1) == ([-1], [-1])
    # the largest snr among the matches; a tie goes to the lower index; one that does not match does not count
    c = cands_of([(100, 5, 3, 2, 9.0), (101, 5, 3, 2, 12.5), (102, 5, 3, 1, 12.5), (103, 5, 2, 1, 99.0), (400, 5, 3, 1, 50.0)])
    assert both(c) == ([1], [1])
    # several truths, one candidate list; t_lo - t_tol below zero; no candidates at all
    truth = [(0, 3, 0, 0), (100, 107, 5, 3), (500, 500, 1, 1)]
    assert both(c, t_tol=10) == ([-1, 1, -1], [-1, 1, -1])
    assert both(cands_of([(2, 0, 0, 1, 8.5)]), t_tol=10) == ([0, -1, -1], [0, -1, -1])
    assert list(api.Injector.match(truth, cands_of([]))) == [-1, -1, -1]
    best = np.zeros(1, np.int32)
    assert lib.bf_inj_match(None, 1, c.ctypes.data, len(c), 0, 0, best.ctypes.data) == BF_ERR_INVALID
    assert lib.bf_inj_match(c.ctypes.data, 1, None, 1, 0, 0, best.ctypes.data) == BF_ERR_INVALID
    assert lib.bf_inj_match(c.ctypes.data, 1, c.ctypes.data, 1, 0, -1, best.ctypes.data) == BF_ERR_INVALID


# ---- the stage's argument checks that need no device -------------------------------------------------------------------------------
def test_null_pointers_and_bad_bounds_without_a_device(lib):
    s = C.c_void_p()
    assert lib.bf_inj_create(None, 16, 64, 8, 64, None) == BF_ERR_INVALID
    for n_f, max_rows, max_pulses, max_width, word in ((0, 64, 8, 64, b"n_freq_total"), (16, 0, 8, 64, b"max_rows_per_push"), (16, 64, 0, 64, b"max_pulses"),
                                                       (16, 64, 4097, 64, b"max_pulses"), (16, 64, 8, 0, b"max_width"), (16, 64, 8, 4097, b"max_width")):
        assert lib.bf_inj_create(None, n_f, max_rows, max_pulses, max_width, C.byref(s)) == BF_ERR_INVALID and not s.value
        assert word in lib.bf_last_error()
    assert lib.bf_inj_create(None, 16, 64, 8, 64, C.byref(s)) == BF_ERR_INVALID and b"handle is NULL" in lib.bf_last_error()
    pid = C.c_uint64()
    assert lib.bf_inj_add_burst(None, 0, 1, None, None, None, C.byref(pid)) == BF_ERR_INVALID
    assert lib.bf_inj_add_train(None, None, 0, 1, 2, None, None, None, C.byref(pid)) == BF_ERR_INVALID
    assert lib.bf_inj_apply(None, None, 1, None) == BF_ERR_INVALID
    assert lib.bf_dm_stream_attach_injector(None, None) == BF_ERR_INVALID
    assert lib.bf_inj_next_row(None) == 0 and lib.bf_inj_launches(None) == 0
    assert lib.bf_inj_destroy(None) == 0


# ---- the oracle's own checks: conditions on what the GPU tests upload ---------------------------------------------------------------
@pytest.mark.parametrize("case", inj_cases.BURST_CASES, ids=lambda c: "b%d-f%d-w%d" % c)
def test_burst_inputs_make_order_and_windows_show(case):
    c = inj_cases.burst_case(case)
    want = inj_cases.expected(c)
    # two of the three bursts overlap in cells, and adding them in the other order changes bits
    t = [inj_cases.touched_by(case[1], [b]) for b in c["bursts"]]
    assert (t[0] & t[1]).any()
    assert not np.array_equal(bits(want), bits(inj_cases.expected(c, reverse=True)))
    # the cut into applies does not show
    cuts = [n for _, n in inj_cases.cuts_of(inj_cases.N_ROWS, inj_cases.SIZES)]
    assert np.array_equal(bits(want), bits(inj_cases.expected(c, cuts=cuts)))
    # outside every window nothing changes -- the planted -0.0 and the NaN's payload included --, inside something does
    touched = inj_cases.touched_by(case[1], c["bursts"])
    assert np.array_equal(bits(want)[~touched], bits(c["x"])[~touched]) and not np.array_equal(bits(want)[touched], bits(c["x"])[touched])
    a, b = c["planted"]
    assert not touched[a] and not touched[b]
    assert np.all(bits(want[a]) == 0x80000000) and np.all(bits(want[b]) == inj_cases.NAN_BITS)
    # one channel of the third burst is never touched, one burst starts on a cut, and (W >= 3) one straddles the cuts at 105 and 106
    t0, delay, profile, _ = c["bursts"][2]
    assert not inj_cases.touched_by(case[1], [c["bursts"][2]])[:, case[1] // 2].any()
    assert t0 + int(delay.min()) + profile.shape[1] > inj_cases.N_ROWS or profile.shape[1] == 1      # it runs off the end
    assert c["bursts"][0][0] + int(c["bursts"][0][1].min()) == 105 in [at for at, _ in inj_cases.cuts_of(inj_cases.N_ROWS, inj_cases.SIZES)]
    if case[2] >= 3:
        assert t[1][104, 0] and t[1][105, 0] and t[1][106, 0]


@pytest.mark.parametrize("case", inj_cases.TRAIN_CASES, ids=lambda c: "b%d-f%d-bins%d-tr%d%s" % (c[0], c[1], c[2], c[3], "-" + c[4] if c[4] else ""))
def test_train_inputs_and_the_folders_bins(case):
    n_b, n_f, n_bins, n_tr, _ = case
    c = inj_cases.train_case(case)
    want = inj_cases.expected(c)
    cuts = [n for _, n in inj_cases.cuts_of(inj_cases.N_ROWS, inj_cases.SIZES)]
    assert np.array_equal(bits(want), bits(inj_cases.expected(c, cuts=cuts)))
    if n_tr >= 2:
        assert not np.array_equal(bits(want), bits(inj_cases.expected(c, reverse=True)))
    a, b = c["planted"]
    assert np.all(bits(want[a]) == 0x80000000) and np.all(bits(want[b]) == inj_cases.NAN_BITS)
    # one train alone on rows of +0.0 with a response of 1: what arrives in cell (r, f) is profile[f][bin], and the bin is the folder's
    for model, delay, profile, _, first, n in c["trains"]:
        end = inj_cases.N_ROWS if n is None else first + n
        got = inj_oracle.inject(np.zeros((inj_cases.N_ROWS, n_f, 4), np.float32), trains=[(model, delay, profile, np.ones(4, np.float32), first, n)])
        bk = psr_oracle.bins(model, delay, first, end - first, n_bins)                     # [rows][f]
        assert np.array_equal(bits(got[first:end, :, 0]), bits(profile[np.arange(n_f)[None, :], bk] + np.float32(0.0)))
        assert not got[:first].any() and not got[end:].any()


def test_lifetime_of_a_pulse_in_the_oracle():
    """The slot rules the GPU test holds the device to, on the oracle: max_pulses live pulses refuse a third, a spent one gives its slot
    back, a pulse that starts before next_row is refused."""
    inj = inj_oracle.Injector(2, 4, 64, max_pulses=2, max_width=8)
    tab = lambda W: (np.array([0, 3], np.int32), np.ones((2, W), np.float32), np.ones(4, np.float32))     # noqa: E731
    inj.add_burst(10, *tab(4))
    inj.add_burst(40, *tab(4))
    with pytest.raises(inj_oracle.Refused) as e:
        inj.add_burst(50, *tab(4))
    assert e.value.code == inj_oracle.STATE
    inj.apply(np.zeros((16, 2, 4), np.float32))                 # next_row 16 = 10 + 3 + 4 - 1: not yet spent
    assert len(inj.live) == 2
    inj.apply(np.zeros((1, 2, 4), np.float32))
    assert len(inj.live) == 1
    with pytest.raises(inj_oracle.Refused) as e:
        inj.add_burst(16, *tab(4))
    assert e.value.code == inj_oracle.STATE
    inj.add_burst(17, *tab(4))
