"""CPU-side checks of the single-pulse search stage (docs/SINGLE_PULSE.md): the candidate selection bf_sps_select against its numpy
restatement, the argument errors of bf_sps_create, the `beam` options, and the oracle itself.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import sps_oracle  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from dsabeamformer_amd import build as b
    from dsabeamformer_amd import _lib

    b.build()
    return _lib.load()


def series_for(n_dm, n_t, n_beams, seed):
    """The random series of tests/test_gpu_sps.py: a wide spread of magnitudes on a pedestal, so that fp32 sums round at every add."""
    rng = np.random.default_rng(seed)
    return (1e3 + rng.standard_normal((n_dm, n_t, n_beams)) * np.exp(rng.uniform(0.0, 6.0, (n_dm, n_t, n_beams)))).astype(np.float32)


# The push-size cycle of tests/test_gpu_sps_shapes.py: 1-row pushes, one exact 128-time tile, a tile and one row, a tile less one row,
# two exact tiles, three tiles (257), short pushes behind long ones; 1100 times = one pass of the cycle.
SHAPE_SIZES = [1, 1, 1, 126, 128, 129, 3, 257, 127, 2, 256, 5, 64]
SHAPE_T = sum(SHAPE_SIZES)


def pushes_of(sizes, n_t):
    """(first time, times) of every push when a series of n_t times is cut into pieces `sizes`, cycled."""
    out, at, k = [], 0, 0
    while at < n_t:
        n = min(sizes[k % len(sizes)], n_t - at)
        out.append((at, n))
        at += n
        k += 1
    return out


def _hand_built_records():
    """K = 4, 3 trials, 8 beams: every branch of the selection in one set of records."""
    K, n_dm, n_b, n = 4, 3, 8, 200
    mu = np.full((n_dm, n_b), 10.0)
    sig = np.full((n_dm, n_b), 2.0)
    value = np.zeros((K, n_dm, n_b), np.float32)
    t_end = np.zeros((K, n_dm, n_b), np.int32)
    for k in range(K):                                   # default: every width at S/N 1 -> below the threshold
        value[k] = (1 << k) * 10.0 + 1.0 * 2.0 * np.sqrt(1 << k)
        t_end[k] = 20 + k
    snr_to_value = lambda k, snr: np.float32((1 << k) * 10.0 + snr * 2.0 * np.sqrt(1 << k))   # noqa: E731
    # (0, 1): width 4 wins clearly: t_start = first_t + t_end - 3
    value[2, 0, 1], t_end[2, 0, 1] = snr_to_value(2, 12.0), 40
    # (0, 2): widths 1 and 4 tie EXACTLY (value - w mu = 2^j * 16, sigma sqrt(w) = 2^j * 2): the lowest k wins
    value[0, 0, 2], value[2, 0, 2] = np.float32(10.0 + 16.0), np.float32(40.0 + 32.0)
    t_end[0, 0, 2], t_end[2, 0, 2] = 7, 9
    # (0, 3): the only width above the threshold has no time in this push (-inf / -1 would be read as a value otherwise)
    value[:, 0, 3], t_end[:, 0, 3] = -np.inf, -1
    # (0, 4): widths 0 .. 2 without a time, width 8 a candidate
    value[:3, 0, 4], t_end[:3, 0, 4] = -np.inf, -1
    value[3, 0, 4], t_end[3, 0, 4] = snr_to_value(3, 9.0), 11
    # (1, 0): sigma == 0 (sumsq / n == mu^2): skipped although the value is huge
    sig[1, 0] = 0.0
    value[1, 1, 0] = 1e6
    # (1, 5) and (2, 7): two more candidates, for the (d, b) order; (2, 7) exactly AT the threshold-reaching side
    value[1, 1, 5], t_end[1, 1, 5] = snr_to_value(1, 30.0), 1
    value[0, 2, 7], t_end[0, 2, 7] = snr_to_value(0, 8.5), 0
    tot_sum = mu * n
    tot_sumsq = (sig * sig + mu * mu) * n
    return value, t_end, tot_sum, tot_sumsq, n


def test_select_matches_the_numpy_restatement_on_hand_built_records(lib):
    from dsabeamformer_amd import api

    value, t_end, tot_sum, tot_sumsq, n = _hand_built_records()
    n_b = value.shape[2]
    kw = dict(first_t=1000, dm_first=17, min_samples=64, threshold=8.0)
    want = sps_oracle.select(value, t_end, tot_sum, tot_sumsq, n, **kw)
    got = api.sps_select((value, t_end), (tot_sum, tot_sumsq), n, n_b, **kw)
    sps_oracle.assert_candidates_equal(got, want, rtol=1e-12)
    # ... and the restatement says what the contract says
    assert [(c[1], c[2], c[3]) for c in want] == [(17, 1, 4), (17, 2, 1), (17, 4, 8), (18, 5, 2), (19, 7, 1)]       # (d, b) order, dm_first offset
    assert [c[0] for c in want] == [1000 + 40 - 3, 1000 + 7, 1000 + 11 - 7, 1000 + 1 - 1, 1000]                    # t_end -> t_start
    assert abs(want[0][5] - 12.0) < 1e-6 and abs(want[1][5] - 8.0) < 1e-12                                          # the tie sits AT the threshold
    # n < min_samples: nothing, whatever the records say; n == min_samples: everything again
    assert len(api.sps_select((value, t_end), (tot_sum, tot_sumsq), n, n_b, **dict(kw, min_samples=n + 1))) == 0
    assert sps_oracle.select(value, t_end, tot_sum, tot_sumsq, n, **dict(kw, min_samples=n + 1)) == []
    assert len(api.sps_select((value, t_end), (tot_sum, tot_sumsq), n, n_b, **dict(kw, min_samples=n))) == len(want)
    # a threshold just above the tie drops exactly that candidate
    hi = api.sps_select((value, t_end), (tot_sum, tot_sumsq), n, n_b, **dict(kw, threshold=8.0 + 1e-9))
    sps_oracle.assert_candidates_equal(hi, sps_oracle.select(value, t_end, tot_sum, tot_sumsq, n, **dict(kw, threshold=8.0 + 1e-9)), rtol=1e-12)
    assert len(hi) == len(want) - 1 and 2 not in hi["beam"]


def test_select_on_random_records(lib):
    from dsabeamformer_amd import api

    rng = np.random.default_rng(5)
    K, n_dm, n_b, n = 6, 4, 12, 777
    x = series_for(n_dm, 300, n_b, 3)
    rec = sps_oracle.push_records(sps_oracle.tree_sums(x, K), 10, 140)
    s, q = sps_oracle.push_stats(x, 0, n)
    rec[1][rng.random(rec[1].shape) < 0.2] = -1
    for thr in (-5.0, 2.0, 3.5):
        want = sps_oracle.select(rec[0], rec[1], s, q, 300, first_t=10, dm_first=3, min_samples=64, threshold=thr)
        got = api.sps_select(rec, (s, q), 300, n_b, first_t=10, dm_first=3, min_samples=64, threshold=thr)
        sps_oracle.assert_candidates_equal(got, want, rtol=1e-12)
    assert 0 < len(want) < n_dm * n_b


def test_create_rejects_bad_arguments_with_a_message(lib):
    s = C.c_void_p()
    assert lib.bf_sps_create(None, 4, 0, 6, 128, 4, 8, 64, 8.0, C.byref(s)) == -1
    assert b"handle is NULL" in lib.bf_last_error() and not s.value
    for k in (0, 9):
        assert lib.bf_sps_create(None, 4, 0, k, 128, 4, 8, 64, 8.0, C.byref(s)) == -1
        assert b"n_widths must be 1 .. 8" in lib.bf_last_error() and not s.value
    assert lib.bf_sps_create(None, 4, 0, 6, 128, 4, 8, 64, 8.0, None) == -1
    assert lib.bf_sps_destroy(None) == 0 and lib.bf_sps_pending(None) == -1
    assert lib.bf_dm_stream_attach_search(None, None) == -1
    n_out = C.c_size_t()
    assert lib.bf_sps_select(None, None, 10, 1, 1, 4, 0, 0, 1, 1.0, None, 0, C.byref(n_out)) == -1


def test_beam_search_options_need_the_dm_stage():
    beam = os.path.join(ROOT, "dsabeamformer_amd", "beam")
    r = subprocess.run([beam, "-j", "8", "-S", "8"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-S" in r.stderr and "-M" in r.stderr
    r = subprocess.run([beam, "-j", "8", "-M", "250", "-C", "x.txt"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-S" in r.stderr
    r = subprocess.run([beam, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("-S snr", "-B n_widths", "-C file"):
        assert opt in r.stdout
    assert "requires -M" in r.stdout


def test_the_oracle_pins_the_association():
    """The GPU test compares peak VALUES bit for bit: that only pins the tree if another association gives other bits on the very
    series it uses.  On an integer-valued series every association gives the exact integer sums."""
    K = 8
    x = series_for(5, 370, 132, 11)
    tree, run = sps_oracle.tree_sums(x, K), sps_oracle.running_sums(x, K)
    pt, pr = sps_oracle.push_records(tree, 0, 370), sps_oracle.push_records(run, 0, 370)
    assert np.array_equal(pt[0][:2], pr[0][:2])                       # widths 1 and 2: one association only
    for k in range(2, K):
        assert not np.array_equal(pt[0][k], pr[0][k]), k              # ... from width 4 on the peaks themselves differ
    exact = np.cumsum(np.asarray(x, np.float64), axis=1)
    for k in (3, 7):                                                  # both are sums of the same window, to fp32 accuracy
        w = 1 << k
        win = exact[:, w:] - exact[:, :-w]
        assert np.allclose(tree[k][:, w:], win, rtol=w * 2.0 ** -23, atol=0) and np.allclose(run[k][:, w:], win, rtol=w * 2.0 ** -23, atol=0)
    xi = np.random.default_rng(1).integers(-1000, 1000, (2, 300, 8)).astype(np.float32)
    ti, ri = sps_oracle.tree_sums(xi, K), sps_oracle.running_sums(xi, K)
    ei = np.cumsum(xi.astype(np.int64), axis=1)
    for k in range(K):
        w = 1 << k
        assert np.array_equal(ti[k][:, w - 1:], ri[k][:, w - 1:])
        assert np.array_equal(ti[k][:, w:].astype(np.int64), ei[:, w:] - ei[:, :-w])
    # records: first occurrence, and -inf / -1 where the push has no time with S_k
    v, t = sps_oracle.push_records(ti, 0, 5)
    assert np.all(t[3:] == -1) and np.all(np.isneginf(v[3:])) and np.all(t[2] == 3 + np.argmax(ti[2][:, 3:5], axis=1) - 0)
    flat = sps_oracle.push_records(sps_oracle.tree_sums(np.ones((1, 40, 4), np.float32), 3), 10, 40)
    assert np.all(flat[1] == 0) and np.array_equal(flat[0][:, 0, 0], [1, 2, 4])


@pytest.mark.parametrize("n_beams", [4, 68])
def test_the_oracle_pins_the_association_on_the_shape_tests_series(n_beams):
    """tests/test_gpu_sps_shapes.py compares peak values bit for bit on few beams and short pushes: also there -- its series, its
    push boundaries in both rotations, 4 and 68 beams -- a left-to-right sum gives other peak bits than the tree for every width
    from 4 on, so a kernel that associated differently at any level could not pass."""
    K = 8
    assert SHAPE_T == 1100 and max(SHAPE_SIZES) == 257
    x = series_for(3, SHAPE_T, n_beams, 1000 * K + n_beams)
    tree, run = sps_oracle.tree_sums(x, K), sps_oracle.running_sums(x, K)
    for rot in (0, 3):
        differs = np.zeros(K, bool)
        for lo, n in pushes_of(SHAPE_SIZES[rot:] + SHAPE_SIZES[:rot], SHAPE_T):
            pt, pr = sps_oracle.push_records(tree, lo, lo + n), sps_oracle.push_records(run, lo, lo + n)
            assert np.array_equal(pt[1] < 0, pr[1] < 0)                   # the same records exist
            differs |= [not np.array_equal(pt[0][k], pr[0][k]) for k in range(K)]
        assert not differs[:2].any() and differs[2:].all(), (rot, differs)
