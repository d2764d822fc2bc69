"""The inputs of tests/test_gpu_dm_paths.py held to their own conditions, without a GPU (tests/support/dm_paths.py): every case
reaches the paths of csrc/bf_dm_wide.hip it claims, the cases together reach all of them, and the C oracle the GPU tests compare
with agrees bit for bit with an independent numpy restatement of the definition on exactly these inputs -- the rows before the
series and past its end included."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))

import dm_paths  # noqa: E402

CASES = dm_paths.all_cases()


@pytest.fixture(scope="module")
def censuses():
    return {c.name: c.census() for c in CASES}


def test_rows_cap_is_even_bounded_and_shrinks_with_the_channel_count():
    caps = [dm_paths.rows_cap(n) for n in range(1, dm_paths.MAX_FREQ + 1)]
    assert all(c % 2 == 0 and 16 < c <= 128 for c in caps)
    assert all(a >= b for a, b in zip(caps, caps[1:]))
    assert caps[0] > caps[-1]                                            # ... and really does: the tables take LDS
    # the figures the cases are built around (csrc/bf_dm_wide.hip: 159 KiB of LDS, 40 table bytes per channel, 3 x 512-byte rows)
    assert (dm_paths.rows_cap(8), dm_paths.rows_cap(64), dm_paths.rows_cap(256), dm_paths.rows_cap(1024)) == (104, 102, 98, 78)
    # a fourth piece per wave exists from 97 rows on: only windows of few channels reach it
    assert dm_paths.pieces_per_wave(96).max() == 3 and dm_paths.pieces_per_wave(97).tolist() == [4] + [3] * 15
    assert dm_paths.pieces_per_wave(16).tolist() == [1] * 8 + [0] * 8


def test_names_are_unique_and_nothing_is_drawn_twice_differently():
    assert len({c.name for c in CASES}) == len(CASES)
    again = dm_paths.all_cases()
    for a, b in zip(CASES, again):
        assert a.name == b.name and np.array_equal(a.delays, b.delays) and a.n_t_outs == b.n_t_outs
    assert np.array_equal(CASES[0].series(), again[0].series())


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_case_reaches_what_it_claims(case, censuses):
    got, claims = censuses[case.name], dict(case.claims)
    assert case.mask == claims.pop("mask"), (case.fits, got)
    assert 120 <= case.n_t <= 320 and case.n_b <= 256 and case.n_b % 4 == 0
    assert case.series().nbytes <= 8 << 20
    if "pairs_exactly" in claims:
        assert got["pairs"] == claims.pop("pairs_exactly")
    for key in ("pairs", "pieces", "paths", "lane_kinds"):
        if key in claims:
            assert claims.pop(key) <= got[key], (key, got[key])
    if case.name.startswith("edges") and case.n_b < dm_paths.BEAMS:
        assert got["paths"] == {"lane"}                                  # no full beam tile: never the buffer-addressed path
    for key in ("mixed_tile", "piece_runs"):
        if key in claims:
            assert got[key] == claims.pop(key), key
    assert not claims, claims


def test_the_cases_together_reach_every_path(censuses):
    union = {k: set().union(*(c[k] for c in censuses.values())) for k in ("pairs", "pieces", "paths", "lane_kinds")}
    assert union["pairs"] == set(dm_paths.PAIR_CLASSES)
    assert union["pieces"] == {0, 1, 2, 3, 4}
    assert union["paths"] == {"inside", "lane"}
    assert union["lane_kinds"] == {"before_start", "past_end", "straddle_end", "partial_beams"}
    assert any(c["mixed_tile"] for c in censuses.values())
    # the class changes from channel to channel within ONE wave of pair_distances
    d = dm_paths.pair_distances().delays.astype(np.int64)
    delta = d[1::2] - d[0::2]
    assert all(len(set(np.clip(row, -1, 4).tolist())) >= 4 for row in delta)
    assert all((row[1:] != row[:-1]).sum() >= len(row) // 2 for row in delta)
    # both sides of the fit boundary, exactly one row apart, at more than one channel count
    sides = {}
    for n_f in dm_paths.CAP_CHANNELS[:3] + (8,):
        case = dm_paths.cap_by_channels(n_f) if n_f != 8 else dm_paths.piece_counts()
        rows = [int((g.max(axis=0) - g.min(axis=0)).max()) + dm_paths.TB for g in dm_paths.groups_of(case.delays)]
        sides[n_f] = {(r - dm_paths.rows_cap(n_f), bool(f)) for r, f in zip(rows, case.fits)}
        assert {(0, True), (1, False)} <= sides[n_f], (n_f, sides[n_f])
    assert len({dm_paths.rows_cap(n) for n in sides}) == 4
    # a group whose trials all share one delay, and the trial counts and channel counts of the ring's prologue and tails
    g0 = dm_paths.piece_counts().delays[:32]
    assert (g0 == g0[0]).all()
    assert {c.n_f for c in CASES} >= {1, 2, 3, 4, 5, 64, 1024, 1025} and {c.n_dm for c in CASES} >= {1, 2, 31, 32, 33, 63}
    # the two ladders the stale-flag test alternates flip group 1 and keep the trial count
    a, b = dm_paths.flag_ladders()[:2]
    assert a.n_dm == b.n_dm and a.mask ^ b.mask == 0b010


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_c_oracle_is_the_definition_on_every_case(case, orc):
    """The GPU tests lean on orc.dedisperse_dm where it had only been compared with the kernels: negative rows, rows past the end."""
    series = case.series()
    rows = series.reshape(case.n_t, -1)
    assert len(np.unique(rows[:, :4], axis=0)) == case.n_t              # every row distinct
    for n_t_out in case.n_t_outs:
        want = dm_paths.dedisperse_numpy(series, case.delays, n_t_out)
        got = orc.dedisperse_dm(series, case.delays, n_t_out)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case, n_t_out)


def test_dedisperse_numpy_on_a_sum_worked_by_hand():
    series = np.array([[[1.0], [2.0 ** -30]], [[3.0], [1.0]], [[5.0], [7.0]]], np.float32)      # [t = 3][f = 2][b = 1]
    delays = np.array([[0, 0], [1, -1], [-1, 2], [3, 0]], np.int32)
    out = dm_paths.dedisperse_numpy(series, delays, 2)
    one = np.float32(1.0)
    assert out[:, :, 0].tolist() == [[float(one + np.float32(2.0 ** -30)), 4.0], [3.0, float(np.float32(5.0) + np.float32(2.0 ** -30))],
                                     [7.0, 1.0], [float(np.float32(2.0 ** -30)), 1.0]]
