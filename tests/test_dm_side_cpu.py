"""tests/support/dm_side.py without a GPU: it imports, and the host-side pieces the GPU tests lean on (the driver's ladder, the share of a
rank, the stamp request of an event, the closing lines of a log) give what the driver's code says."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dm_side  # noqa: E402


def test_the_ladder_is_the_drivers_and_the_shares_cover_it():
    from dsabeamformer_amd import host

    for n_cap in (8, 7, 6, 1):
        dms, freq, delays = dm_side.beam_ladder(250.0, n_cap)
        assert len(dms) == n_cap and dms[0] == 0.0 and delays.shape == (n_cap, 256) and delays.dtype == np.int32
        assert not delays[0].any() and not delays[:, 0].any() and np.all(np.diff(delays.max(axis=1)) > 0)      # referred to channel 0, ascending
        for world in (2, 4):
            shares = [host.dm_trial_share(n_cap, world, rk) for rk in range(world)]
            assert [f for f, _ in shares] == [sum(c for _, c in shares[:rk]) for rk in range(world)] and sum(c for _, c in shares) == n_cap
            assert max(c for _, c in shares) - min(c for _, c in shares) <= 1 and sorted((c for _, c in shares), reverse=True) == [c for _, c in shares]
    assert [host.dm_trial_share(6, 4, rk) for rk in range(4)] == [(0, 2), (2, 2), (4, 1), (5, 1)]
    assert host.dm_trial_share(1, 2, 1) == (1, 0)


def test_the_stamp_request_and_the_closing_lines():
    best = dict(t_start=300, width=8, dm=5, beam=3)
    assert dm_side.stamp_request(dict(best=best)) == (300 + 4 - 32 * 4, 5, 3, 4, 8)          # 64 bins of width / 2 rows, centred on the boxcar
    assert dm_side.stamp_request(dict(best=dict(best, t_start=3, width=1))) == (0, 5, 3, 1, 1)  # clipped at the first row
    log = "DM stage: 8 trials\nSynchronized\nDM stage: trials 0 .. 7 of 8\nWrote 3 candidates to c\nEvents: 2 events\n"
    assert dm_side.closing_lines(log) == ["DM stage: trials 0 .. 7 of 8", "Events: 2 events"]
