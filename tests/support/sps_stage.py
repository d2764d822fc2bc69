"""The driver the GPU tests of the single-pulse search stage share (tests/test_gpu_sps.py, tests/test_gpu_sps_shapes.py): one series
pushed through an api.SinglePulseSearch in pieces, every collected push checked against tests/support/sps_oracle.py."""
from __future__ import annotations

import numpy as np
import pytest

import sps_oracle


def run_stage(torch, bf, x, n_widths, sizes, max_t, lag=1, n_streams=2, t_offset=0, log=None, **kw):
    """Pushes x [n_dm][T][n_b] through a SinglePulseSearch in pieces `sizes` (cycled) on `n_streams` alternating HIP streams,
    collecting `lag` pushes behind (max_in_flight = lag + 1), and checks every collected push against the oracle: records to the
    bit, statistics to n_t 2^-52, candidates in their integer fields and snr to 1e-9.  The device is told first_t = t_offset + the
    push's place in x, the oracle t_offset; the other keywords go to both.  Returns the number of candidates; `log`, a list, gets
    one (oracle's dict, device records, device candidates) per push."""
    from dsabeamformer_amd import api

    n_dm, T, n_b = x.shape
    orc = sps_oracle.Search(x, n_widths, t_offset=t_offset, **kw)
    sps = api.SinglePulseSearch(bf, n_dm, n_widths, max_t, max_in_flight=lag + 1, **kw)
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    keep, want, at, k, n_cands = [], [], 0, 0, 0

    def collect():
        nonlocal n_cands
        w = want.pop(0)
        cands = sps.collect()
        rec = sps.last_records()
        where = (w["first_t"], w["n_t"], n_widths, n_dm, n_b)
        assert (rec["first_t"], rec["n_t"]) == (w["first_t"], w["n_t"]), where
        assert np.array_equal(rec["t_end"], w["t_end"]), where
        assert np.array_equal(rec["value"], w["value"]), where                      # the -inf records included
        assert np.array_equal(rec["value"].view(np.uint32), w["value"].view(np.uint32)), where
        rtol = w["n_t"] * 2.0 ** -52
        assert np.allclose(rec["sum"], w["sum"], rtol=rtol, atol=0.0) and np.allclose(rec["sumsq"], w["sumsq"], rtol=rtol, atol=0.0), where
        sps_oracle.assert_candidates_equal(cands, w["cands"], rtol=1e-9)
        n_cands += len(cands)
        if log is not None:
            log.append((w, rec, cands))

    while at < T:
        n = min(sizes[k % len(sizes)], T - at)
        chunk = torch.from_numpy(np.ascontiguousarray(x[:, at:at + n])).cuda()    # [n_dm][n][n_b], as bf_dm_stream_push emits it
        keep.append(chunk)
        sps.push(chunk, n, t_offset + at, streams[k % n_streams].cuda_stream)
        want.append(orc.push(n))
        assert sps.pending == len(want)
        if len(want) > lag:
            collect()
        at += n
        k += 1
    while want:
        collect()
    assert sps.pending == 0
    with pytest.raises(Exception, match="no push is pending"):
        sps.collect()
    sps.close()
    return n_cands
