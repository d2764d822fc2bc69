"""GPU tests (-m gpu) of the single-pulse search stage (include/dsabf.h: bf_sps_*; docs/SINGLE_PULSE.md), through the C-ABI.
The reference is tests/support/sps_oracle.py: the boxcar tree over the WHOLE series, cut at the pushes' boundaries."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dm_side  # noqa: E402
import sps_oracle  # noqa: E402
from sps_stage import run_stage as _run_stage  # noqa: E402
from test_sps_cpu import series_for  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_STATE = -4


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


# 130 = one whole 128-time tile and a second of 2 (129: of 1); three 1-row pushes in a row, far shorter than the carried tail
MAX_T = 130
SIZES = [MAX_T, 1, 1, 1, 7, 2, 31, MAX_T - 1, 64]


@pytest.mark.sweep_cap(12)
@pytest.mark.parametrize("n_widths", [1, 6, 8])
@pytest.mark.parametrize("n_beams", [132, 256])
@pytest.mark.parametrize("n_dm", [1, 5])
def test_peaks_to_the_bit_whatever_the_pushes(torch, bfmod, n_dm, n_beams, n_widths):
    """The records of every push -- maximum of S_k over the push's times, first time attaining it, -inf / -1 where S_k does not
    exist yet -- equal the oracle's whole-series tree cut at the same boundaries, bit for bit; the statistics to n_t 2^-52.  Once
    with the cycle as it stands (first push = the largest), once starting at its second entry: the first pushes are then single
    rows, shorter than 2^(K-1), and the stream start runs through the -inf records of every width."""
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_beams, n_freq=8))
    x = series_for(n_dm, 370, n_beams, 1000 * n_dm + n_beams + n_widths)
    for rot in (0, 1):
        n = _run_stage(torch, bf, x, n_widths, SIZES[rot:] + SIZES[:rot], MAX_T, threshold=3.0)
        assert n > 0
    bf.close()


def test_ties_and_plateaus_resolve_to_the_first_time(torch, bfmod):
    n_dm, T, n_b = 3, 300, 132
    rng = np.random.default_rng(8)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    # integers 0 .. 3: every width has its maximum many times over
    x = rng.integers(0, 4, (n_dm, T, n_b)).astype(np.float32)
    # a constant series: every time ties
    const = np.full((n_dm, T, n_b), 7.0, np.float32)
    # one maximum on the last time of a tile-sized stretch (127) and again just behind it (128, the next tile's first), and the
    # same at the boundary between row-lanes (15 | 16) in another trial
    edge = rng.integers(0, 4, (n_dm, T, n_b)).astype(np.float32)
    edge[0, 127], edge[0, 128] = 100.0, 100.0
    edge[1, 15], edge[1, 16], edge[1, 143] = 50.0, 50.0, 50.0
    for series in (x, const, edge):
        for sizes in ([T], [MAX_T, 1, 40]):
            _run_stage(torch, bf, series, 5, sizes, T, threshold=1e9)
    v, t = sps_oracle.push_records(sps_oracle.tree_sums(edge, 5), 0, T)
    assert np.all(t[0, 0] == 127) and np.all(t[0, 1] == 15) and np.all(t[1, 0] == 128) and np.all(v[1, 0] == 200.0)   # what the device was held to
    bf.close()


# ---- behind the DM stage -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fine_ladder(orc):
    """The fine_ladder construction of tests/test_gpu_round5.py (210 x 48 x 256, 40 trials), the pulse widened to 4 rows."""
    from test_gpu_round5 import _pulse_delays

    rng = np.random.default_rng(77)
    n_t, n_f, n_b, n_dm, max_rows = 210, 48, 256, 40, 32
    delays = _pulse_delays(n_dm, n_f, 45)
    D = int(delays.max())
    series = (rng.random((n_t, n_f, n_b), dtype=np.float32) * 1e3).astype(np.float32)
    k_true, t0 = n_dm // 2, 70
    for f in range(n_f):
        for j in range(4):
            series[t0 + delays[k_true, f] + j, f, :] += np.float32(5e5)
    want = orc.dedisperse_dm(series, delays, n_t - D)          # [n_dm][n_t - D][n_b]
    return dict(n_t=n_t, n_f=n_f, n_b=n_b, n_dm=n_dm, max_rows=max_rows, delays=delays, D=D, series=series, k_true=k_true, t0=t0, want=want)


DM_SIZES = [32, 1, 7, 32, 3, 19, 2, 32, 31, 11]     # the ragged pieces of the DM stage's own test
# Widths 1, 2, 4.  The pulse outweighs the noise ten-thousandfold, so the deviation of every window that holds it IS the pulse, and
# snr = sqrt(n) * C / sqrt(w * sum p^2) with C the boxcar's share of the pulse profile p: by Cauchy-Schwarz at most sqrt(n), reached
# only by a rectangular profile that fills the boxcar -- trial k_true, width 4.  That holds as long as no boxcar reaches back to pulse
# samples in front of the baseline window; widths up to 4 do not (wider ones do: a 32-sample boxcar of a LATER chunk still catches
# the tail of a smeared trial whose deviation is the noise's alone, and wins).
THRESHOLD, N_WIDTHS = 6.0, 3


def _dm_pushes(fl):
    """(rows pushed, first output time, output times) of every push of the ragged run."""
    out, pushed, k = [], 0, 0
    while pushed < fl["n_t"]:
        n = min(DM_SIZES[k % len(DM_SIZES)], fl["n_t"] - pushed)
        out.append((n, max(0, pushed - fl["D"]), max(0, pushed + n - fl["D"]) - max(0, pushed - fl["D"])))
        pushed += n
        k += 1
    return out


def test_behind_the_dm_stage_the_pulse_is_the_best_candidate(torch, bfmod, fine_ladder):
    """The stage attached to a bf_dm_stream: every chunk the DM stage emits is searched where it lies.  The candidates of every
    push equal the oracle's over orc.dedisperse_dm of the whole series (integers exactly; snr to 1e-9: the n 2^-52 bound of the
    fp64 statistics times the cancellation factor (mu^2 + var) / var of sigma -- about 4 for uniform samples, 145 for their sums
    over 48 channels, near 1 where the pulse sets the deviation -- stays below 1e-11 for n <= 250), with the zero-copy and the copy
    feed, the ring and the linear buffer; the chunks themselves stay bit-equal to the oracle's."""
    import ctypes as C

    from dsabeamformer_amd import _lib, api

    hip = _lib._preload_hip_runtime()
    fl = fine_ladder
    n_dm, n_b, n_f, D, max_rows, want = fl["n_dm"], fl["n_b"], fl["n_f"], fl["D"], fl["max_rows"], fl["want"]
    # ---- the oracle alone: the search finds the pulse, and no S/N sits on the threshold
    orc = sps_oracle.Search(want, N_WIDTHS, dm_first=0, threshold=-np.inf)
    pushes = _dm_pushes(fl)
    every = [c for _, _, n_out in pushes if n_out for c in orc.push(n_out)["cands"]]
    snr = np.array([c[5] for c in every])
    assert np.all(np.abs(snr - THRESHOLD) > 1e-6 * THRESHOLD)
    best = every[int(snr.argmax())]
    assert np.count_nonzero(snr == snr.max()) == 1
    assert (best[0], best[1], best[3]) == (fl["t0"], fl["k_true"], 4), best
    assert 0 < np.count_nonzero(snr >= THRESHOLD) < len(every)
    # ---- the device
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    d_series = torch.from_numpy(fl["series"]).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    row_bytes = n_f * n_b * 4
    for feed, ring in (("reserve", 1), ("copy", 1), ("reserve", 0), ("copy", 0)):
        bf.set_switch("dm_ring", ring)
        dm = api.DmStream(bf, fl["delays"], n_f, max_rows)
        sps = api.SinglePulseSearch(bf, n_dm, N_WIDTHS, max_rows, threshold=THRESHOLD)
        dm.attach_search(sps)
        orc = sps_oracle.Search(want, N_WIDTHS, threshold=THRESHOLD)
        host = torch.full((n_dm * max_rows * n_b,), float("nan"), dtype=torch.float32).pin_memory()
        parts, pushed, found = [], 0, []
        for k, (n, first_t, n_out) in enumerate(pushes):
            st = streams[k % 2]
            src = d_series.data_ptr() + pushed * row_bytes
            if feed == "reserve":
                dst = dm.reserve(n, st.cuda_stream)
                assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(n * row_bytes), 3, C.c_void_p(st.cuda_stream)) == 0
                src = dst
            assert dm.push(src, n, host, st.cuda_stream) == (first_t, n_out)
            pushed += n
            assert sps.pending == (1 if n_out else 0)
            if not n_out:
                continue
            st.synchronize()
            parts.append(host[:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b).copy())
            w = orc.push(n_out)
            cands = sps.collect()
            sps_oracle.assert_candidates_equal(cands, w["cands"], rtol=1e-9)
            rec = sps.last_records()
            assert (rec["first_t"], rec["n_t"]) == (first_t, n_out) and np.array_equal(rec["value"], w["value"]) and np.array_equal(rec["t_end"], w["t_end"])
            found.append(cands)
        assert np.array_equal(np.concatenate(parts, axis=1), want), (feed, ring)       # the DM chunks themselves
        found = np.concatenate(found)
        top = found[int(found["snr"].argmax())]
        assert (int(top["t_start"]), int(top["dm"]), int(top["width"])) == (fl["t0"], fl["k_true"], 4)
        sps.close()
        dm.close()
    bf.set_switch("dm_ring", 1)
    bf.close()


def test_back_pressure_lifetime_and_detaching(torch, bfmod, fine_ladder):
    from dsabeamformer_amd import api

    fl = fine_ladder
    n_dm, n_b, n_f, D, max_rows = fl["n_dm"], fl["n_b"], fl["n_f"], fl["D"], fl["max_rows"]
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    # ---- max_in_flight + 1 pushes without a collect: BF_ERR_STATE, and nothing is lost
    x = series_for(2, 90, n_b, 4)
    sps = api.SinglePulseSearch(bf, 2, 4, 30, max_in_flight=2, threshold=2.5)
    orc = sps_oracle.Search(x, 4, threshold=2.5)
    chunks = [torch.from_numpy(np.ascontiguousarray(x[:, 30 * i:30 * i + 30])).cuda() for i in range(3)]
    st = torch.cuda.Stream()
    sps.push(chunks[0], 30, 0, st.cuda_stream)
    sps.push(chunks[1], 30, 30, st.cuda_stream)
    with pytest.raises(bfmod.DsabfError) as e:
        sps.push(chunks[2], 30, 60, st.cuda_stream)
    assert e.value.code == BF_ERR_STATE and sps.pending == 2
    assert str(e.value) == "libdsabf error -4: bf_sps_push: 2 pushes are uncollected (max_in_flight): bf_sps_collect first"
    out = np.zeros(4, api._candidate_dtype())
    import ctypes as C
    n_out = C.c_size_t()
    assert sps._lib.bf_sps_collect(sps._s, api._ptr(out), out.size, C.byref(n_out)) == -1 and sps.pending == 2   # max_out < n_dm * n_beams
    for i in range(3):
        if i == 2:
            sps.push(chunks[2], 30, 60, st.cuda_stream)
        w = orc.push(30)
        sps_oracle.assert_candidates_equal(sps.collect(), w["cands"], rtol=1e-9)
        rec = sps.last_records()
        assert np.array_equal(rec["value"], w["value"]) and np.array_equal(rec["t_end"], w["t_end"]) and rec["first_t"] == 30 * i
    # ---- through the DM stage: the push that would overrun the search is refused before it queues anything; detaching mid-stream
    dm = api.DmStream(bf, fl["delays"], n_f, max_rows)
    small = api.SinglePulseSearch(bf, n_dm, 3, max_rows, max_in_flight=1, threshold=1e9)
    with pytest.raises(bfmod.DsabfError, match="trials"):
        dm.attach_search(sps)                                                       # n_dm does not match
    dm.attach_search(small)
    d_series = torch.from_numpy(fl["series"]).cuda()
    host = torch.zeros((n_dm * max_rows * n_b,), dtype=torch.float32).pin_memory()
    row = n_f * n_b * 4
    pushed, parts = 0, []

    def push(n):
        nonlocal pushed
        first, n_out = dm.push(d_series.data_ptr() + pushed * row, n, host, st.cuda_stream)
        st.synchronize()
        pushed += n
        if n_out:
            parts.append(host[:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b).copy())
        return first, n_out

    assert push(32) == (0, 0) and small.pending == 0                                # nothing emitted yet: no search push
    assert push(32) == (0, 64 - D) and small.pending == 1
    with pytest.raises(bfmod.DsabfError) as e:
        push(8)
    assert e.value.code == BF_ERR_STATE and pushed == 64
    assert str(e.value) == ("libdsabf error -4: bf_dm_stream_push: the attached search stage has 1 uncollected pushes (max_in_flight): "
                            "bf_sps_collect first")
    small.collect()
    assert push(8) == (64 - D, 8) and small.pending == 1
    small.collect()
    assert small.last_records()["first_t"] == 64 - D
    dm.attach_search(None)                                                          # detached: the DM stage goes on alone
    assert push(32)[1] == 32 and push(5)[1] == 5 and small.pending == 0
    assert np.array_equal(np.concatenate(parts, axis=1), fl["want"][:, :pushed - D])
    # ---- the handle destroyed first: the stages answer BF_ERR_STATE and can still be destroyed
    dm.attach_search(small)
    bf.close()
    for call in (lambda: sps.push(chunks[0], 30, 90, st.cuda_stream), sps.collect, lambda: dm.push(d_series, 1, None, 0), lambda: dm.attach_search(None)):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE
    small.close()
    sps.close()
    dm.close()


def test_beam_cli_writes_the_candidates_the_oracle_finds_in_its_dm_file(tmp_path):
    """`beam -j 33 -M 250 -N 8 -S 4 -B 6 -W dm.bin -C cands.txt`: 25 burn-in reads + 8 analysed blocks (the junk source counts the
    burn-in reads, so `-j 8` alone would analyse nothing).  The candidates are recomputed from dm.bin by the oracle -- the same
    chunk boundaries, the baseline window of 8 chunks and the 64-sample minimum run_observation uses -- and compared with the file.
    Threshold 4: the maximum of ~10^3 boxcar sums of near-Gaussian noise passes 4 sigma in a few per cent of the 16384 (trial,
    beam, chunk) records."""
    from dsabeamformer_amd import build, host

    dm_file, cand_file = tmp_path / "dm.bin", tmp_path / "cands.txt"
    thr = 4.0
    r = subprocess.run([build.BEAM, "-j", "33", "-M", "250", "-N", "8", "-S", str(thr), "-B", "6", "-W", str(dm_file), "-C", str(cand_file)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hdr, data, chunks = host.read_dm_file(str(dm_file))
    assert data.shape[0] == 8 and len(chunks) == 8 and sum(n for _, n in chunks) == data.shape[1]
    # (the comparison itself: tests/support/dm_side.py, shared with the trial-split runs of tests/test_gpu_trial_split.py)
    got, want = dm_side.check_candidates(cand_file, r.stdout, data, chunks, 6, thr)
    print("candidates recomputed from dm.bin:", len(want))
    assert 1 <= len(got) == len(want) <= 5000
