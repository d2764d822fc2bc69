"""GPU tests (-m gpu) of the pulse injector (include/dsabf.h: bf_inj_*, bf_dm_stream_attach_injector; docs/INJECTION.md), through the
C-ABI.  The reference is tests/support/inj_oracle.py, a numpy restatement of the contract; rows are compared with it bit for bit
(.view(np.uint32): a -0.0 and a NaN's payload cannot hide).

The inputs come from tests/support/inj_cases.py: x = N(0, 1) * 2^e with e in -20 .. 20, so that the order of two pulses on one cell and
every rounding show.  tests/test_inj_cpu.py holds the oracle to that on exactly these inputs, without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cond_oracle  # noqa: E402
import dm_side  # noqa: E402
import inj_cases  # noqa: E402
import inj_oracle  # noqa: E402
import sps_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
N_ROWS, SIZES = inj_cases.N_ROWS, inj_cases.SIZES


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def add_all(inj, c):
    """Every pulse of a case, bursts first: the ids the oracle's inject() gives them."""
    ids = [inj.add_burst(t0, delay, profile, response) for t0, delay, profile, response in c["bursts"]]
    ids += [inj.add_train(model, delay, profile, response, first, n) for model, delay, profile, response, first, n in c["trains"]]
    assert ids == list(range(len(ids)))


def apply_all(inj, d_x, row_bytes, cuts, streams):
    """The rows of d_x through `inj` in the given cuts, alternating over the streams, no host synchronisation in between."""
    for k, (at, n) in enumerate(cuts):
        inj.apply(d_x.data_ptr() + at * row_bytes, n, streams[k % len(streams)].cuda_stream)


def run_case(torch, bfmod, c, sizes=SIZES):
    from dsabeamformer_amd import api

    x = c["x"]
    _, n_f, n_b = x.shape
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    inj = api.Injector(bf, n_f, max(sizes), max_pulses=8, max_width=c["max_width"])
    add_all(inj, c)
    apply_all(inj, d_x, n_f * n_b * 4, inj_cases.cuts_of(x.shape[0], sizes), streams)
    torch.cuda.synchronize()
    got = d_x.cpu().numpy()
    assert inj.next_row == x.shape[0] and inj.launches > 0
    inj.close()
    bf.close()
    return got


# ---- 1. bursts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.sweep_cap(len(inj_cases.BURST_CASES))
@pytest.mark.parametrize("case", inj_cases.BURST_CASES, ids=lambda c: "b%d-f%d-w%d" % c)
def test_bursts_every_shape_to_the_bit(torch, bfmod, case):
    """203 rows cut [1, 7, 33, 64] cyclically over two queues; three bursts, two of them overlapping in cells, one starting on a cut, one
    straddling two, one running off the end, one channel's delay beyond the series; -0.0 and a NaN planted outside every window."""
    c = inj_cases.burst_case(case)
    want = inj_cases.expected(c)
    got = run_case(torch, bfmod, c)
    assert np.array_equal(bits(got), bits(want))
    a, b = c["planted"]
    assert np.all(bits(got[a]) == 0x80000000) and np.all(bits(got[b]) == inj_cases.NAN_BITS)


def test_the_cut_into_applies_does_not_matter(torch, bfmod):
    c = inj_cases.burst_case((68, 3, 64))
    want = inj_cases.expected(c)
    for sizes in ([N_ROWS], [1], [33, 1, 64, 7, 2, 64]):
        assert np.array_equal(bits(run_case(torch, bfmod, c, sizes)), bits(want)), sizes


def test_more_bursts_than_one_launch_takes(torch, bfmod):
    """Eleven bursts on the same cells: three launches per apply, in id order."""
    from dsabeamformer_amd import api

    n_b, n_f, W, n = 64, 3, 7, 40
    rng = np.random.default_rng(11)
    x = inj_cases.wide(rng, (n, n_f, n_b))
    bursts = [(5 + k % 3, rng.integers(0, 4, n_f).astype(np.int32), inj_cases.wide(rng, (n_f, W), 6), inj_cases.response_of(rng, n_b)) for k in range(11)]
    want = inj_oracle.inject(x, bursts)
    assert not np.array_equal(bits(want), bits(inj_oracle.inject(x, bursts, reverse=True)))
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    d_x = torch.from_numpy(x).cuda()
    inj = api.Injector(bf, n_f, n, max_pulses=11, max_width=W)
    for b in bursts:
        inj.add_burst(*b)
    inj.apply(d_x, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert inj.launches == 3 and np.array_equal(bits(d_x.cpu().numpy()), bits(want))
    inj.close()
    bf.close()


# ---- 2. trains ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.sweep_cap(len(inj_cases.TRAIN_CASES))
@pytest.mark.parametrize("case", inj_cases.TRAIN_CASES, ids=lambda c: "b%d-f%d-bins%d-tr%d%s" % (c[0], c[1], c[2], c[3], "-" + c[4] if c[4] else ""))
def test_trains_to_the_bit(torch, bfmod, case):
    """1 .. 4 trains of the four model kinds behind a burst on the same cells; first_row and n_rows gate inside a cut."""
    c = inj_cases.train_case(case)
    want = inj_cases.expected(c)
    got = run_case(torch, bfmod, c)
    assert np.array_equal(bits(got), bits(want))
    a, b = c["planted"]
    assert np.all(bits(got[a]) == 0x80000000) and np.all(bits(got[b]) == inj_cases.NAN_BITS)


# ---- 3. closure with the folder -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_bins", [("fast", 5), ("slow", 64), ("creep", 4096)])
def test_closure_with_the_folder(torch, bfmod, kind, n_bins):
    """A train injected into rows of +0.0 and folded with the same model and delays: profile[f][j][b] = hits[f][j] *
    (double)fl(profile_inj[f][j] response[b]) EXACTLY -- one fp32 value added fewer than 2^20 times in fp64 is exact.  The injector's
    bin is the folder's bin, with no oracle in between."""
    from dsabeamformer_amd import api

    n_b, n_f = 68, 3
    rng = np.random.default_rng(n_bins)
    model = inj_cases.models_for(1, n_bins, N_ROWS, kind)[0]
    delay = rng.integers(0, 25, n_f).astype(np.int32)
    prof_inj = inj_cases.wide(rng, (n_f, n_bins), 6)
    resp = inj_cases.response_of(rng, n_b)
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    d_x = torch.zeros((N_ROWS, n_f, n_b), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    inj = api.Injector(bf, n_f, 64, max_width=n_bins)
    inj.add_train(model, delay, prof_inj, resp)
    folder = api.PulsarFolder(bf, n_f, 64, n_bins, [model], delay[None, :])
    for at, n in inj_cases.cuts_of(N_ROWS, SIZES):
        p = d_x.data_ptr() + at * n_f * n_b * 4
        inj.apply(p, n, st.cuda_stream)
        folder.push(p, n, st.cuda_stream)
    folder.dump()
    prof, hits, _, n_rows = folder.collect()
    assert n_rows == N_ROWS and int(hits.sum()) == N_ROWS * n_f
    cell = (prof_inj[:, :, None] * resp[None, None, :]).astype(np.float64)                    # fp32 product, widened
    want = hits[0].astype(np.float64)[:, :, None] * cell
    assert np.array_equal(np.ascontiguousarray(prof[0]).view(np.uint64), np.ascontiguousarray(want + 0.0).view(np.uint64))
    assert np.count_nonzero(hits[0]) > (1 if kind != "creep" else 60)
    folder.close()
    inj.close()
    bf.close()


# ---- 4. idle costs nothing ----------------------------------------------------------------------------------------------------------
def test_idle_applies_launch_nothing(torch, bfmod, orc):
    from dsabeamformer_amd import api

    n_b, n_f, n = 8, 5, 64
    rng = np.random.default_rng(4)
    x = inj_cases.wide(rng, (3 * n, n_f, n_b))
    x[7, 2].view(np.uint32)[:] = inj_cases.NAN_BITS
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    d_x = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    inj = api.Injector(bf, n_f, n, max_width=8)
    delay = np.array([0, 1, 2, 3, 500], np.int32)
    ones = np.ones((n_f, 8), np.float32)
    inj.add_burst(2 * n + 10, delay, ones, np.ones(n_b, np.float32))
    inj.add_train((0, 1 << 60, 0, 0), delay, ones, np.ones(n_b, np.float32), first_row=2 * n + 20, n_rows=5)
    for k in range(2):                               # no pulse overlaps the first two applies
        inj.apply(d_x.data_ptr() + k * n * n_f * n_b * 4, n, st)
        assert inj.launches == 0 and inj.next_row == (k + 1) * n
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_x.cpu().numpy()), bits(x))
    inj.apply(d_x.data_ptr() + 2 * n * n_f * n_b * 4, n, st)
    assert inj.launches == 2                         # one launch for the burst, one for the train
    torch.cuda.synchronize()
    want = inj_oracle.inject(x, [(2 * n + 10, delay, ones, np.ones(n_b, np.float32))],
                             [((0, 1 << 60, 0, 0), delay, ones, np.ones(n_b, np.float32), 2 * n + 20, 5)], cuts=[n, n, n])
    assert np.array_equal(bits(d_x.cpu().numpy()), bits(want)) and not np.array_equal(bits(want), bits(x))
    inj.close()
    # ---- attached and idle: the DM chunks are those of an unattached stream
    delays = np.array([[d * (n_f - 1 - f) for f in range(n_f)] for d in range(3)], np.int32)
    D = int(delays.max())
    x[7, 2] = 1.0                                    # (no NaN through the sums: its payload is not the contract's)
    want = orc.dedisperse_dm(x, delays, 3 * n - D)
    parts = {}
    for attached in (False, True):
        d_x = torch.from_numpy(x).cuda()
        dm = api.DmStream(bf, delays, n_f, n)
        inj = api.Injector(bf, n_f, n)
        if attached:
            dm.attach_injector(inj)
        host = torch.zeros(3 * n * n_b, dtype=torch.float32).pin_memory()
        got = []
        for k in range(3):
            first_t, n_out = dm.push(d_x.data_ptr() + k * n * n_f * n_b * 4, n, host, st)
            torch.cuda.synchronize()
            got.append(host[:3 * n_out * n_b].numpy().reshape(3, n_out, n_b).copy())
        parts[attached] = np.concatenate(got, axis=1)
        assert inj.launches == 0 and inj.next_row == (3 * n if attached else 0)
        inj.close()
        dm.close()
    assert np.array_equal(bits(parts[True]), bits(parts[False])) and np.array_equal(bits(parts[False]), bits(want))
    bf.close()


# ---- 5. slots -----------------------------------------------------------------------------------------------------------------------
def test_slots_and_refusals(torch, bfmod):
    from dsabeamformer_amd import _lib, api

    lib = _lib.load()
    n_b, n_f = 8, 2
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    x = inj_cases.wide(np.random.default_rng(5), (96, n_f, n_b))
    d_x = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    inj = api.Injector(bf, n_f, 32, max_pulses=2, max_width=8)
    orc = inj_oracle.Injector(n_f, n_b, 32, max_pulses=2, max_width=8)
    rng = np.random.default_rng(6)
    tab = lambda W=4: (np.array([0, 3], np.int32), inj_cases.wide(rng, (n_f, W), 4), inj_cases.response_of(rng, n_b))     # noqa: E731
    for t0 in (10, 40):
        t = tab()
        assert inj.add_burst(t0, *t) == orc.add_burst(t0, *t)
    with pytest.raises(bfmod.DsabfError, match="max_pulses") as e:                # both slots live
        inj.add_burst(50, *tab())
    assert e.value.code == BF_ERR_STATE
    want = x.copy()
    for at, n in ((0, 16), (16, 1)):                                               # past the first burst: rows 10 .. 16
        inj.apply(d_x.data_ptr() + at * n_f * n_b * 4, n, st)
        orc.apply(want[at:at + n])
    with pytest.raises(bfmod.DsabfError, match="lies before") as e:               # starts before next_row = 17
        inj.add_burst(16, *tab())
    assert e.value.code == BF_ERR_STATE
    with pytest.raises(bfmod.DsabfError, match="lies before") as e:
        inj.add_train((0, 1 << 60, 0, 0), *tab(), first_row=16)
    assert e.value.code == BF_ERR_STATE
    t = tab(8)                                                                      # a larger table than the slot's last: accepted
    assert inj.add_burst(17, *t) == orc.add_burst(17, *t) == 2
    for k in range(4):                                                              # four trains, and no room for them: max_pulses first
        with pytest.raises(bfmod.DsabfError, match="max_pulses"):
            inj.add_train((0, 1 << 60, 0, 0), *tab(), first_row=20)
    for at, n in ((17, 32), (49, 15)):
        inj.apply(d_x.data_ptr() + at * n_f * n_b * 4, n, st)
        orc.apply(want[at:at + n])
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_x.cpu().numpy()[:64]), bits(want[:64])) and inj.next_row == 64
    # every apply has ended: the next pulses' tables go into the spent ones' device allocations, and the rows still come out right
    for t0, W in ((70, 4), (66, 8)):
        t = tab(W)
        assert inj.add_burst(t0, *t) == orc.add_burst(t0, *t)
    inj.apply(d_x.data_ptr() + 64 * n_f * n_b * 4, 32, st)
    orc.apply(want[64:96])
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_x.cpu().numpy()), bits(want)) and inj.next_row == 96 and not np.array_equal(bits(want[64:]), bits(x[64:]))
    # ---- five trains: the fifth is refused
    inj2 = api.Injector(bf, n_f, 32, max_pulses=8, max_width=8)
    for k in range(4):
        inj2.add_train((0, 1 << 60, 0, 0), *tab(), first_row=k)
    with pytest.raises(bfmod.DsabfError, match="trains are alive") as e:
        inj2.add_train((0, 1 << 60, 0, 0), *tab())
    assert e.value.code == BF_ERR_STATE
    # ---- BF_ERR_INVALID, nothing stored or launched
    d, p, r = tab()
    pid = C.c_uint64()
    before = inj2.launches
    for args in ((-1, 4, d, p, r), (0, 0, d, p, r), (0, 9, d, p, r), (0, 4, None, p, r), (0, 4, d, None, r), (0, 4, d, p, None),
                 (0, 4, np.array([0, -1], np.int32), p, r)):
        ptrs = [a.ctypes.data if a is not None else None for a in args[2:]]
        assert lib.bf_inj_add_burst(inj2._c, args[0], args[1], *ptrs, C.byref(pid)) == BF_ERR_INVALID, args[:2]
    m = _lib.BfPsrModel(0, 1 << 60, 0, 0)
    for n_bins, n_rows, model in ((1, 5, m), (9, 5, m), (4, 0, m), (4, 5, None)):
        assert lib.bf_inj_add_train(inj2._c, C.byref(model) if model else None, 0, n_rows, n_bins, d.ctypes.data, p.ctypes.data, r.ctypes.data,
                                    C.byref(pid)) == BF_ERR_INVALID, (n_bins, n_rows)
    for rows, n in ((d_x.data_ptr(), 0), (d_x.data_ptr(), 33), (d_x.data_ptr(), -1), (None, 4), (d_x.data_ptr() + 4, 4)):
        assert lib.bf_inj_apply(inj2._c, rows, n, None) == BF_ERR_INVALID, n
    assert inj2.launches == before and inj2.next_row == 0
    # a train that would reach |n| >= 2^31 on a row it covers is refused as the folder refuses a push
    inj3 = api.Injector(bf, n_f, 32, max_width=8)
    inj3.add_train((0, 1 << 60, 0, -(1 << 31) + 10), *tab())
    inj3.apply(d_x, 10, st)
    with pytest.raises(bfmod.DsabfError, match="2\\^31") as e:
        inj3.apply(d_x, 1, st)
    assert e.value.code == BF_ERR_INVALID and inj3.next_row == 10
    torch.cuda.synchronize()
    for s in (inj, inj2, inj3):
        s.close()
    bf.close()


# ---- 6. attached, and the point of it all -------------------------------------------------------------------------------------------
def _oracle_chain(orc, s, x, conditioned):
    """(rows the DM stage dedisperses, chunks [n_dm][T - D][b], candidates per push) of the oracle chain over the series x."""
    T, n = s["T"], s["push"]
    D = int(s["ladder"].max())
    if conditioned:
        c = cond_oracle.Conditioner(s["n_f"], s["n_b"], **s["cond"])
        x = np.concatenate([c.push(x[at:at + n]) for at in range(0, T, n)])
    ded = orc.dedisperse_dm(x, s["ladder"], T - D)
    search = sps_oracle.Search(ded, s["n_widths"], threshold=s["threshold"])
    per_push = []
    for at in range(0, T, n):
        lo, hi = max(0, at - D), max(0, at + n - D)
        per_push.append(search.push(hi - lo)["cands"] if hi > lo else None)
    return ded, per_push


def _as_records(cands):
    from dsabeamformer_amd.api import _candidate_dtype

    out = np.zeros(len(cands), _candidate_dtype())
    for i, c in enumerate(cands):
        out[i] = c
    return out


@pytest.mark.parametrize("conditioned", [False, True])
def test_attached_the_search_finds_the_injected_burst(torch, bfmod, orc, conditioned):
    """640 rows of N(0, 1) noise, 16 channels, 8 beams, a ladder of 8 trials, pushes of 64 rows; one burst on trial 5's delays at row
    301, fluence 6 per channel in beam 3.  First the condition on the input, by the oracle chain alone (inj_oracle -> orc.dedisperse_dm ->
    sps_oracle): the raw series has no candidate, the injected one has a candidate that bf_inj_match accepts at t_tol 0, dm_tol 0.  Then
    the device: chunks bit-equal to the chain's, candidates equal to it (snr to the 1e-9 of tests/test_gpu_sps.py), and Injector.match
    picks that candidate.  With a conditioner attached the chain runs cond_oracle over the injected rows; the "found" assertions
    belong to the unconditioned leg."""
    from dsabeamformer_amd import api

    s = inj_cases.found_case()
    s["cond"] = dict(baseline_pushes=3, zero_dm=True, auto_threshold=0.0)
    T, n_f, n_b, n_dm, n = s["T"], s["n_f"], s["n_b"], s["n_dm"], s["push"]
    x_inj = inj_oracle.inject(s["x"], [s["burst"]], cuts=[n] * (T // n))
    assert not any(_oracle_chain(orc, s, s["x"], False)[1])                        # the raw series: no candidate in any push
    _, found = _oracle_chain(orc, s, x_inj, False)
    every = [c for push in found if push for c in push]
    assert len(every) == 1 and every[0][:4] == (304, 5, 3, 2) and 9.0 < every[0][5] < 10.0
    assert list(inj_oracle.match(s["truth"], _as_records(every))) == [0] and list(api.Injector.match(s["truth"], _as_records(every))) == [0]
    want_ded, want_cands = _oracle_chain(orc, s, x_inj, conditioned)
    # ---- the device
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=n_f))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_x = torch.from_numpy(s["x"]).cuda()
    torch.cuda.synchronize()
    dm = api.DmStream(bf, s["ladder"], n_f, n)
    inj = api.Injector(bf, n_f, n, max_width=s["W"])
    sps = api.SinglePulseSearch(bf, n_dm, s["n_widths"], n, threshold=s["threshold"])
    inj.add_burst(*s["burst"])
    dm.attach_injector(inj)
    if conditioned:
        cond = api.Conditioner(bf, n_f, n, **s["cond"])
        dm.attach_conditioner(cond)
    dm.attach_search(sps)
    with pytest.raises(bfmod.DsabfError, match="attached") as e:                   # the DM stage applies it now
        inj.apply(d_x, 1, 0)
    assert e.value.code == BF_ERR_STATE
    host = torch.zeros(n_dm * n * n_b, dtype=torch.float32).pin_memory()
    parts, got_cands = [], []
    for k, at in enumerate(range(0, T, n)):
        st = streams[k % 2]
        first_t, n_out = dm.push(d_x.data_ptr() + at * n_f * n_b * 4, n, host, st.cuda_stream)
        assert inj.next_row == at + n
        if not n_out:
            continue
        st.synchronize()
        parts.append(host[:n_dm * n_out * n_b].numpy().reshape(n_dm, n_out, n_b).copy())
        cands = sps.collect()
        sps_oracle.assert_candidates_equal(cands, want_cands[k], rtol=1e-9)
        got_cands.append(cands)
    torch.cuda.synchronize()
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(want_ded))
    assert inj.launches == 2                       # the burst's rows 301 .. 383 lie in the pushes [256, 320) and [320, 384)
    assert np.array_equal(bits(d_x.cpu().numpy()), bits(s["x"]))                   # the caller's rows stay raw
    got_cands = np.concatenate(got_cands)
    if not conditioned:
        best = api.Injector.match(s["truth"], got_cands)
        assert len(got_cands) == 1 and list(best) == [0]
        c = got_cands[0]
        assert (int(c["t_start"]), int(c["dm"]), int(c["beam"]), int(c["width"])) == (304, 5, 3, 2)
    for stage in (sps, inj, dm) + ((cond,) if conditioned else ()):
        stage.close()
    bf.close()


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------------------
def test_lifetime_and_attach_conditions(torch, bfmod):
    from dsabeamformer_amd import api

    n_b, n_f, max_rows = 8, 5, 4
    bf = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    other = bfmod.Beamformer(bfmod.debug_config(n_beams=n_b, n_freq=8))
    delays = np.zeros((2, n_f), np.int32)
    x = inj_cases.wide(np.random.default_rng(3), (2 * max_rows, n_f, n_b))
    d_x = torch.from_numpy(x).cuda()
    tab = (np.zeros(n_f, np.int32), np.ones((n_f, 2), np.float32), np.ones(n_b, np.float32))
    # ---- a mismatched attach
    dm = api.DmStream(bf, delays, n_f, max_rows)
    for bad, msg, code in ((api.Injector(bf, n_f + 1, max_rows), "channels", BF_ERR_INVALID), (api.Injector(bf, n_f, max_rows - 1), "max_rows_per_push", BF_ERR_INVALID),
                           (api.Injector(other, n_f, max_rows), "different handles", BF_ERR_INVALID)):
        with pytest.raises(bfmod.DsabfError, match=msg) as e:
            dm.attach_injector(bad)
        assert e.value.code == code
        bad.close()
    ahead = api.Injector(bf, n_f, max_rows)                                        # it has applied rows the DM stage has not been pushed
    ahead.apply(d_x, 2, 0)
    with pytest.raises(bfmod.DsabfError, match="has applied 2 rows") as e:
        dm.attach_injector(ahead)
    assert e.value.code == BF_ERR_STATE
    ahead.close()
    inj = api.Injector(bf, n_f, max_rows)
    dm.attach_injector(inj)
    dm.attach_injector(inj)                                                         # again: nothing changes
    dm2 = api.DmStream(bf, delays, n_f, max_rows)
    with pytest.raises(bfmod.DsabfError, match="another DM stage") as e:
        dm2.attach_injector(inj)
    assert e.value.code == BF_ERR_STATE
    # ---- destroying an attached injector detaches it: the DM stage goes on, raw
    inj.add_burst(0, *tab)
    inj.close()
    host = torch.zeros(2 * max_rows * n_b, dtype=torch.float32).pin_memory()
    assert dm.push(d_x, max_rows, host, 0) == (0, max_rows)
    torch.cuda.synchronize()
    want = np.zeros((max_rows, n_b), np.float32)
    for f in range(n_f):
        want = want + x[:max_rows, f, :]
    assert np.array_equal(bits(host[:max_rows * n_b].numpy().reshape(max_rows, n_b)), bits(want))
    # ---- detached by hand it applies on its own again, from the row it had reached
    inj = api.Injector(bf, n_f, max_rows)
    inj.apply(d_x, max_rows, 0)
    dm.attach_injector(inj)
    dm.attach_injector(None)
    inj.apply(d_x, 1, 0)
    assert inj.next_row == max_rows + 1
    # ---- the handle destroyed before the stage: BF_ERR_STATE, and the stage can still be destroyed
    dm.attach_injector(None)
    inj2 = api.Injector(bf, n_f, max_rows)
    torch.cuda.synchronize()
    bf.close()
    for call in (lambda: inj2.apply(d_x, 1, 0), lambda: inj2.add_burst(0, *tab), lambda: inj2.add_train((0, 1, 0, 0), *tab),
                 lambda: dm.attach_injector(inj2), lambda: dm2.attach_injector(None)):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE
    for stage in (inj, inj2, dm, dm2):
        stage.close()
    other.close()


# ---- 8. `beam` end to end -----------------------------------------------------------------------------------------------------------
BEAM_T0, BEAM_W, BEAM_BEAM, BEAM_FLUENCE, BEAM_TSAMP = 356, 8, 3, 2.0e5, 0.02
TRAIN_F0, TRAIN_BEAM, TRAIN_AMP, TRAIN_DUTY, TRAIN_BINS = 400.0, 5, 3.0e4, 0.05, 64      # a period of 125 rows of 0.02 ms; 3 bins on


def test_beam_injects_and_finds_the_burst(tmp_path, orc):
    """`beam -j 27 -M 40 -N 4 -T 0.02 -S 8 -B 5 -w raw.bin -C cands.txt --inject 356:<trial 2's DM>:3:2e5:1:8 --inject-train
    400:<trial 1's DM>:5:3e4 --inject-out truth.txt`: 25 burn-in reads + 2 analysed blocks of 256 rows, a burst and a pulse train.  The -w file keeps the RAW stream of the junk source's blocks (the host copies are queued in front
    of the push that injects).  On it, by the oracle chain alone (inj_oracle -> orc.dedisperse_dm -> sps_oracle, the chunk boundaries
    of run_observation): the raw rows give no candidate that matches the truth, the injected rows give one -- the fluence, 2e5 per
    channel against a cell noise of 1.7e4, is fixed by that.  Then cands.txt must hold the chain's candidates, the truth file must
    parse with its trial equal to nearest_trial, and Injector.match must pick the same candidate from the file as from the chain."""
    from dsabeamformer_amd import api, build, host

    raw_file, cand_file, truth_file = tmp_path / "raw.bin", tmp_path / "cands.txt", tmp_path / "truth.txt"
    dms, freq, ladder = dm_side.beam_ladder(40.0, 4, 256, BEAM_TSAMP)                # what `beam -M 40 -N 4 -T 0.02` picks
    dm = float(dms[2])
    r = subprocess.run([build.BEAM, "-j", "27", "-M", "40", "-N", "4", "-T", str(BEAM_TSAMP), "-S", "8", "-B", "5", "-w", str(raw_file), "-C", str(cand_file),
                        "--inject", "%d:%.17g:%d:%.17g:1:%d" % (BEAM_T0, dm, BEAM_BEAM, BEAM_FLUENCE, BEAM_W),
                        "--inject-train", "%.17g:%.17g:%d:%.17g" % (TRAIN_F0, float(dms[1]), TRAIN_BEAM, TRAIN_AMP), "--inject-out", str(truth_file)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    # the train's launch in both pushes, the burst's in the second
    assert "Injector: 1 bursts and 1 trains added to the rows in front of the DM stage, 3 kernels launched" in r.stdout
    # ---- the truth file
    lines = [l.split() for l in open(truth_file).read().splitlines() if not l.startswith("#")]
    assert len(lines) == 2 and lines[0][:2] == ["0", "burst"] and lines[1][:2] == ["1", "train"]
    assert [float(v) for v in lines[1][2:4]] == [TRAIN_F0, float(dms[1])] and [int(v) for v in lines[1][4:6]] == [1, TRAIN_BEAM]
    assert [float(v) for v in lines[1][6:8]] == [TRAIN_AMP, TRAIN_DUTY] and int(lines[1][8]) == TRAIN_BINS
    t0, trial, beam, W, t_lo, t_hi = int(lines[0][2]), int(lines[0][4]), int(lines[0][5]), int(lines[0][8]), int(lines[0][9]), int(lines[0][10])
    assert (t0, beam, W, t_lo, t_hi) == (BEAM_T0, BEAM_BEAM, BEAM_W, BEAM_T0, BEAM_T0 + BEAM_W - 1)
    assert float(lines[0][3]) == dm and float(lines[0][6]) == BEAM_FLUENCE and float(lines[0][7]) == 1.0
    raw = dm_side.read_rows(raw_file)
    rows = raw.shape[0] // 2
    assert raw.shape == (512, 256, 256)
    delay = host.dm_delays(np.array([dm]), freq, float(freq[0]), BEAM_TSAMP)[0]
    assert trial == api.Injector.nearest_trial(ladder, delay) == inj_oracle.nearest_trial(ladder, delay) == 2
    truth = [(t_lo, t_hi, trial, beam)]
    # ---- the oracle chain over the raw rows: the condition on the input
    D = int(ladder.max())

    def chain(x):
        search = sps_oracle.Search(orc.dedisperse_dm(x, ladder, x.shape[0] - D), 5, threshold=8.0)
        return [c for at in (0, rows) for c in search.push(max(0, at + rows - D) - max(0, at - D))["cands"]]

    assert list(inj_oracle.match(truth, _as_records(chain(raw)), t_tol=2, dm_tol=1)) == [-1]
    # (the tables the driver made, with the same helpers, and inj_oracle over them: tests/support/dm_side.py, shared with
    #  tests/test_gpu_trial_split.py)
    want = chain(dm_side.injected_rows(raw, rows, freq, BEAM_TSAMP, [(t0, dm, beam, BEAM_FLUENCE, 1.0, W)],
                                       [(TRAIN_F0, float(dms[1]), TRAIN_BEAM, TRAIN_AMP, TRAIN_DUTY, TRAIN_BINS)]))
    best = inj_oracle.match(truth, _as_records(want), t_tol=0, dm_tol=0)
    print("chain:", len(want), "candidates,", sum(c[2] == TRAIN_BEAM for c in want), "of them in the train's beam; the burst's:", want[best[0]] if best[0] >= 0 else None)
    assert best[0] >= 0 and want[best[0]][5] >= 8.0
    # ---- the driver found the same
    got = dm_side.read_candidates(cand_file)
    sps_oracle.assert_candidates_equal(got, want, rtol=1e-9)
    assert list(api.Injector.match(truth, got)) == list(best)


def test_beam_shards_inject_the_whole_band_redundantly(tmp_path):
    """`beam … -R 2 -r <rank> -X -S 8 -B 5 -C cands.txt --inject 356:<trial 4's DM>:3:2e5:1:8 --inject-out truth.txt` as two loopback shard
    processes: the band is gathered to both, the six trials are split, and BOTH ranks inject the whole band where they dedisperse it.
    Each writes the same truth to truth.txt.<rank> (the trial numbered over the whole ladder); the rank that owns trial 4 finds the
    burst there, the other rank's trials hold nothing that matches it at dm_tol 0."""
    from dsabeamformer_amd import api, build

    FAKE = dm_side.fake_rccl()                                                       # (built here if no test has built it yet)
    dms, _, _ = dm_side.beam_ladder(40.0, 6, 256, BEAM_TSAMP)                        # what `beam -M 40 -N 6` picks
    cands, truth_file = tmp_path / "cands.txt", tmp_path / "truth.txt"
    cmd = lambda rk: [build.BEAM, "-j", "27", "-D", "0", "-M", "40", "-N", "6", "-T", str(BEAM_TSAMP), "-R", "2", "-r", str(rk), "-I", str(tmp_path / "id"),  # noqa: E731
                      "-X", "-S", "8", "-B", "5", "-C", str(cands), "--inject", "%d:%.17g:%d:%.17g:1:%d" % (BEAM_T0, float(dms[4]), BEAM_BEAM, BEAM_FLUENCE, BEAM_W),
                      "--inject-out", str(truth_file)]
    procs = [subprocess.Popen(cmd(rk), env=dict(os.environ, DSABF_RCCL_LIB=FAKE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rk in (0, 1)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    lines = [open(str(truth_file) + ".%d" % rk).read() for rk in (0, 1)]
    assert lines[0] == lines[1] and not os.path.exists(truth_file)
    rec = [l.split() for l in lines[0].splitlines() if not l.startswith("#")]
    assert len(rec) == 1 and rec[0][:3] == ["0", "burst", str(BEAM_T0)] and int(rec[0][4]) == 4 and int(rec[0][5]) == BEAM_BEAM
    truth = [(int(rec[0][9]), int(rec[0][10]), int(rec[0][4]), int(rec[0][5]))]
    for rk in (0, 1):
        assert ("Shard %d dedisperses trials %d .. %d" % (rk, 3 * rk, 3 * rk + 2)) in outs[rk]
        assert "Injector: 1 bursts and 0 trains added to the rows in front of the DM stage, 1 kernels launched" in outs[rk], outs[rk]
        got = dm_side.read_candidates(str(cands) + ".%d" % rk)
        best = api.Injector.match(truth, got)
        print("rank %d: %d candidates, the burst's: %s" % (rk, len(got), got[best[0]] if best[0] >= 0 else None))
        assert (best[0] >= 0) == (rk == 1)
        if rk == 1:
            assert int(got[best[0]]["dm"]) == 4 and got[best[0]]["snr"] >= 8.0
